// Kernel G: what the aligned reads say about every base of every transcript (include/rattle_hip.h, "align_pileup"; DESIGN.md, "Kernel G";
// tests/pileup_ref.py is the contract).  It runs behind kernel F's gather (pair_cigar.hip) on the same stream, over what that left on the
// device: the compact ops of a sub-chunk's pairs, out[off[p] .. off[p + 1]) each len << 4 | op from the alignment's start to its end, the
// cigar_pair records (where the rectangle's first row and first column lie, rows, cols, strand) and the read bytes.  It adds into the
// call's table, which is PLANAR: eight arrays of `plane` uint32 -- A, C, G, T, del, ins, starts, ends -- over the uploaded targets, so that
// the 64 lanes of a wavefront on 64 consecutive columns of an '=' run add into at most four contiguous segments, one per letter, instead
// of 64 rows of 32 bytes with one lane each.  The counts are integers: the sums do not depend on the order of the adds.
//
// One wavefront per pair.  A round takes 64 ops, one per lane, and scans their advances -- alignment columns, read rows, target columns --
// across the wave, which gives every op the alignment column, the row and the target position it begins at.  The lane that holds an I op
// that is neither the first nor the last op of the pair adds 1 to `ins` at its position: an I run consumes no target column, so that is
// the position of the column behind it.  Then the round's alignment columns are taken 64 at a time, one per lane: a binary search over the
// 64 scanned starts (six ds_bpermute) finds the column's op, its offset in the op gives the row and the position; a column of '=' or 'X'
// reads its read base as kernel F addresses it (q[r], on the reverse strand the complement of q[-r], U as T) and adds 1 to that letter's
// plane, a column of 'D' adds 1 to `del`, a column of 'I' adds nothing.  Lane 0 adds `starts` at the rectangle's first column and `ends`
// at its last.  (A run of 2^28 columns or more comes in pieces, pair_wave.h: its ops are adjacent I ops and would count once each.  No
// input within the library's other limits reaches that.)
//
// Bounds: every loop runs over the pair's own op count and lengths.  The op count is cut at rows + cols, the words of the pair's ops
// region; the alignment columns of all rounds together are cut at rows + cols too, which is the most a valid CIGAR has (the scan of the
// columns saturates, so a sum that does not fit 32 bits is still larger than the cut); so a pair costs at most (rows + cols) / 64 rounds
// and as many column steps more, whatever the ops say.  Every target position is checked against `cols` and every row against `rows`
// before the load or the add; the host has checked that every rectangle's columns lie inside a plane.  An op code other than the four
// advances nothing.  A wrong op gives wrong counts, never a store out of range or a hang.
#include "common.h"
#include "pair_wave.h"

namespace rattle {

namespace {

constexpr uint32_t PU_DEL = 4, PU_INS = 5, PU_STARTS = 6, PU_ENDS = 7;         // the planes behind the four letters' (pw_code)

__device__ __forceinline__ uint32_t pu_sat_add(uint32_t a, uint32_t b) { const uint32_t s = a + b; return s < a ? ~0u : s; }

__global__ __launch_bounds__(256) void pair_pileup_kernel(const cigar_pair *__restrict__ pairs, uint32_t n_pairs, const uint64_t *__restrict__ off,
                                                          const uint32_t *__restrict__ ops, const uint8_t *__restrict__ qseq, uint32_t *table,
                                                          uint64_t plane) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const cigar_pair P = pairs[p];
    const uint32_t rows = pw_uniform(P.rows), cols = pw_uniform(P.cols), rev = pw_uniform(P.rev);
    if (!cols) return;                                               // (never planned: nothing to count)
    const uint64_t a0 = off[p];
    const uint32_t region = rows + cols;                             // both below 2^31
    const uint32_t n_ops = pw_uniform((uint32_t)min(off[p + 1] - a0, (uint64_t)region));
    const uint32_t *src = ops + a0;
    const uint8_t *q = qseq + P.q;                                   // row r: q[r], or on the reverse strand the complement of q[-r]
    uint32_t *tab = table + P.t;                                     // position j of the rectangle in plane k: tab[k * plane + j], j < cols
    if (lane == 0) {
        atomicAdd(tab + PU_STARTS * plane, 1u);
        atomicAdd(tab + PU_ENDS * plane + (cols - 1), 1u);
    }
    uint32_t row0 = 0, col0 = 0;                                     // rows and target columns of the rounds before this one
    uint32_t budget = region;                                        // alignment columns the pair may still take
    for (uint32_t k0 = 0; k0 < n_ops && budget; k0 += min(64u, n_ops - k0)) {
        const uint32_t k = k0 + lane;                                // the op's index in the pair; used only where lane < n_ops - k0
        uint32_t len = 0, code = 0;
        if (lane < n_ops - k0) { const uint32_t o = src[k]; len = o >> 4; code = o & 15u; }
        const bool on_q = code == PW_OP_EQ || code == PW_OP_X || code == PW_OP_I, on_t = code == PW_OP_EQ || code == PW_OP_X || code == PW_OP_D;
        if (!on_q && !on_t) len = 0;
        // inclusive scans over the wave: alignment columns (saturating), rows, target columns (wrapping: checked where they are used)
        uint32_t ac = len, rw = on_q ? len : 0u, tc = on_t ? len : 0u;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t x = __shfl_up(ac, d), y = __shfl_up(rw, d), z = __shfl_up(tc, d);
            if (lane >= d) { ac = pu_sat_add(ac, x); rw += y; tc += z; }
        }
        const uint32_t before = __shfl_up(ac, 1);
        const uint32_t a_at = lane ? before : 0u;                    // the op's first alignment column in the round
        const uint32_t r_at = row0 + rw - (on_q ? len : 0u), t_at = col0 + tc - (on_t ? len : 0u);      // its first row, its position
        const uint32_t take = min((uint32_t)__builtin_amdgcn_readlane((int32_t)ac, 63), budget);
        budget -= take;
        if (code == PW_OP_I && len && k > 0 && lane + 1 < n_ops - k0 && t_at < cols) atomicAdd(tab + PU_INS * plane + t_at, 1u);
        for (uint64_t w = 0; w < take; w += 64) {
            const uint64_t a64 = w + lane;
            const uint32_t a = (uint32_t)min(a64, (uint64_t)take - 1);                 // every lane searches: the shuffles read all 64
            uint32_t at = 0;                                         // the last op that begins at or before column a (lane 0's begins at 0)
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t s = __shfl(a_at, (int)(at + step));   // at + step <= 63
                if (s <= a) at += step;
            }
            const uint32_t c = __shfl(code, (int)at), d = a - __shfl(a_at, (int)at);   // d < the op's length: the next op begins behind a
            const uint32_t r0 = __shfl(r_at, (int)at), j0 = __shfl(t_at, (int)at);
            if (a64 >= take) continue;
            if (c == PW_OP_EQ || c == PW_OP_X) {
                const uint32_t r = r0 + d, j = j0 + d;
                if (r < rows && j < cols) {
                    const uint32_t base = (uint32_t)(rev ? 3 - pw_code(*(q - r)) : pw_code(q[r]));
                    atomicAdd(tab + base * plane + j, 1u);
                }
            } else if (c == PW_OP_D) {
                const uint32_t j = j0 + d;
                if (j < cols) atomicAdd(tab + PU_DEL * plane + j, 1u);
            }
        }
        row0 += (uint32_t)__builtin_amdgcn_readlane((int32_t)rw, 63);
        col0 += (uint32_t)__builtin_amdgcn_readlane((int32_t)tc, 63);
    }
}

}  // namespace

// Kernel G over the m pairs of the sub-chunk whose gather has just been launched on ctx->stream: R.d_pairs, R.d_off and R.d_out as the
// gather uses them, the reads in d_q, into R.d_pileup.  One launch under id 11 of the stats with `alg` bytes.
int pair_pileup_launch(rattle_ctx *ctx, const cigar_run &R, uint32_t m, const uint8_t *d_q, uint64_t alg) {
    ktimer kt(ctx, K_PILEUP, alg);
    hipLaunchKernelGGL(pair_pileup_kernel, dim3((m + 3) / 4), dim3(256), 0, ctx->stream, R.d_pairs.p, m, R.d_off.p, R.d_out.p, d_q, R.d_pileup,
                       R.pileup_n);
    RT_HIP(hipGetLastError());
    return 0;
}

}  // namespace rattle
