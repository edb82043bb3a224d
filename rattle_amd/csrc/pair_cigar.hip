// Kernel F: the CIGAR of every pair kernel E aligned (include/rattle_hip.h, "align_cigars"; DESIGN.md, "Kernel F").
//
// Kernel E's record gives a pair its rectangle on the aligned strand: `rows` read bases from the alignment's first to its last, `cols`
// transcript bases likewise.  The same recurrence over the rectangle alone (zeros on its top row and left column) reproduces the full
// matrix on every cell of the chosen path and is nowhere larger (DESIGN.md states the lemma, tests/test_cigar_ref.py checks it), so a walk
// back from the rectangle's last cell is the walk of the full matrix and ends at the rectangle's first cell.
//
// Forward pass: one wavefront per pair, kernel E's skewed form -- lane l owns row 64 b + l of block b, at step s it computes column s - l --
// with the score alone: `up` and the sliding letter by the DPP wave_shr:1, lane 0's `up` from the pair's hand-over strip (4 bytes per
// column, read 64 columns at a time one refill ahead, updated in place behind the reads as in kernel E).  Each cell's decision is a 2-bit
// code (0 zero cell: the path stops, 1 diagonal, 2 up, 3 left), from kernel E's selects.  Two ballots per step, the low and the high bit,
// make the 16-byte record of (block, step): an anti-diagonal of 64 cells.  Lane k keeps the record of step S + k of the current 64 steps,
// and the 64 records go out as one coalesced store; lane 63's scores for the strip leave the same way.  A block's records lie cols + 63
// apart.
//
// Walk: the same wavefront, after a device-scope fence.  The state (block, lane, column) is wave-uniform.  A window holds 64 consecutive
// records of one block, one per lane; every lane shifts the walk's row out of its own record, and v_readlane by the step's index fetches
// the code: a diagonal move goes back two steps, up and left one, up out of lane 0 goes to lane 63 of the block above (a new window).  The
// letters at a diagonal cell come from two windows of the same kind (the block's 64 read bases, 64 transcript bases).  Runs are merged in
// scalar registers; lane 0 writes a finished run as len << 4 | op (BAM's numbers) from the end of the pair's ops region backwards, so the
// ops lie in start-to-end order, and the run count beside them.
//
// Bounds: every loop runs over the pair's own lengths -- the walk makes at most rows + cols moves whatever the codes say, the window
// index is step - window start in [0, 64) by construction -- and every load and store lies in the pair's own sequences, strip, records,
// ops region or count.  A wrong code gives a wrong string, never a hang or a store out of range.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "cigar_plan.h"
#include "common.h"

namespace rattle {

namespace {

constexpr int32_t CG_MATCH = 5, CG_MISMATCH = -4, CG_GAP = -8;
constexpr uint32_t CG_OP_I = 1, CG_OP_D = 2, CG_OP_EQ = 7, CG_OP_X = 8;      // BAM's numbers
constexpr uint32_t CG_MAX_RUN = 0x0FFFFFFFu;                                  // 28 bits of length: a longer run is written in pieces

// value of lane - 1 (lane 0 receives `fill`): the helper of pair_align.hip
__device__ __forceinline__ int32_t cg_shr1(int32_t v, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
}

// A 0, C 1, G 2, T and U 3 (the complement of code c is 3 - c); the host has refused every other byte
__device__ __forceinline__ int32_t cg_code(uint32_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3; }

__device__ __forceinline__ uint32_t cg_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v); }

__global__ __launch_bounds__(256) void pair_cigar_kernel(const cigar_pair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qseq,
                                                         const uint8_t *__restrict__ tseq, uint4 *__restrict__ codes, int32_t *__restrict__ strips,
                                                         uint32_t *__restrict__ ops, uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const cigar_pair P = pairs[p];
    const uint32_t sq = cg_uniform(P.rows), st = cg_uniform(P.cols), rev = cg_uniform(P.rev);
    // row r of the rectangle is read base q[r] (forward) or the complement of q[-r] (reverse: q points at the last base of the span)
    const uint8_t *q = qseq + P.q, *t = tseq + P.t;
    uint4 *code = codes + P.codes;
    int32_t *strip = strips + P.strip;
    uint32_t *op = ops + P.ops;
    const uint64_t stride = (uint64_t)st + CG_ROWS - 1;               // records of one block

    // ---- forward: the codes of every cell of the rectangle ----
    for (uint32_t r0 = 0, b = 0; r0 < sq; r0 += CG_ROWS, ++b) {
        const uint32_t r = r0 + lane;                                // the lane's row
        const bool row = r < sq;
        int32_t ql = 4;                                              // (matches nothing)
        if (row) ql = rev ? 3 - cg_code(*(q - r)) : cg_code(q[r]);
        const bool from_strip = r0 > 0, to_strip = r0 + CG_ROWS < sq;
        const uint32_t n_steps = st + min(CG_ROWS, sq - r0) - 1;     // the block's last row computes its last column at the last step
        uint4 *rec_b = code + (uint64_t)b * stride;
        int32_t cH = 0, dH = 0, tl = 4;                              // the lane's previous cell (left), lane - 1's as received one step ago (diag)
        // refill in flight: the transcript's letters and the strip's scores of columns [S + 64, S + 128)
        int32_t nT = 4, nS = 0;
        if (lane < st) { nT = cg_code(t[lane]); if (from_strip) nS = strip[lane]; }
        for (uint32_t S = 0; S < n_steps; S += 64) {
            const int32_t bT = nT, bS = nS;
            nT = 4; nS = 0;
            if (S + 64 + lane < st) { nT = cg_code(t[S + 64 + lane]); if (from_strip) nS = strip[S + 64 + lane]; }
            const uint32_t k_end = min(64u, n_steps - S);
            uint4 rec = make_uint4(0, 0, 0, 0);                      // lane k: the record of step S + k
            int32_t last = 0;                                        // lane k: lane 63's score after step S + k, column S + k - 63
            for (uint32_t k = 0; k < k_end; ++k) {
                const uint32_t s = S + k;
                // lane 0's up cell and letter: column s of the buffers (zeros on the first block and beyond the transcript's end)
                const int32_t fT = __builtin_amdgcn_readlane(bT, k), fH = __builtin_amdgcn_readlane(bS, k);
                const int32_t uH = cg_shr1(cH, fH);
                tl = cg_shr1(tl, fT);
                const uint32_t c = s - lane;                         // the lane's column (wraps below 0: fails the test)
                const bool on = row && c < st;
                const int32_t d = dH + (ql == tl ? CG_MATCH : CG_MISMATCH), u = uH + CG_GAP, l = cH + CG_GAP;
                const int32_t h = max(max(d, 0), max(u, l));
                const uint32_t cd = !on || h == 0 ? 0u : d >= u && d >= l ? 1u : u >= l ? 2u : 3u;      // diagonal, then up, then left
                dH = uH;
                if (on) cH = h;
                const uint64_t lo = __ballot(cd & 1u), hi = __ballot(cd & 2u);
                const bool mine = lane == k;
                rec.x = mine ? (uint32_t)lo : rec.x; rec.y = mine ? (uint32_t)(lo >> 32) : rec.y;
                rec.z = mine ? (uint32_t)hi : rec.z; rec.w = mine ? (uint32_t)(hi >> 32) : rec.w;
                if (to_strip) { const int32_t h63 = __builtin_amdgcn_readlane(cH, 63); last = mine ? h63 : last; }
            }
            if (lane < k_end) {
                rec_b[S + lane] = rec;                               // S + lane < n_steps <= stride
                const uint32_t cc = S + lane - 63;                   // lane 63's column at that step (wraps below 0: fails the test)
                if (to_strip && S + lane >= 63 && cc < st) strip[cc] = last;      // behind every read of the strip: columns <= S were loaded a refill ago
            }
        }
        __threadfence();                                             // the strip's stores of this block before the next block's loads; the records before the walk
    }

    // ---- walk: from the rectangle's last cell back to its first ----
    uint32_t b = (sq - 1) >> 6, L = (sq - 1) & 63u, c = st - 1;      // block, lane (row 64 b + L), column
    const uint32_t region = sq + st;                                 // words of the ops region = the most moves a path can make
    uint32_t pos = region, run_op = 0, run_len = 0;
    uint32_t wb = ~0u, W = 0, qb = ~0u, T0 = ~0u;                    // the windows: block and first step of the records, block of the read bases, first column
    uint4 win = make_uint4(0, 0, 0, 0);
    int32_t qw = 4, tw = 4;
    for (uint32_t m = 0; m < region; ++m) {
        const uint32_t s = c + L;
        if (b != wb || s < W || s - W >= 64) {                       // records [W, W + 64) of block b, W + 63 = s unless the block begins before
            wb = b; W = s >= 63 ? s - 63 : 0;
            win = make_uint4(0, 0, 0, 0);
            if (W + lane <= s) win = code[(uint64_t)b * stride + W + lane];
        }
        const uint32_t lo = L < 32 ? win.x : win.y, hi = L < 32 ? win.z : win.w;
        const uint32_t mine = ((lo >> (L & 31u)) & 1u) | (((hi >> (L & 31u)) & 1u) << 1);
        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int32_t)mine, s - W);
        if (cd == 0) break;                                          // a zero cell: the path begins behind it
        uint32_t o = cd == 2 ? CG_OP_I : CG_OP_D;
        if (cd == 1) {
            if (b != qb) {
                qb = b; qw = 4;
                const uint32_t r = b * CG_ROWS + lane;
                if (r < sq) qw = rev ? 3 - cg_code(*(q - r)) : cg_code(q[r]);
            }
            if (c < T0 || c - T0 >= 64) {
                T0 = c >= 63 ? c - 63 : 0; tw = 4;
                if (T0 + lane <= c) tw = cg_code(t[T0 + lane]);
            }
            o = __builtin_amdgcn_readlane(qw, L) == __builtin_amdgcn_readlane(tw, c - T0) ? CG_OP_EQ : CG_OP_X;
        }
        if (o == run_op && run_len < CG_MAX_RUN) ++run_len;
        else {
            if (run_len && pos) { --pos; if (lane == 0) op[pos] = run_len << 4 | run_op; }
            run_op = o; run_len = 1;
        }
        bool done = false;
        if (cd != 3) { if (L) --L; else if (b) { --b; L = 63; } else done = true; }      // up out of lane 0: lane 63 of the block above
        if (cd != 2) { if (c) --c; else done = true; }
        if (done) break;                                             // the rectangle's top row or left column
    }
    if (run_len && pos) { --pos; if (lane == 0) op[pos] = run_len << 4 | run_op; }
    if (lane == 0) counts[p] = region - pos;
}

// ops [region - count, region) of every pair's region to out[off[p] ..): one wavefront per pair
__global__ __launch_bounds__(256) void cigar_gather_kernel(const cigar_pair *__restrict__ pairs, uint32_t n_pairs, const uint64_t *__restrict__ off,
                                                           const uint32_t *__restrict__ ops, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;
    const uint32_t region = pairs[p].rows + pairs[p].cols;
    const uint64_t a = off[p], n = off[p + 1] - a;                   // n <= region: the host has seen to it
    const uint32_t *src = ops + pairs[p].ops + (region - n);
    for (uint64_t k = lane; k < n; k += 64) out[a + k] = src[k];
}

}  // namespace

uint64_t cigar_code_cap() {
    const char *v = getenv("RATTLE_CIGAR_CODE_BYTES");               // (tests lower the cap to see a chunk split)
    return v ? std::max<uint64_t>(1, strtoull(v, nullptr, 10)) : CG_CODE_CAP;
}

// The pairs `in` of one chunk of kernel E, whose sequences lie in d_q and d_t: the ops of every pair with status 0 appended to R.ops, their
// number to R.count[read].  Sub-chunks as cigar_plan.h plans them; per sub-chunk one launch of kernel F (id 7 of the stats), the counts to
// the host, offsets from them, one gather launch, and the compact ops back.  With `scoring` the launch is that of the three-state kernel
// (pair_cigar_affine.hip, id 9): 32-byte records, two strip words per column; everything around it is the same.
int pair_cigar_chunk(rattle_ctx *ctx, const uint8_t *d_q, const uint8_t *d_t, const cigar_in *in, uint32_t n, uint32_t pair_chunk, cigar_run &R,
                     const rattle_align_scoring *scoring) {
    const uint64_t rec_bytes = scoring ? CG_AFFINE_REC_BYTES : CG_REC_BYTES;
    const int kid = scoring ? K_CIGAR_AFFINE : K_CIGAR;
    std::vector<uint8_t> status(n);
    std::vector<uint32_t> rows(n), cols(n);
    for (uint32_t i = 0; i < n; ++i) { status[i] = in[i].status; rows[i] = in[i].rows; cols[i] = in[i].cols; }
    cigar_plan plan;
    plan_cigar(status.data(), rows.data(), cols.data(), n, pair_chunk, R.code_cap, plan, rec_bytes, scoring ? CG_AFFINE_STRIP_WORDS : 1);
    for (size_t c = 0; c + 1 < plan.first.size(); ++c) {
        const uint32_t a = plan.first[c], m = plan.first[c + 1] - a;
        RT_TRY(R.h_pairs.reserve(m));
        uint64_t recs = 0, strip = 0, words = 0, alg = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const cigar_in &I = in[plan.sub[a + i]];
            cigar_pair &P = R.h_pairs.p[i];
            P.q = I.q; P.t = I.t; P.codes = recs; P.strip = strip; P.ops = words;
            P.rows = I.rows; P.cols = I.cols; P.rev = I.rev; P.pad = 0;
            recs = cg_add(recs, plan.recs[a + i]); strip += plan.strip[a + i]; words += plan.ops[a + i];
            // the rectangle's sequence bytes, the code records written (a block of h rows writes cols + h - 1 of them), the count
            const uint64_t blocks = ((uint64_t)I.rows + CG_ROWS - 1) / CG_ROWS;
            alg += (uint64_t)I.rows + I.cols + rec_bytes * (blocks * ((uint64_t)I.cols - 1) + I.rows) + 4;
        }
        if (recs > (~0ull >> 8)) { set_error("align_cigars: out of memory (the code records of one pair)"); return RATTLE_ERR_HIP; }
        RT_TRY(R.d_pairs.reserve(m));
        RT_TRY(R.d_codes.reserve(recs * (rec_bytes / sizeof(uint4))));
        RT_TRY(R.d_strip.reserve(std::max<uint64_t>(1, strip)));
        RT_TRY(R.d_ops.reserve(words));
        RT_TRY(R.d_count.reserve(m));
        RT_TRY(R.h_count.reserve(m));
        RT_TRY(R.d_off.reserve((size_t)m + 1));
        RT_TRY(R.h_off.reserve((size_t)m + 1));
        RT_HIP(hipMemcpyAsync(R.d_pairs.p, R.h_pairs.p, (size_t)m * sizeof(cigar_pair), hipMemcpyHostToDevice, ctx->stream));
        {
            ktimer kt(ctx, kid, alg);
            if (scoring) pair_cigar_affine_launch(ctx->stream, R.d_pairs.p, m, d_q, d_t, R.d_codes.p, R.d_strip.p, R.d_ops.p, R.d_count.p, *scoring);
            else hipLaunchKernelGGL(pair_cigar_kernel, dim3((m + 3) / 4), dim3(256), 0, ctx->stream, R.d_pairs.p, m, d_q, d_t, R.d_codes.p, R.d_strip.p,
                               R.d_ops.p, R.d_count.p);
            RT_HIP(hipGetLastError());
        }
        RT_HIP(hipMemcpyAsync(R.h_count.p, R.d_count.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
        uint64_t total = 0;
        for (uint32_t i = 0; i < m; ++i) {                           // (a count is never trusted beyond the pair's region)
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(R.h_count.p[i], plan.ops[a + i]);
            R.h_off.p[i] = total;
            R.count[in[plan.sub[a + i]].read] = cnt;
            total += cnt;
        }
        R.h_off.p[m] = total;
        ctx->stats[kid].bytes += 4 * total;                      // ... and 4 bytes per op
        if (!total) continue;
        RT_TRY(R.d_out.reserve(total));
        RT_TRY(R.h_out.reserve(total));
        RT_HIP(hipMemcpyAsync(R.d_off.p, R.h_off.p, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(cigar_gather_kernel, dim3((m + 3) / 4), dim3(256), 0, ctx->stream, R.d_pairs.p, m, R.d_off.p, R.d_ops.p, R.d_out.p);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpyAsync(R.h_out.p, R.d_out.p, total * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
        R.ops.insert(R.ops.end(), R.h_out.p, R.h_out.p + total);
    }
    return 0;
}

}  // namespace rattle
