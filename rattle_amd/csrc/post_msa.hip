// Kernel D: the post-MSA logic of `rattle correct` on the device, so MSA rows never leave HBM.
// Replaces /root/reference/correct.cpp:32-92 (fix_msa_ends), :94-193 (column vote) and :196-309
// (per-read correction); restated for the CPU in oracle/orc_correct.hpp.
//
// One 256-thread workgroup (four wavefronts) per pack, every step in wide passes:
//   a. expand: a wavefront per row builds the row of bases (and of quality bytes) in LDS -- '-' everywhere, then every base at the
//      MSA column kernel C assigned to it -- and writes it out in 16-byte lines; the first and last line of a row, shared with its
//      neighbours (rows are W bytes apart, whatever W is), leave byte by byte.  Rows wider than POST_STAGE_W: the matrix is filled
//      in 16-byte lines, then the bases are scattered;
//   b. fix ends: a wavefront per row runs the reference's scan from both ends (small leading blocks followed by a long gap are
//      blanked) over ballot masks of 64 cells, starting at the row's first / last base (its column is known: col[]); the row's
//      voting window [first, last] and the number of bases trimmed at each end are kept, the windows also in LDS;
//   c. vote: a thread per four adjacent columns (one 4-byte load of bases, one of quality bytes per row) walks the rows IN ROW ORDER
//      (the reference's accumulation order with one thread, so the double sums are bit-identical), then takes the means, the winner
//      in the reference's slot order with strict '>', the two occupancy tests and the quality symbol of the winner's mean error;
//   d. MODE 1 (after POA #1): a wavefront per row rewrites the read against the column winners, 256 columns a round: every lane
//      decides its columns, a ballot and a prefix count give the output position (in place: all loads of a round stand before its
//      stores, and the output cursor never passes the round's first column);
//      MODE 2 (after POA #2 / #3): the gap-stripped column winners are the pack consensus.
// The REPORT form of MODE 1 (rattle_hip_set_correction_report) also counts, per row, the columns of its window by the branch of step d
// that handled them: six counters per lane, summed over the wavefront once per row and stored next to olen.  It is an instance of its
// own.
// The REPORT form of MODE 2 (rattle_hip_set_consensus_support) keeps what the column vote knows about every base of the consensus: the
// winner's count and the number of rows that voted (step c, vote_support: uint32 per column), written by step d' at the compacted
// index of the base.  A pack below A.n_composed is a POA #3 pack: its rows are pack consensi that carry a support and a depth per
// base, counted in reads.  They are expanded beside the bases (step a, two uint32 matrices), the row's wavefront carries the depth forward
// into the gap cells of its window (step b), and the column's thread sums, in its row loop, the depth of every row whose window covers
// the column and the support of the rows per slot; the winner's sum is the support in reads.  Again an instance of its own: every
// line of it sits in an `if constexpr`.
//
// phred_symbol (utils.cpp:6-8) is `(char)(-10*log10(p)+33)`: the host libm's log10 decides the
// truncation, so the device does not evaluate log10 at all.  The host tabulates, for every integer n
// the expression can take, the smallest double p whose symbol value is <= n (bit-level bisection with
// the host's own log10, verified exhaustively in a window around every threshold, deviations kept as
// explicit exceptions) and the device bisects that table: bit-exact by construction.
//
// HBM traffic (algorithmic): per MSA cell 1 B (+1 B quality) written once by (a) and read by (c) and (d); (b) reads a few 64-cell
// blocks at either end of a row.
#include <cmath>
#include <cstring>

#include "common.h"

namespace rattle {

__device__ __forceinline__ uint8_t d_comp_base(uint8_t c) {                       // utils.hpp:8-14
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'T': return 'A';
        case 'G': return 'C';
        case 'U': return 'A';
    }
    return c;
}

// One wavefront per descriptor: dst[0..len) = src[0..len) or its reverse complement (qualities: reversed).
__global__ __launch_bounds__(256) void gather_kernel(const gather_desc *D, uint32_t n, const uint8_t *sseq, const uint8_t *squal,
                                                      uint8_t *dseq, uint8_t *dqual) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= n) return;
    const gather_desc d = D[w];
    if (d.flags & 1u) {
        for (uint32_t t = lane; t < d.len; t += 64) {
            const uint64_t s = d.src + d.len - 1 - t;
            dseq[d.dst + t] = d_comp_base(sseq[s]);
            if (dqual) dqual[d.dst + t] = squal[s];
        }
    } else {
        for (uint32_t t = lane; t < d.len; t += 64) {
            dseq[d.dst + t] = sseq[d.src + t];
            if (dqual) dqual[d.dst + t] = squal[d.src + t];
        }
    }
}

int launch_gather(rattle_ctx *ctx, const gather_desc *d_desc, uint32_t n, const uint8_t *sseq, const uint8_t *squal, uint8_t *dseq,
                  uint8_t *dqual) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(gather_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_desc, n, sseq, squal, dseq, dqual);
    RT_HIP(hipGetLastError());
    return 0;
}

// symbol value of a mean error: smallest n with p >= lo[n - n0]; exceptions override.
__device__ int phred_value(const post_args &A, double p) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(p);
    int a = 0, b = (int)A.n_exc;
    while (a < b) { const int m = (a + b) >> 1; if (A.exc_bits[m] < bits) a = m + 1; else b = m; }
    if (a < (int)A.n_exc && A.exc_bits[a] == bits) return A.exc_val[a];
    int lo = 0, hi = A.phred_cnt - 1;          // lo[] is non-increasing in n; p >= lo[cnt-1] always holds for valid input
    while (lo < hi) { const int m = (lo + hi) >> 1; if (p >= A.phred_lo[m]) hi = m; else lo = m + 1; }
    return A.phred_n0 + lo;
}

constexpr uint32_t POST_WAVES = 4;            // wavefronts of the workgroup: steps b and d give each of them a row at a time
constexpr uint32_t POST_WIN_ROWS = 1024;      // rows of a pack whose voting window step c finds in LDS (the rows behind them: in memory)
constexpr uint32_t POST_STAGE_W = 2048;      // widest row step a builds in LDS (wider rows: 16-byte fill, then the scatter)
constexpr int POST_VOTE_COLS = 4;             // adjacent columns per thread in step c: one dword of bases, one of quality bytes
constexpr int POST_FIX_BLOCKS = 4;            // 64-column blocks of a row that step d loads before it stores

__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    return v;
}

// One side of fix_msa_ends (correct.cpp:32-92) for one row by one wavefront: the reference's scan, cell for cell, over bits instead
// of bytes.  The wavefront reads 64 cells in one load and keeps `cell is a base` as a ballot mask, so every variable of the state
// machine is the same in all lanes.  Position p counts from the side the scan starts at (REV: column n - 1 - p).  `start` is a
// position at or before the side's first base (the cells in front of it are gaps: they only would be skipped); columns below `floor`
// read as gaps (phase 2 after phase 1: what phase 1 blanked lies in front of its stop, so nothing it stored is read back).
// Two shortcuts leave the outcome as it is: the block scan ends at its 10th base (sz only grows, and sz >= 10 stops the scan
// whatever follows), and the gap run behind a short block is counted up to 20 (the test is gaps >= 20; the rest of the run is
// skipped as the next block's leading gaps).  Blanking the block blanks the run too: its cells are gaps already.
template <bool REV>
__device__ void fix_wave(uint8_t *r, uint32_t n, uint32_t lane, uint32_t start, uint32_t floor, uint32_t &trimmed, uint32_t &stop_pos,
                         bool &stopped) {
    uint32_t wbase = 0;
    unsigned long long m = 0;
    bool loaded = false;
    auto base_at = [&](uint32_t p) -> bool {      // p < n
        if (!loaded || p - wbase >= 64u) {
            wbase = p & ~63u; loaded = true;
            const uint32_t q = wbase + lane;
            bool b = false;
            if (q < n) { const uint32_t c = REV ? n - 1u - q : q; b = c >= floor && r[c] != '-'; }
            m = __ballot(b);
        }
        return (m >> (p - wbase)) & 1ull;
    };
    auto skip_gaps = [&](uint32_t pos) -> uint32_t {
        while (pos < n && !base_at(pos)) {
            const unsigned long long rest = m >> (pos - wbase);
            pos = rest ? pos + (uint32_t)__builtin_ctzll(rest) : wbase + 64u;
        }
        return pos < n ? pos : n;
    };
    trimmed = 0; stopped = false; stop_pos = n;
    uint32_t pos = skip_gaps(start < n ? start : n);
    if (pos >= n) { stopped = true; return; }      // a row of gaps: the reference's first block is empty and stops the scan at n
    while (pos < n) {
        uint32_t end = pos;
        int gaps = 0, sz = 0;
        while (gaps < 4 && end < n && sz < 10) {
            if (!base_at(end)) ++gaps; else { ++sz; gaps = 0; }
            ++end;
        }
        if (sz < 10) {
            uint32_t run = end;
            while (run < n && gaps < 20 && !base_at(run)) { ++run; ++gaps; }
            if (gaps >= 20) {
                for (uint32_t t = pos + lane; t < end; t += 64) r[REV ? n - 1u - t : t] = '-';
                trimmed += (uint32_t)sz;
                pos = skip_gaps(run);      // the reference's `end`: behind the whole run
                continue;
            }
        }
        stopped = true; stop_pos = pos;
        break;
    }
}

// Step c of the consensus support: the vote of MODE 2 (rows in order, the reference's slot order with strict '>') that also keeps, per
// column, four uint32, field f at ccnt[f * cnt_stride]: support and depth in reads, then the winner's count and the total in rows of
// this MSA.  Rows that are reads (msup == null) count 1 each: the first pair is the second.
__device__ __forceinline__ void vote_support(const post_args &A, uint32_t p, uint32_t tid, uint32_t q0, uint32_t R, uint32_t W, const uint8_t *rc,
                                             const uint32_t *msup, const uint32_t *mdep) {
    uint8_t *ccons = A.ccons + A.coff[p];
    uint32_t *ccnt = A.ccnt + A.coff[p];
    uint8_t o[6];
    for (int s = 0; s < 6; ++s) o[s] = A.order[s];
    for (uint32_t k = tid; k < W; k += 256) {
        uint32_t occ[6] = {0, 0, 0, 0, 0, 0}, sup[6] = {0, 0, 0, 0, 0, 0}, dep = 0;
        for (uint32_t i = 0; i < R; ++i) {
            if ((int32_t)k < A.rfirst[q0 + i] || (int32_t)k > A.rlast[q0 + i]) continue;
            const uint8_t nt = rc[(uint64_t)i * W + k];
            const uint32_t sv = !msup ? 1u : nt != '-' ? msup[(uint64_t)i * W + k] : 0u;
            dep += msup ? mdep[(uint64_t)i * W + k] : 1u;
#pragma unroll
            for (int s = 0; s < 6; ++s) if (nt == o[s]) { ++occ[s]; sup[s] += sv; }
        }
        uint32_t best = 0, bsup = 0, total = 0;
        uint8_t nt = 0;
#pragma unroll
        for (int s = 0; s < 6; ++s) { total += occ[s]; if (occ[s] > best) { best = occ[s]; nt = o[s]; bsup = sup[s]; } }
        ccons[k] = nt ? nt : (uint8_t)'-';
        ccnt[k] = bsup; ccnt[A.cnt_stride + k] = dep; ccnt[2 * A.cnt_stride + k] = best; ccnt[3 * A.cnt_stride + k] = total;
    }
}

// LDS accesses of one wavefront are served in program order; this keeps the compiler from moving them across a point where the lanes
// read what other lanes of the wavefront wrote
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// -DPOST_MSA_TICKS: thread 0 of every workgroup adds the 100 MHz ticks it spent in each step (a, b, c, d) to g_post_ticks, and
// launch_post_msa prints the sums of the launch (profiles/post_msa_wide.txt).  Not part of any shipped build.
#ifdef POST_MSA_TICKS
__device__ unsigned long long g_post_ticks[4];
#define POST_TICK_BEGIN unsigned long long t_prev = wall_clock64();
#define POST_TICK(n) do { if (tid == 0) { const unsigned long long t_now = wall_clock64(); atomicAdd(&g_post_ticks[n], t_now - t_prev); t_prev = t_now; } } while (0)
#else
#define POST_TICK_BEGIN
#define POST_TICK(n) do {} while (0)
#endif

// Step a for one row by one wavefront: the bases [b0, b1) of the row go to the cell of their MSA column in dc (their quality bytes in
// dq; with dsup, the support and depth of a composed pack's bases in dsup / ddep).  256 bases a round: the loads of a round are
// issued together.
template <int MODE>
__device__ __forceinline__ void scatter_row(const post_args &A, uint64_t b0, uint64_t b1, uint32_t lane, uint32_t W, uint8_t *dc, uint8_t *dq,
                                            uint32_t *dsup, uint32_t *ddep) {
    for (uint64_t b = b0 + lane; b < b1; b += 256) {
        uint32_t c[4];
        uint8_t sv[4], qv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t bu = b + 64u * u < b1 ? b + 64u * u : b;      // (a lane behind the row's end loads base b again and drops it)
            c[u] = A.col[bu]; sv[u] = A.seq[bu]; qv[u] = MODE == 1 ? A.qual[bu] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b + 64u * u >= b1 || c[u] >= W) continue;
            dc[c[u]] = sv[u];
            if (MODE == 1) dq[c[u]] = qv[u];
            if (dsup) { dsup[c[u]] = A.in_sup[b + 64u * u]; ddep[c[u]] = A.in_dep[b + 64u * u]; }
        }
    }
}

template <int MODE, bool REPORT = false>
__global__ __launch_bounds__(256) void post_msa_kernel(post_args A) {
    constexpr bool SUPPORT = MODE == 2 && REPORT;      // <1, true>: the correction report; <2, true>: the consensus support
    __shared__ double s_perr[256];
    __shared__ int32_t s_first[POST_WIN_ROWS], s_last[POST_WIN_ROWS];
    __shared__ uint4 s_rowc[POST_WAVES][POST_STAGE_W / 16 + 2];
    __shared__ uint4 s_rowq[MODE == 1 ? POST_WAVES : 1][MODE == 1 ? POST_STAGE_W / 16 + 2 : 1];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = wave_uniform(tid >> 6);
    const uint32_t q0 = A.pack_first[p], q1 = A.pack_first[p + 1], R = q1 - q0;
    const uint32_t W = A.width[p];
    uint8_t *rc = A.rowc + A.moff[p];
    uint8_t *rq = MODE == 1 ? A.rowq + A.moff[p] : nullptr;
    const uint64_t cells = (uint64_t)R * W;
    if (MODE == 1) s_perr[tid] = A.perr[tid];
    if (R == 0 || W == 0) {
        if (tid == 0 && MODE == 2) A.cons_len[p] = 0;
        if (MODE == 1) for (uint32_t i = tid; i < R; i += 256) { A.olen[q0 + i] = 0; A.tfront[q0 + i] = 0; A.tback[q0 + i] = 0; }
        if (REPORT && MODE == 1) for (uint32_t i = tid; i < R; i += 256) for (uint32_t f = 0; f < REP_KERNEL; ++f) A.rep[(uint64_t)f * A.rep_stride + q0 + i] = 0;
        return;
    }
    POST_TICK_BEGIN
    // ---- a. expand: a wavefront per row
    const uint4 gap16 = make_uint4(0x2d2d2d2du, 0x2d2d2d2du, 0x2d2d2d2du, 0x2d2d2d2du), zero16 = make_uint4(0u, 0u, 0u, 0u);
    const bool composed = SUPPORT && p < A.n_composed;
    if (W <= POST_STAGE_W) {
        // the row is built in LDS at the offset its first cell has in a 16-byte line of memory (s: the matrix starts on such a line,
        // the row i * W cells behind it) and leaves in whole lines; the first and the last line of a row, which it shares with its
        // neighbours, leave byte by byte
        uint4 *l16c = s_rowc[wave], *l16q = s_rowq[MODE == 1 ? wave : 0];
        uint8_t *lc = reinterpret_cast<uint8_t *>(l16c), *lq = reinterpret_cast<uint8_t *>(l16q);
        for (uint32_t i = wave; i < R; i += POST_WAVES) {
            const uint64_t at = (uint64_t)i * W;
            const uint32_t s = (uint32_t)(at & 15u), nline = (s + W + 15u) >> 4;
            for (uint32_t j = lane; j < nline; j += 64) { l16c[j] = gap16; if (MODE == 1) l16q[j] = zero16; }
            wave_sync();
            const uint64_t b0 = A.off[q0 + i], b1 = A.off[q0 + i + 1];
            scatter_row<MODE>(A, b0, b1, lane, W, lc + s, MODE == 1 ? lq + s : nullptr, composed ? A.msup + A.moff[p] + at : nullptr, composed ? A.mdep + A.moff[p] + at : nullptr);
            wave_sync();
            uint8_t *gc = rc + at - s, *gq = MODE == 1 ? rq + at - s : nullptr;
            for (uint32_t j = lane; j < nline; j += 64) {
                const uint32_t x0 = 16u * j;
                if (x0 >= s && x0 + 16u <= s + W) {
                    *reinterpret_cast<uint4 *>(gc + x0) = l16c[j];
                    if (MODE == 1) *reinterpret_cast<uint4 *>(gq + x0) = l16q[j];
                } else {
                    for (uint32_t x = x0 < s ? s : x0; x < x0 + 16u && x < s + W; ++x) { gc[x] = lc[x]; if (MODE == 1) gq[x] = lq[x]; }
                }
            }
            wave_sync();
        }
    } else {
        // a row that fits no staging: the matrix is filled in 16-byte lines (its room ends on one), then the bases are scattered
        uint4 *c16 = reinterpret_cast<uint4 *>(rc), *q16 = reinterpret_cast<uint4 *>(rq);
        const uint64_t nline = (cells + 15u) >> 4;
        for (uint64_t t = tid; t < nline; t += 256) { c16[t] = gap16; if (MODE == 1) q16[t] = zero16; }
        __syncthreads();
        for (uint32_t i = wave; i < R; i += POST_WAVES) {
            const uint64_t at = (uint64_t)i * W;
            const uint64_t b0 = A.off[q0 + i], b1 = A.off[q0 + i + 1];
            scatter_row<MODE>(A, b0, b1, lane, W, rc + at, MODE == 1 ? rq + at : nullptr, composed ? A.msup + A.moff[p] + at : nullptr, composed ? A.mdep + A.moff[p] + at : nullptr);
        }
    }
    __syncthreads();
    POST_TICK(0);
    // ---- b. fix ends (correct.cpp:32-92): phase 1 from the left, phase 2 from the right, a wavefront per row.  Each side starts at
    // the column of the row's first / last base: what lies in front of it is gaps
    for (uint32_t i = wave; i < R; i += POST_WAVES) {
        uint8_t *row = rc + (uint64_t)i * W;
        const uint64_t b0 = A.off[q0 + i], b1 = A.off[q0 + i + 1];
        uint32_t c_first = W, c_last = 0;
        if (b1 > b0) { c_first = wave_uniform(A.col[b0]); c_last = wave_uniform(A.col[b1 - 1]); }
        uint32_t t1 = 0, t2 = 0, p1 = W, p2 = W;
        bool s1 = false, s2 = false;
        fix_wave<false>(row, W, lane, c_first, 0u, t1, p1, s1);
        if (s1) fix_wave<true>(row, W, lane, b1 > b0 && c_last < W ? W - 1u - c_last : 0u, p1, t2, p2, s2);
        int32_t first = (int32_t)W, last = -1;
        if (s1 && s2 && p1 < W && p2 < W) { first = (int32_t)p1; last = (int32_t)(W - 1u - p2); }
        if (lane == 0) {
            A.rfirst[q0 + i] = first; A.rlast[q0 + i] = last;
            if (i < POST_WIN_ROWS) { s_first[i] = first; s_last[i] = last; }
            if (MODE == 1) { A.tfront[q0 + i] = t1; A.tback[q0 + i] = t2; }
        }
        if constexpr (SUPPORT) if (composed) {
            // a gap inside the window stands for the depth of the row's last base before it (a window starts on a base): 64 cells at
            // a time, every gap takes the depth of the nearest base below it in the block, or what the blocks before carried over
            uint32_t *drow = A.mdep + A.moff[p] + (uint64_t)i * W;
            uint32_t carry = 0;
            for (int32_t kb = first; kb <= last; kb += 64) {
                const int32_t k = kb + (int32_t)lane;
                const bool in = k <= last, base = in && row[k] != '-';
                const uint32_t v = base ? drow[k] : 0u;
                const unsigned long long mb = __ballot(base), below = mb & (~0ull >> (63u - lane));
                const uint32_t from_block = (uint32_t)__shfl((int)v, below ? 63 - __builtin_clzll(below) : 0);
                if (in && !base) drow[k] = below ? from_block : carry;
                const uint32_t top = (uint32_t)__shfl((int)v, mb ? 63 - __builtin_clzll(mb) : 0);
                if (mb) carry = top;
            }
        }
    }
    __syncthreads();
    POST_TICK(1);
    // ---- c. vote (correct.cpp:94-193): POST_VOTE_COLS adjacent columns per thread, rows in order.  A row's cells of these columns
    // are one 4-byte load wherever the row starts (the columns behind the row's end are the next row's cells, or the 64 spare bytes
    // behind the last matrix: no window covers them)
    uint8_t *ccons = A.ccons + A.coff[p];
    uint8_t *cflag = A.cflag + A.coff[p];
    uint8_t *csym = A.csym + A.coff[p];
    double *cerr = A.cerr + A.coff[p];
    const uint8_t o0 = A.order[0], o1 = A.order[1], o2 = A.order[2], o3 = A.order[3], o4 = A.order[4], o5 = A.order[5];
    if constexpr (SUPPORT) vote_support(A, p, tid, q0, R, W, rc, p < A.n_composed ? A.msup + A.moff[p] : nullptr, p < A.n_composed ? A.mdep + A.moff[p] : nullptr);
    else for (uint32_t k0 = tid * POST_VOTE_COLS; k0 < W; k0 += 256 * POST_VOTE_COLS) {
        static_assert(POST_VOTE_COLS == 4, "one dword of cells per row");
        // the sums of column k0 + c, a variable per vote slot (arrays indexed by the slot that matched would leave the registers)
#define VOTE_SUMS(c) int occ0_##c = 0, occ1_##c = 0, occ2_##c = 0, occ3_##c = 0, occ4_##c = 0, occ5_##c = 0; \
                     double e0_##c = 0.0, e1_##c = 0.0, e2_##c = 0.0, e3_##c = 0.0, e4_##c = 0.0, e5_##c = 0.0;
        VOTE_SUMS(0) VOTE_SUMS(1) VOTE_SUMS(2) VOTE_SUMS(3)
#undef VOTE_SUMS
        const uint8_t *pc = rc + k0, *pq = MODE == 1 ? rq + k0 : nullptr;
#define VOTE_CELL(c)                                                                                                                        \
            if ((int32_t)k0 + c >= first && (int32_t)k0 + c <= last) {                                                                      \
                const uint8_t nt = (uint8_t)(vc >> (8 * c));                                                                                \
                if (MODE == 1) {                                                                                                            \
                    const double ep = nt != '-' ? s_perr[(vq >> (8 * c)) & 0xFFu] : 0.0;                                                    \
                    /* one slot matches; the other sums are unchanged (x + 0.0 == x for x >= +0.0) */                                       \
                    if (nt == o0) { ++occ0_##c; e0_##c += ep; } else if (nt == o1) { ++occ1_##c; e1_##c += ep; }                            \
                    else if (nt == o2) { ++occ2_##c; e2_##c += ep; } else if (nt == o3) { ++occ3_##c; e3_##c += ep; }                       \
                    else if (nt == o4) { ++occ4_##c; e4_##c += ep; } else if (nt == o5) { ++occ5_##c; e5_##c += ep; }                       \
                } else {                                                                                                                    \
                    occ0_##c += nt == o0; occ1_##c += nt == o1; occ2_##c += nt == o2; occ3_##c += nt == o3; occ4_##c += nt == o4; occ5_##c += nt == o5; \
                }                                                                                                                           \
            }
#define VOTE_ROW(i, first_of_row, last_of_row)                                  \
        {                                                                       \
            const int32_t first = first_of_row, last = last_of_row;             \
            uint32_t vc, vq = 0;                                                \
            __builtin_memcpy(&vc, pc + (uint64_t)(i) * W, 4);                   \
            if (MODE == 1) __builtin_memcpy(&vq, pq + (uint64_t)(i) * W, 4);    \
            VOTE_CELL(0) VOTE_CELL(1) VOTE_CELL(2) VOTE_CELL(3)                 \
        }
        // the windows of the first POST_WIN_ROWS rows are in LDS (every lane asks for the same row), those of the rows behind in memory
        const uint32_t R_lds = R < POST_WIN_ROWS ? R : POST_WIN_ROWS;
#pragma unroll 4
        for (uint32_t i = 0; i < R_lds; ++i) VOTE_ROW(i, s_first[i], s_last[i])
#pragma unroll 1
        for (uint32_t i = R_lds; i < R; ++i) VOTE_ROW(i, A.rfirst[q0 + i], A.rlast[q0 + i])
#undef VOTE_ROW
#undef VOTE_CELL
        // reference iteration order, strict '>' (correct.cpp:174-186); means as err / double(occ)
#define SLOT(occ, err, oc)                                                          \
            { double m = err; if (occ > 0 && MODE == 1) m = err / double(occ);      \
              if (occ > best) { best = occ; nt = oc; bocc = occ; berr = m; } }
#define VOTE_COLUMN(c)                                                                                                                      \
        if (k0 + c < W) {                                                                                                                   \
            const uint32_t k = k0 + c;                                                                                                      \
            const int total = occ0_##c + occ1_##c + occ2_##c + occ3_##c + occ4_##c + occ5_##c;                                              \
            int best = 0, bocc = 0;                                                                                                         \
            uint8_t nt = 0;                                                                                                                 \
            double berr = 0.0;                                                                                                              \
            SLOT(occ0_##c, e0_##c, o0) SLOT(occ1_##c, e1_##c, o1) SLOT(occ2_##c, e2_##c, o2)                                                \
            SLOT(occ3_##c, e3_##c, o3) SLOT(occ4_##c, e4_##c, o4) SLOT(occ5_##c, e5_##c, o5)                                                \
            if (nt == 0) { ccons[k] = '-'; if (MODE == 1) { cflag[k] = 0; csym[k] = 0; cerr[k] = 0.0; } }                                   \
            else {                                                                                                                          \
                ccons[k] = nt;                                                                                                              \
                if (MODE == 1) {                                                                                                            \
                    const double ratio = double(bocc) / double(total);                                                                      \
                    cflag[k] = (uint8_t)((ratio >= A.gap_occ ? 1 : 0) | (ratio >= A.min_occ ? 2 : 0));                                      \
                    cerr[k] = berr;                                                                                                         \
                    csym[k] = (uint8_t)(phred_value(A, berr) & 0xFF);                                                                       \
                }                                                                                                                           \
            }                                                                                                                               \
        }
        VOTE_COLUMN(0) VOTE_COLUMN(1) VOTE_COLUMN(2) VOTE_COLUMN(3)
#undef VOTE_COLUMN
#undef SLOT
    }
    __syncthreads();
    POST_TICK(2);
    if (MODE == 1) {
        // ---- d. per-read correction (correct.cpp:196-309), in place, a wavefront per row, POST_FIX_BLOCKS blocks of 64 columns at
        // a time.  Every lane decides its column; the emitted bytes go to the output cursor plus the number of emitting lanes below.
        // In place is safe because (1) all loads of a round stand before its first store, and (2) a column emits at most one byte, so
        // the cursor never passes the first column of the round: the stores touch only cells this or an earlier round has read.
        for (uint32_t i = wave; i < R; i += POST_WAVES) {
            uint8_t *row = rc + (uint64_t)i * W;
            uint8_t *qrow = rq + (uint64_t)i * W;
            const int32_t first = (int32_t)wave_uniform((uint32_t)A.rfirst[q0 + i]), last = (int32_t)wave_uniform((uint32_t)A.rlast[q0 + i]);
            uint32_t o = 0;
            uint32_t n_match = 0, n_subst = 0, n_miskept = 0, n_ins = 0, n_del = 0, n_gapkept = 0;      // REPORT: the branch taken, per lane
            for (int32_t kb = first; kb <= last; kb += 64 * POST_FIX_BLOCKS) {
                uint8_t nt[POST_FIX_BLOCKS], qq[POST_FIX_BLOCKS], cnt[POST_FIX_BLOCKS], fl[POST_FIX_BLOCKS], sy[POST_FIX_BLOCKS];
                double ce[POST_FIX_BLOCKS];
#pragma unroll
                for (int u = 0; u < POST_FIX_BLOCKS; ++u) {
                    const int32_t k = kb + 64 * u + (int32_t)lane, kk = k <= last ? k : last;      // (a lane behind the window loads the window's last column and drops it)
                    nt[u] = row[kk]; qq[u] = qrow[kk]; cnt[u] = ccons[kk]; fl[u] = cflag[kk]; sy[u] = csym[kk]; ce[u] = cerr[kk];
                }
#pragma unroll
                for (int u = 0; u < POST_FIX_BLOCKS; ++u) {
                    const int32_t k = kb + 64 * u + (int32_t)lane;
                    uint8_t es = 0, eq = 0;
                    bool emit = k <= last;
                    if (!emit) {
                    } else if (cnt[u] == '-') {
                        if (nt[u] != '-' && !(fl[u] & 1)) { es = nt[u]; eq = qq[u]; if (REPORT) ++n_gapkept; }
                        else { emit = false; if (REPORT && nt[u] != '-') ++n_del; }
                    } else if (nt[u] == '-') {
                        if (fl[u] & 1) { es = cnt[u]; eq = sy[u]; if (REPORT) ++n_ins; } else emit = false;
                    } else if (nt[u] == cnt[u]) {
                        es = nt[u]; eq = qq[u];
                        if (REPORT) ++n_match;
                    } else if ((fl[u] & 2) && A.err_ratio * s_perr[qq[u]] > ce[u]) {
                        es = cnt[u]; eq = sy[u];
                        if (REPORT) ++n_subst;
                    } else {
                        es = nt[u]; eq = qq[u];
                        if (REPORT) ++n_miskept;
                    }
                    const unsigned long long m = __ballot(emit);
                    if (emit) { const uint32_t at = o + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); row[at] = es; qrow[at] = eq; }
                    o += (uint32_t)__popcll(m);
                }
            }
            if (lane == 0) A.olen[q0 + i] = o;
            if (REPORT) {
                n_match = wave_sum(n_match); n_subst = wave_sum(n_subst); n_miskept = wave_sum(n_miskept);
                n_ins = wave_sum(n_ins); n_del = wave_sum(n_del); n_gapkept = wave_sum(n_gapkept);
                if (lane == 0) {
                    uint32_t *rep = A.rep + q0 + i;
                    const uint64_t s = A.rep_stride;
                    rep[(REP_MATCH - REP_MATCH) * s] = n_match; rep[(REP_SUBST - REP_MATCH) * s] = n_subst; rep[(REP_MISKEPT - REP_MATCH) * s] = n_miskept;
                    rep[(REP_INS - REP_MATCH) * s] = n_ins; rep[(REP_DEL - REP_MATCH) * s] = n_del; rep[(REP_GAPKEPT - REP_MATCH) * s] = n_gapkept;
                }
            }
        }
    } else {
        // ---- d'. consensus = column winners without gaps
        if (tid < 64) {
            uint8_t *out = A.cons_out + A.coff[p];
            uint32_t o = 0;
            for (uint32_t base = 0; base < W; base += 64) {
                const uint32_t k = base + tid;
                const uint8_t c = k < W ? ccons[k] : (uint8_t)'-';
                const bool keep = c != '-';
                const unsigned long long m = __ballot(keep);
                if (keep) out[o + __popcll(m & ((1ull << tid) - 1ull))] = c;
                if constexpr (SUPPORT) if (keep) {
                    const uint32_t *cc = A.ccnt + A.coff[p] + k;
                    uint32_t *oc = A.ocnt + A.coff[p] + o + __popcll(m & ((1ull << tid) - 1ull));
                    for (uint32_t f = 0; f < 4; ++f) oc[f * A.cnt_stride] = cc[f * A.cnt_stride];
                }
                o += (uint32_t)__popcll(m);
            }
            if (tid == 0) A.cons_len[p] = o;
        }
    }
    POST_TICK(3);
}

int launch_post_msa(rattle_ctx *ctx, const post_args &A, uint32_t n_packs, int mode) {
    if (n_packs == 0) return 0;
    // step a writes the rows in 16-byte lines: moff counts from a 16-byte boundary
    if (((uintptr_t)A.rowc | (uintptr_t)A.rowq) & 15u) { set_error("post-MSA kernel: the row matrices are not 16-byte aligned"); return RATTLE_ERR_HIP; }
#ifdef POST_MSA_TICKS
    unsigned long long ticks[4] = {0, 0, 0, 0};
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_post_ticks), ticks, sizeof(ticks)));
    struct report {
        rattle_ctx *ctx; int mode; uint32_t n_packs;
        ~report() {
            unsigned long long t[4] = {0, 0, 0, 0};
            if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpyFromSymbol(t, HIP_SYMBOL(g_post_ticks), sizeof(t)) != hipSuccess) return;
            fprintf(stderr, "post_msa ticks (10 ns, summed over workgroups): mode %d packs %u a %llu b %llu c %llu d %llu\n", mode, n_packs, t[0], t[1], t[2], t[3]);
        }
    } rep{ctx, mode, n_packs};
#endif
    ktimer T(ctx, K_POST, 0);
    if (mode == 1 && A.rep) hipLaunchKernelGGL((post_msa_kernel<1, true>), dim3(n_packs), dim3(256), 0, ctx->stream, A);      // the report form: same timer slot
    else if (mode == 1) hipLaunchKernelGGL(post_msa_kernel<1>, dim3(n_packs), dim3(256), 0, ctx->stream, A);
    else if (A.ccnt) hipLaunchKernelGGL((post_msa_kernel<2, true>), dim3(n_packs), dim3(256), 0, ctx->stream, A);      // the consensus support
    else hipLaunchKernelGGL(post_msa_kernel<2>, dim3(n_packs), dim3(256), 0, ctx->stream, A);
    RT_HIP(hipGetLastError());
    return 0;
}

// ---- phred_symbol table (host) ----------------------------------------------------------------------
namespace {
inline int phred_host(double p) { return (int)(-10 * log10(p) + 33); }      // utils.cpp:6-8 before the (char) narrowing
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
}  // namespace

void build_phred_table(phred_table &T) {
    // symbol values n0 .. n0+cnt-1 cover p in [1e-36, 1e33]; quality bytes give p in [1e-10, 1e17]
    T.n0 = -300;
    const int cnt = 700;
    T.lo.assign(cnt, 0.0);
    T.exc_bits.clear(); T.exc_val.clear();
    const uint64_t bmin = 1, bmax = 0x7FEFFFFFFFFFFFFFull;
    for (int t = 0; t < cnt; ++t) {
        const int n = T.n0 + t;
        // smallest positive double with phred_host(p) <= n (phred_host is non-increasing in p up to libm wiggles)
        uint64_t a = bmin, b = bmax;
        while (a < b) { const uint64_t m = a + (b - a) / 2; if (phred_host(from_bits(m)) <= n) b = m; else a = m + 1; }
        T.lo[t] = from_bits(a);
    }
    // exhaustive check around every threshold; anything the table would get wrong becomes an exception
    auto table_value = [&](double p) {
        int lo = 0, hi = cnt - 1;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (p >= T.lo[m]) hi = m; else lo = m + 1; }
        return T.n0 + lo;
    };
    std::vector<std::pair<uint64_t, int>> exc;
    for (int t = 0; t < cnt; ++t) {
        uint64_t c; memcpy(&c, &T.lo[t], 8);
        if (c < 4096 || c > bmax - 4096) continue;
        for (uint64_t b = c - 2048; b <= c + 2048; ++b) {
            const double p = from_bits(b);
            const int want = phred_host(p);
            if (table_value(p) != want) exc.emplace_back(b, want);
        }
    }
    std::sort(exc.begin(), exc.end());
    exc.erase(std::unique(exc.begin(), exc.end()), exc.end());
    for (auto &e : exc) { T.exc_bits.push_back(e.first); T.exc_val.push_back(e.second); }
}

// Host mirror of the device lookup (phred_value), for the CPU-side test of the table construction.
int phred_lookup_host(const phred_table &T, double p) {
    uint64_t bits;
    memcpy(&bits, &p, 8);
    const auto it = std::lower_bound(T.exc_bits.begin(), T.exc_bits.end(), bits);
    if (it != T.exc_bits.end() && *it == bits) return T.exc_val[it - T.exc_bits.begin()];
    int lo = 0, hi = (int)T.lo.size() - 1;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (p >= T.lo[m]) hi = m; else lo = m + 1; }
    return T.n0 + lo;
}

}  // namespace rattle
