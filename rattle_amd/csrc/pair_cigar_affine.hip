// Kernel F with three states: the CIGAR of every pair the three-state kernel E aligned (include/rattle_hip.h, "align_cigars_scored";
// DESIGN.md, "Kernels E and F with three states"; tests/align_affine_ref.py is the contract).
//
// The record gives a pair its rectangle on the aligned strand.  Gotoh's recurrence over the rectangle alone (H' = 0, U' = L' = -inf on its
// top row and left column) reproduces the full matrices on every (cell, state) of the chosen path and is nowhere larger (DESIGN.md states
// the lemma, tests/test_align_affine_ref.py checks it), so a walk back from H' of the rectangle's last cell is the walk of the full
// matrices and ends at the rectangle's first cell.
//
// Forward pass: kernel F's (pair_cigar.hip), with the two scores that cross a row -- H and U come from lane l - 1 by the DPP wave_shr:1,
// L stays in the lane; lane 0's H and U from the pair's hand-over strip, 8 bytes per column, read 64 columns at a time one refill ahead
// and updated in place behind the reads.  Each cell's decision is four bits: H's 2-bit code (0 zero cell: the path stops, 1 diagonal,
// 2 U, 3 L), "U extends" and "L extends" (open wins a tie, so a bit is set only where extend is strictly larger).  Four ballots per step
// make the 32-byte record of (block, step): two uint4, the code's low and high bit, then the U and the L bit.  Lane k keeps the record of
// step S + k of the current 64 steps and the 64 records go out as one coalesced store, lane 63's two scores for the strip likewise.
//
// Walk: the same wavefront, after a device-scope fence, with a wave-uniform state H | U | L beside (block, lane, column).  In H it reads
// the 2-bit code and either emits = / X and moves diagonally, or switches to U or L WITHOUT moving.  In U it emits I and moves up, and the
// U bit OF THE CELL IT LEFT says whether it stays in U (that cell's U came from the U above) or lands in H; L is the same with D, moving
// left.  Windows, letters and the ops region are kernel F's.
//
// Bounds: an emitting move lowers the row or the column and the walk ends at row 0 or column 0, so at most rows + cols moves emit; a
// switch of state is followed by an emitting move, and the loop is cut at 2 (rows + cols) iterations whatever the codes say.  The window
// index is step - window start in [0, 64) by construction; the ops cursor is checked before every store.  Every load and store lies in
// the pair's own sequences, strip, records, ops region or count.  A wrong code gives a wrong string, never a hang or a store out of range.
#include "cigar_plan.h"
#include "common.h"

namespace rattle {

namespace {

constexpr int32_t CA_NEG = -(1 << 30);                                        // minus infinity: CA_NEG - 64 does not wrap
constexpr uint32_t CA_OP_I = 1, CA_OP_D = 2, CA_OP_EQ = 7, CA_OP_X = 8;      // BAM's numbers
constexpr uint32_t CA_MAX_RUN = 0x0FFFFFFFu;                                  // 28 bits of length: a longer run is written in pieces
constexpr uint32_t CA_H = 0, CA_U = 1, CA_L = 2;                              // the walk's state

__device__ __forceinline__ int32_t ca_shr1(int32_t v, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
}

// A 0, C 1, G 2, T and U 3 (the complement of code c is 3 - c); the host has refused every other byte
__device__ __forceinline__ int32_t ca_code(uint32_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3; }

__device__ __forceinline__ uint32_t ca_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v); }

__global__ __launch_bounds__(256) void pair_cigar_affine_kernel(const cigar_pair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qseq,
                                                                const uint8_t *__restrict__ tseq, uint4 *__restrict__ codes, int2 *__restrict__ strips,
                                                                uint32_t *__restrict__ ops, uint32_t *__restrict__ counts, int32_t sm, int32_t sx,
                                                                int32_t so, int32_t se) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const cigar_pair P = pairs[p];
    const uint32_t sq = ca_uniform(P.rows), st = ca_uniform(P.cols), rev = ca_uniform(P.rev);
    // row r of the rectangle is read base q[r] (forward) or the complement of q[-r] (reverse: q points at the last base of the span)
    const uint8_t *q = qseq + P.q, *t = tseq + P.t;
    uint4 *code = codes + 2 * P.codes;                               // two uint4 per record
    int2 *strip = strips + P.strip / 2;                              // (the plan counts words: two per column)
    uint32_t *op = ops + P.ops;
    const uint64_t stride = (uint64_t)st + CG_ROWS - 1;               // records of one block

    // ---- forward: the codes of every cell of the rectangle ----
    for (uint32_t r0 = 0, b = 0; r0 < sq; r0 += CG_ROWS, ++b) {
        const uint32_t r = r0 + lane;                                // the lane's row
        const bool row = r < sq;
        int32_t ql = 4;                                              // (matches nothing)
        if (row) ql = rev ? 3 - ca_code(*(q - r)) : ca_code(q[r]);
        const bool from_strip = r0 > 0, to_strip = r0 + CG_ROWS < sq;
        const uint32_t n_steps = st + min(CG_ROWS, sq - r0) - 1;     // the block's last row computes its last column at the last step
        uint4 *rec_b = code + 2 * ((uint64_t)b * stride);
        int32_t cH = 0, cU = CA_NEG, cL = CA_NEG, dH = 0, tl = 4;    // the lane's previous cell in its three states, lane - 1's H as received one step ago
        // refill in flight: the transcript's letters and the strip's scores (H, U) of columns [S + 64, S + 128)
        int32_t nT = 4;
        int2 nS = make_int2(0, CA_NEG);
        if (lane < st) { nT = ca_code(t[lane]); if (from_strip) nS = strip[lane]; }
        for (uint32_t S = 0; S < n_steps; S += 64) {
            const int32_t bT = nT;
            const int2 bS = nS;
            nT = 4; nS = make_int2(0, CA_NEG);
            if (S + 64 + lane < st) { nT = ca_code(t[S + 64 + lane]); if (from_strip) nS = strip[S + 64 + lane]; }
            const uint32_t k_end = min(64u, n_steps - S);
            uint4 rec0 = make_uint4(0, 0, 0, 0), rec1 = make_uint4(0, 0, 0, 0);      // lane k: the record of step S + k
            int2 last = make_int2(0, CA_NEG);                        // lane k: lane 63's H and U after step S + k, column S + k - 63
            for (uint32_t k = 0; k < k_end; ++k) {
                const uint32_t s = S + k;
                // lane 0's up cell and letter: column s of the buffers (H 0 and U minus infinity on the first block and beyond the transcript's end)
                const int32_t fT = __builtin_amdgcn_readlane(bT, k);
                const int32_t uH = ca_shr1(cH, __builtin_amdgcn_readlane(bS.x, k)), uU = ca_shr1(cU, __builtin_amdgcn_readlane(bS.y, k));
                tl = ca_shr1(tl, fT);
                const uint32_t c = s - lane;                         // the lane's column (wraps below 0: fails the test)
                const bool on = row && c < st;
                const int32_t uo = uH - so, ue = uU - se, lo_ = cH - so, le = cL - se;
                const int32_t u = max(uo, ue), l = max(lo_, le);
                const int32_t d = dH + (ql == tl ? sm : -sx);
                const int32_t h = max(max(d, 0), max(u, l));
                const uint32_t cd = !on || h == 0 ? 0u : d >= u && d >= l ? 1u : u >= l ? 2u : 3u;      // diagonal, then U, then L
                dH = uH;
                if (on) { cH = h; cU = u; cL = l; }
                const uint64_t b0 = __ballot(cd & 1u), b1 = __ballot(cd & 2u), b2 = __ballot(on && ue > uo), b3 = __ballot(on && le > lo_);
                const bool mine = lane == k;
                rec0.x = mine ? (uint32_t)b0 : rec0.x; rec0.y = mine ? (uint32_t)(b0 >> 32) : rec0.y;
                rec0.z = mine ? (uint32_t)b1 : rec0.z; rec0.w = mine ? (uint32_t)(b1 >> 32) : rec0.w;
                rec1.x = mine ? (uint32_t)b2 : rec1.x; rec1.y = mine ? (uint32_t)(b2 >> 32) : rec1.y;
                rec1.z = mine ? (uint32_t)b3 : rec1.z; rec1.w = mine ? (uint32_t)(b3 >> 32) : rec1.w;
                if (to_strip) {
                    const int32_t h63 = __builtin_amdgcn_readlane(cH, 63), u63 = __builtin_amdgcn_readlane(cU, 63);
                    last.x = mine ? h63 : last.x; last.y = mine ? u63 : last.y;
                }
            }
            if (lane < k_end) {
                rec_b[2 * (uint64_t)(S + lane)] = rec0;              // S + lane < n_steps <= stride
                rec_b[2 * (uint64_t)(S + lane) + 1] = rec1;
                const uint32_t cc = S + lane - 63;                   // lane 63's column at that step (wraps below 0: fails the test)
                if (to_strip && S + lane >= 63 && cc < st) strip[cc] = last;      // behind every read of the strip: columns <= S were loaded a refill ago
            }
        }
        __threadfence();                                             // the strip's stores of this block before the next block's loads; the records before the walk
    }

    // ---- walk: from H of the rectangle's last cell back to its first ----
    uint32_t b = (sq - 1) >> 6, L = (sq - 1) & 63u, c = st - 1;      // block, lane (row 64 b + L), column
    const uint32_t region = sq + st;                                 // words of the ops region = the most moves that emit
    uint32_t pos = region, run_op = 0, run_len = 0, state = CA_H;
    uint32_t wb = ~0u, W = 0, qb = ~0u, T0 = ~0u;                    // the windows: block and first step of the records, block of the read bases, first column
    uint4 win0 = make_uint4(0, 0, 0, 0), win1 = make_uint4(0, 0, 0, 0);
    int32_t qw = 4, tw = 4;
    for (uint64_t it = 0; it < 2ull * region; ++it) {
        const uint32_t s = c + L;
        if (b != wb || s < W || s - W >= 64) {                       // records [W, W + 64) of block b, W + 63 = s unless the block begins before
            wb = b; W = s >= 63 ? s - 63 : 0;
            win0 = make_uint4(0, 0, 0, 0); win1 = make_uint4(0, 0, 0, 0);
            if (W + lane <= s) { win0 = code[2 * ((uint64_t)b * stride + W + lane)]; win1 = code[2 * ((uint64_t)b * stride + W + lane) + 1]; }
        }
        const uint32_t sh = L & 31u;
        const uint32_t w0 = L < 32 ? win0.x : win0.y, w1 = L < 32 ? win0.z : win0.w, w2 = L < 32 ? win1.x : win1.y, w3 = L < 32 ? win1.z : win1.w;
        const uint32_t mine = ((w0 >> sh) & 1u) | (((w1 >> sh) & 1u) << 1) | (((w2 >> sh) & 1u) << 2) | (((w3 >> sh) & 1u) << 3);
        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int32_t)mine, s - W);
        uint32_t o;
        bool up, left;
        if (state == CA_H) {
            const uint32_t hc = cd & 3u;
            if (hc == 0) break;                                      // a zero cell: the path begins behind it
            if (hc != 1) { state = hc == 2 ? CA_U : CA_L; continue; }      // into a gap state of the same cell: no move
            if (b != qb) {
                qb = b; qw = 4;
                const uint32_t r = b * CG_ROWS + lane;
                if (r < sq) qw = rev ? 3 - ca_code(*(q - r)) : ca_code(q[r]);
            }
            if (c < T0 || c - T0 >= 64) {
                T0 = c >= 63 ? c - 63 : 0; tw = 4;
                if (T0 + lane <= c) tw = ca_code(t[T0 + lane]);
            }
            o = __builtin_amdgcn_readlane(qw, L) == __builtin_amdgcn_readlane(tw, c - T0) ? CA_OP_EQ : CA_OP_X;
            up = left = true;
        } else if (state == CA_U) {
            o = CA_OP_I; up = true; left = false;
            if (!(cd & 4u)) state = CA_H;                            // this cell's U was opened from the H above
        } else {
            o = CA_OP_D; up = false; left = true;
            if (!(cd & 8u)) state = CA_H;
        }
        if (o == run_op && run_len < CA_MAX_RUN) ++run_len;
        else {
            if (run_len && pos) { --pos; if (lane == 0) op[pos] = run_len << 4 | run_op; }
            run_op = o; run_len = 1;
        }
        bool done = false;
        if (up) { if (L) --L; else if (b) { --b; L = 63; } else done = true; }      // up out of lane 0: lane 63 of the block above
        if (left) { if (c) --c; else done = true; }
        if (done) break;                                             // the rectangle's top row or left column
    }
    if (run_len && pos) { --pos; if (lane == 0) op[pos] = run_len << 4 | run_op; }
    if (lane == 0) counts[p] = region - pos;
}

}  // namespace

void pair_cigar_affine_launch(hipStream_t stream, const cigar_pair *pairs, uint32_t n_pairs, const uint8_t *d_q, const uint8_t *d_t, uint4 *codes,
                              int32_t *strips, uint32_t *ops, uint32_t *counts, const rattle_align_scoring &S) {
    hipLaunchKernelGGL(pair_cigar_affine_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, stream, pairs, n_pairs, d_q, d_t, codes, (int2 *)strips, ops,
                       counts, (int32_t)S.match, (int32_t)S.mismatch, (int32_t)S.gap_open, (int32_t)S.gap_extend);
}

}  // namespace rattle
