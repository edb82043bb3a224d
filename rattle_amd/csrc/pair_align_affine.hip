// Kernel E with three states: the local alignment of every placed read on its transcript with AFFINE gaps and a scoring the caller chooses
// (include/rattle_hip.h, "align_pairs_scored"; DESIGN.md, "Kernels E and F with three states"; tests/align_affine_ref.py is the contract).
//
// Gotoh's recurrence over the letters A, C, G, T = U, with the four magnitudes m, x, o, e as kernel arguments (scalars):
//   U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)      L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)
//   H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])      H[0][*] = H[*][0] = 0,  U[0][*] = L[*][0] = -inf
// A cell with H == 0 begins a new alignment; in H ties go diagonal, then U, then L; in U and in L open wins a tie with extend; the end
// cell is the largest H, ties to the smallest i, then the smallest j.  No traceback: each of the three states of a cell carries
// (start_i, start_j, matches, mismatches) of the path the rule picks for it -- a gap step copies the payload of the state it comes from, a
// diagonal step out of a zero cell starts at the cell's own coordinates -- and the two gap counts follow from the spans.
//
// Shape: kernel E's (pair_align.hip).  One wavefront per pair, four pairs per block, no LDS; lane l owns row 64 b + l, at step s it
// computes column s - l.  L and its payload stay in the lane; H and U with their payloads come from lane l - 1 by the DPP wave_shr:1 --
// eleven moves per step with the sliding letter.  Lane 0's H and U -- the last row of the block before -- come from the pair's hand-over
// strip, 40 bytes per column (five uint2: H, its payload, U, its payload): lane 63 writes a column with five 8-byte stores, and the strip is
// read back 64 columns at a time, one record per lane and one refill ahead of its use; it is updated in place, column c being read one
// refill before step 64 floor(c / 64) and written at step c + 63 of the same block.  On the first block lane 0's U is AF_NEG, the minus
// infinity: -2^30, so that AF_NEG - 64 does not wrap, and no U or L that is computed lies below -64 once an H has entered it.  Lanes whose
// cell is off the matrix keep their state frozen.  A lane keeps its best cell with a strict `>`; the lanes are reduced once, at the end.
// Every load and store lies inside the pair's own two sequences, its own strip and its own record.
#include "align_plan.h"
#include "common.h"

namespace rattle {

namespace {

constexpr int32_t AF_NEG = -(1 << 30);
constexpr uint32_t AF_STRIP_U2 = AL_AFFINE_STRIP_BYTES / 8;      // uint2s per column of the strip

__device__ __forceinline__ int32_t af_shr1(int32_t v, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
}

// A 0, C 1, G 2, T and U 3 (the complement of code c is 3 - c); the host has refused every other byte
__device__ __forceinline__ int32_t af_code(uint32_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3; }

// a state of a cell: its score and the payload of its path
struct af_cell {
    int32_t s, i, j, m, x;
};

__device__ __forceinline__ af_cell af_pick(bool first, const af_cell &a, const af_cell &b) {
    af_cell r;
    r.s = first ? a.s : b.s; r.i = first ? a.i : b.i; r.j = first ? a.j : b.j; r.m = first ? a.m : b.m; r.x = first ? a.x : b.x;
    return r;
}

__global__ __launch_bounds__(256) void pair_align_affine_kernel(const align_pair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qseq,
                                                                const uint8_t *__restrict__ tseq, uint2 *__restrict__ strips, int32_t *__restrict__ recs,
                                                                int32_t sm, int32_t sx, int32_t so, int32_t se) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const align_pair P = pairs[p];
    const uint32_t lq = P.lq, lt = P.lt;
    const uint8_t *q = qseq + P.q, *t = tseq + P.t;
    uint2 *strip = strips + P.strip * AF_STRIP_U2;

    int32_t bH = 0;                                                  // the lane's best cell: score, end (i, j) as DP indices, payload
    uint32_t bi = 0, bj = 0, bsi = 0, bsj = 0, bm = 0, bx = 0;

    for (uint32_t r0 = 0; r0 < lq; r0 += AL_ROWS) {
        const uint32_t r = r0 + lane;                                // the lane's row: read base r (of the strand aligned)
        const bool row = r < lq;
        int32_t ql = 4;                                              // (matches nothing)
        if (row) { const uint32_t c = af_code(q[P.rev ? lq - 1 - r : r]); ql = (int32_t)(P.rev ? 3 - c : c); }
        const bool from_strip = r0 > 0, to_strip = r0 + AL_ROWS < lq;
        const uint32_t n_steps = lt + min(AL_ROWS, lq - r0) - 1;       // the block's last row computes its last column at the last step
        // the lane's previous cell in its three states (H and U go down the lanes, L stays), lane - 1's previous H as received one step ago
        // (diag), the sliding letter
        af_cell cH = {0, 0, 0, 0, 0}, cU = {AF_NEG, 0, 0, 0, 0}, cL = {AF_NEG, 0, 0, 0, 0}, dH = {0, 0, 0, 0, 0};
        int32_t tl = 4;
        // refill in flight: the transcript's letters and the strip's records of columns [S + 64, S + 128); words 0 - 4 H, 5 - 9 U
        int32_t nT = 4;
        uint2 nR[AF_STRIP_U2];
#pragma unroll
        for (uint32_t w = 0; w < AF_STRIP_U2; ++w) nR[w] = make_uint2(0, 0);
        nR[2].y = (uint32_t)AF_NEG;
        if (lane < lt) {
            nT = af_code(t[lane]);
            if (from_strip) {
#pragma unroll
                for (uint32_t w = 0; w < AF_STRIP_U2; ++w) nR[w] = strip[(uint64_t)lane * AF_STRIP_U2 + w];
            }
        }
        for (uint32_t S = 0; S < n_steps; S += 64) {
            const int32_t bT = nT;
            uint2 bR[AF_STRIP_U2];
#pragma unroll
            for (uint32_t w = 0; w < AF_STRIP_U2; ++w) { bR[w] = nR[w]; nR[w] = make_uint2(0, 0); }
            nT = 4; nR[2].y = (uint32_t)AF_NEG;
            if (S + 64 + lane < lt) {
                nT = af_code(t[S + 64 + lane]);
                if (from_strip) {
#pragma unroll
                    for (uint32_t w = 0; w < AF_STRIP_U2; ++w) nR[w] = strip[(uint64_t)(S + 64 + lane) * AF_STRIP_U2 + w];
                }
            }
            const uint32_t k_end = min(64u, n_steps - S);
            for (uint32_t k = 0; k < k_end; ++k) {
                const uint32_t s = S + k;
                // lane 0's up cell and letter: column s of the buffers (H 0 and U minus infinity on the first block and beyond the transcript's end)
                const int32_t fT = __builtin_amdgcn_readlane(bT, k);
                af_cell uH, uU;
                uH.s = af_shr1(cH.s, __builtin_amdgcn_readlane((int32_t)bR[0].x, k));
                uH.i = af_shr1(cH.i, __builtin_amdgcn_readlane((int32_t)bR[0].y, k));
                uH.j = af_shr1(cH.j, __builtin_amdgcn_readlane((int32_t)bR[1].x, k));
                uH.m = af_shr1(cH.m, __builtin_amdgcn_readlane((int32_t)bR[1].y, k));
                uH.x = af_shr1(cH.x, __builtin_amdgcn_readlane((int32_t)bR[2].x, k));
                uU.s = af_shr1(cU.s, __builtin_amdgcn_readlane((int32_t)bR[2].y, k));
                uU.i = af_shr1(cU.i, __builtin_amdgcn_readlane((int32_t)bR[3].x, k));
                uU.j = af_shr1(cU.j, __builtin_amdgcn_readlane((int32_t)bR[3].y, k));
                uU.m = af_shr1(cU.m, __builtin_amdgcn_readlane((int32_t)bR[4].x, k));
                uU.x = af_shr1(cU.x, __builtin_amdgcn_readlane((int32_t)bR[4].y, k));
                tl = af_shr1(tl, fT);
                const uint32_t c = s - lane;                         // the lane's column (wraps below 0: fails the test)
                const bool on = row && c < lt;
                const bool eq = ql == tl;
                // the two gap states: open wins a tie with extend, and the payload is that of the state the step comes from
                af_cell nU = af_pick(uH.s - so >= uU.s - se, uH, uU), nL = af_pick(cH.s - so >= cL.s - se, cH, cL);
                nU.s = max(uH.s - so, uU.s - se); nL.s = max(cH.s - so, cL.s - se);
                const int32_t d = dH.s + (eq ? sm : -sx), u = nU.s, l = nL.s;
                af_cell nH;
                if (d >= u && d >= l) {                              // diagonal first; a zero predecessor begins the alignment at this cell
                    const bool fresh = dH.s == 0;
                    nH.i = fresh ? (int32_t)r : dH.i; nH.j = fresh ? (int32_t)c : dH.j;
                    nH.m = (fresh ? 0 : dH.m) + (eq ? 1 : 0); nH.x = (fresh ? 0 : dH.x) + (eq ? 0 : 1);
                } else nH = af_pick(u >= l, nU, nL);                 // then U, then L
                nH.s = max(max(d, 0), max(u, l));
                dH = uH;
                if (on) {
                    cH = nH; cU = nU; cL = nL;                       // (payload of a zero cell is never read: see `fresh`, and a gap state opened there stays < 0)
                    if (nH.s > bH) { bH = nH.s; bi = r + 1; bj = c + 1; bsi = (uint32_t)nH.i; bsj = (uint32_t)nH.j; bm = (uint32_t)nH.m; bx = (uint32_t)nH.x; }
                    if (to_strip && lane == 63) {                    // c < lt: inside the pair's strip
                        uint2 *o = strip + (uint64_t)c * AF_STRIP_U2;
                        o[0] = make_uint2((uint32_t)nH.s, (uint32_t)nH.i); o[1] = make_uint2((uint32_t)nH.j, (uint32_t)nH.m);
                        o[2] = make_uint2((uint32_t)nH.x, (uint32_t)nU.s); o[3] = make_uint2((uint32_t)nU.i, (uint32_t)nU.j);
                        o[4] = make_uint2((uint32_t)nU.m, (uint32_t)nU.x);
                    }
                }
            }
        }
        __threadfence();                                             // the strip's stores of this block before the next block's loads
    }

    // the best of the 64 lanes: score desc, i asc, j asc (a lane without a positive cell loses to every other)
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t oH = __shfl_xor(bH, off);
        const uint32_t oi = __shfl_xor(bi, off), oj = __shfl_xor(bj, off), osi = __shfl_xor(bsi, off), osj = __shfl_xor(bsj, off);
        const uint32_t om = __shfl_xor(bm, off), ox = __shfl_xor(bx, off);
        if (oH > bH || (oH == bH && (oi < bi || (oi == bi && oj < bj)))) { bH = oH; bi = oi; bj = oj; bsi = osi; bsj = osj; bm = om; bx = ox; }
    }
    if (lane == 0) {
        int32_t *R = recs + (size_t)p * AL_REC_WORDS;
        if (bH <= 0) { for (uint32_t f = 0; f < AL_REC_WORDS; ++f) R[f] = f == 0 ? 1 : 0; return; }
        const uint32_t sq = bi - bsi, st = bj - bsj;                 // the spans: sq = M + X + q_gap, st = M + X + t_gap
        R[0] = 0; R[1] = bH;
        R[2] = (int32_t)(P.rev ? lq - bi : bsi); R[3] = (int32_t)(P.rev ? lq - bsi : bi);      // on the read as given
        R[4] = (int32_t)bsj; R[5] = (int32_t)bj;
        R[6] = (int32_t)bm; R[7] = (int32_t)bx; R[8] = (int32_t)(sq - bm - bx); R[9] = (int32_t)(st - bm - bx);
    }
}

}  // namespace

void pair_align_affine_launch(hipStream_t stream, const align_pair *pairs, uint32_t n_pairs, const uint8_t *d_q, const uint8_t *d_t, uint2 *strips,
                              int32_t *recs, const rattle_align_scoring &S) {
    hipLaunchKernelGGL(pair_align_affine_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, stream, pairs, n_pairs, d_q, d_t, strips, recs,
                       (int32_t)S.match, (int32_t)S.mismatch, (int32_t)S.gap_open, (int32_t)S.gap_extend);
}

}  // namespace rattle
