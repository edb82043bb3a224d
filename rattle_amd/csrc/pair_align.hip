// Kernel E: the local alignment of every placed read on its one transcript (include/rattle_hip.h, "align_pairs"; DESIGN.md, "Kernel E").
//
// Smith-Waterman with LINEAR gaps (match +5, mismatch -4, gap -8 per gapped column) over the letters A, C, G, T = U:
//   H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), H[i-1][j] - 8, H[i][j-1] - 8),  H[0][*] = H[*][0] = 0,  i over the read, j over the transcript
// A cell with H == 0 begins a new alignment; predecessors that tie are taken diagonal, then up, then left; the end cell is the largest H, ties
// to the smallest i, then the smallest j.  No traceback: every cell carries (start_i, start_j, matches) of the path the rule picks, taken from
// the predecessor it picks, and the other counts follow from the score and the two spans (where lane 0 writes the record).
//
// Shape: one wavefront per pair, the skewed form.  The read goes through in blocks of 64 rows, lane l owning row 64 b + l.  At step s lane l
// computes column s - l: `left` is the lane's own previous cell, `up` is lane l - 1's previous cell and `diag` the one before that, both by the
// DPP wave_shr:1, and the transcript's letter slides down the lanes the same way.  Lane 0's `up` -- the last row of the block before -- comes
// from the pair's hand-over strip in device memory, 16 bytes (score + payload) per column: lane 63 writes it with one 16-byte vector store per
// step, and it is read back 64 columns at a time, one record per lane and one refill ahead of its use, so no step waits on a load; the record
// of column s then reaches lane 0 by v_readlane.  The strip is updated in place: column c is read one refill before step 64 floor(c / 64) and
// written at step c + 63 of the same block, after the load's data has been consumed.  A lane keeps its best cell with a strict `>` over its rows in order (smallest i, then smallest j, per lane); the
// lanes are reduced once, at the end, by (score desc, i asc, j asc).  No wavefront waits for another; every load and store lies inside the
// pair's own two sequences, its own strip and its own record.
#include <algorithm>
#include <cstring>

#include "align_plan.h"
#include "common.h"

namespace rattle {

namespace {

constexpr int32_t AL_MATCH = 5, AL_MISMATCH = -4, AL_GAP = -8;

// value of lane - 1 (lane 0 receives `fill`): the helper of poa.hip
__device__ __forceinline__ int32_t al_shr1(int32_t v, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
}

// A 0, C 1, G 2, T and U 3 (the complement of code c is 3 - c); the host has refused every other byte
__device__ __forceinline__ int32_t al_code(uint32_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3; }

__global__ __launch_bounds__(256) void pair_align_kernel(const align_pair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qseq,
                                                         const uint8_t *__restrict__ tseq, uint4 *__restrict__ strips, int32_t *__restrict__ recs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const align_pair P = pairs[p];
    const uint32_t lq = P.lq, lt = P.lt;
    const uint8_t *q = qseq + P.q, *t = tseq + P.t;
    uint4 *strip = strips + P.strip;

    int32_t bH = 0;                                                  // the lane's best cell: score, end (i, j) as DP indices, payload
    uint32_t bi = 0, bj = 0, bsi = 0, bsj = 0, bm = 0;

    for (uint32_t r0 = 0; r0 < lq; r0 += AL_ROWS) {
        const uint32_t r = r0 + lane;                                // the lane's row: read base r (of the strand aligned)
        const bool row = r < lq;
        int32_t ql = 4;                                              // (matches nothing)
        if (row) { const uint32_t c = al_code(q[P.rev ? lq - 1 - r : r]); ql = (int32_t)(P.rev ? 3 - c : c); }
        const bool from_strip = r0 > 0, to_strip = r0 + AL_ROWS < lq;
        const uint32_t n_steps = lt + min(AL_ROWS, lq - r0) - 1;       // the block's last row computes its last column at the last step
        // the lane's previous cell (left), lane - 1's previous cell as received one step ago (diag), the sliding letter
        int32_t cH = 0, cI = 0, cJ = 0, cM = 0, dH = 0, dI = 0, dJ = 0, dM = 0, tl = 4;
        // refill in flight: the transcript's letters and the strip's records of columns [S + 64, S + 128)
        int32_t nT = 4;
        uint4 nR = make_uint4(0, 0, 0, 0);
        if (lane < lt) { nT = al_code(t[lane]); if (from_strip) nR = strip[lane]; }
        for (uint32_t S = 0; S < n_steps; S += 64) {
            const int32_t bT = nT;
            const uint4 bR = nR;
            nT = 4; nR = make_uint4(0, 0, 0, 0);
            if (S + 64 + lane < lt) { nT = al_code(t[S + 64 + lane]); if (from_strip) nR = strip[S + 64 + lane]; }
            const uint32_t k_end = min(64u, n_steps - S);
            for (uint32_t k = 0; k < k_end; ++k) {
                const uint32_t s = S + k;
                // lane 0's up cell and letter: column s of the buffers (zeros on the first block and beyond the transcript's end)
                const int32_t fT = __builtin_amdgcn_readlane(bT, k);
                const int32_t fH = __builtin_amdgcn_readlane((int32_t)bR.x, k), fI = __builtin_amdgcn_readlane((int32_t)bR.y, k);
                const int32_t fJ = __builtin_amdgcn_readlane((int32_t)bR.z, k), fM = __builtin_amdgcn_readlane((int32_t)bR.w, k);
                const int32_t uH = al_shr1(cH, fH), uI = al_shr1(cI, fI), uJ = al_shr1(cJ, fJ), uM = al_shr1(cM, fM);
                tl = al_shr1(tl, fT);
                const uint32_t c = s - lane;                         // the lane's column (wraps below 0: fails the test)
                const bool on = row && c < lt;
                const bool eq = ql == tl;
                const int32_t d = dH + (eq ? AL_MATCH : AL_MISMATCH), u = uH + AL_GAP, l = cH + AL_GAP;
                const int32_t h = max(max(d, 0), max(u, l));
                int32_t nI, nJ, nM;
                if (d >= u && d >= l) {                              // diagonal first; a zero predecessor begins the alignment at this cell
                    const bool fresh = dH == 0;
                    nI = fresh ? (int32_t)r : dI; nJ = fresh ? (int32_t)c : dJ; nM = (fresh ? 0 : dM) + (eq ? 1 : 0);
                } else if (u >= l) { nI = uI; nJ = uJ; nM = uM; }    // then up: a read base against a gap
                else { nI = cI; nJ = cJ; nM = cM; }                  // then left: a transcript base against a gap
                dH = uH; dI = uI; dJ = uJ; dM = uM;
                if (on) {
                    cH = h; cI = nI; cJ = nJ; cM = nM;               // (payload of a zero cell is never read: see `fresh`, and u, l < 0 there)
                    if (h > bH) { bH = h; bi = r + 1; bj = c + 1; bsi = (uint32_t)nI; bsj = (uint32_t)nJ; bm = (uint32_t)nM; }
                    if (to_strip && lane == 63) strip[c] = make_uint4((uint32_t)h, (uint32_t)nI, (uint32_t)nJ, (uint32_t)nM);
                }
            }
        }
        __threadfence();                                             // the strip's stores of this block before the next block's loads
    }

    // the best of the 64 lanes: score desc, i asc, j asc (a lane without a positive cell loses to every other)
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t oH = __shfl_xor(bH, off);
        const uint32_t oi = __shfl_xor(bi, off), oj = __shfl_xor(bj, off), osi = __shfl_xor(bsi, off), osj = __shfl_xor(bsj, off), om = __shfl_xor(bm, off);
        if (oH > bH || (oH == bH && (oi < bi || (oi == bi && oj < bj)))) { bH = oH; bi = oi; bj = oj; bsi = osi; bsj = osj; bm = om; }
    }
    if (lane == 0) {
        int32_t *R = recs + (size_t)p * AL_REC_WORDS;
        if (bH <= 0) { for (uint32_t f = 0; f < AL_REC_WORDS; ++f) R[f] = f == 0 ? 1 : 0; return; }
        // spans sq, st; S = 5 M - 4 X - 8 (q_gap + t_gap), sq = M + X + q_gap, st = M + X + t_gap  =>  12 X = 8 (sq + st) - 21 M + S
        const uint32_t sq = bi - bsi, st = bj - bsj;
        const uint32_t X = (uint32_t)((8ll * ((long long)sq + st) - 21ll * bm + bH) / 12);
        R[0] = 0; R[1] = bH;
        R[2] = (int32_t)(P.rev ? lq - bi : bsi); R[3] = (int32_t)(P.rev ? lq - bsi : bi);      // on the read as given
        R[4] = (int32_t)bsj; R[5] = (int32_t)bj;
        R[6] = (int32_t)bm; R[7] = (int32_t)X; R[8] = (int32_t)(sq - bm - X); R[9] = (int32_t)(st - bm - X);
    }
}

}  // namespace

// Every read r with target_of_read[r] >= 0, both sequences non-empty and (max_cells == 0 or lq * lt <= max_cells) is aligned; the arguments
// have been checked (abi.hip).  Fills every array of A.  The plan -- statuses settled without the device, strip records, chunks -- is
// align_plan.h's; the strip buffer is sized from the lengths of the chunk.  With `cigars` (rattle_hip_align_cigars) every chunk's records go on
// to kernel F (pair_cigar.hip) while the chunk's sequences are on the device; A is filled exactly as without.  With `scoring`
// (rattle_hip_align_*_scored) the launches are those of the three-state kernels (pair_align_affine.hip, pair_cigar_affine.hip); the plan, the
// uploads and the records are the same, the strip's records are 40 bytes.
int align_pairs_run(rattle_ctx *ctx, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff, uint32_t nr,
                    const int32_t *target, const uint8_t *rev, const rattle_align_params *AP, rattle_alignment *A, cigar_run *cigars, const rattle_align_scoring *scoring) {
    phase_timer T_all("align_pairs: total");
    align_plan plan;
    plan_align(toff, roff, nr, target, AP->max_cells, AP->pair_chunk ? AP->pair_chunk : 32768u,
               scoring ? (1ull << 30) / AL_AFFINE_STRIP_BYTES : 1ull << 26 /* 1 GiB of records */, plan);
    for (uint32_t r = 0; r < nr; ++r) A->status[r] = plan.status[r];
    if (plan.sub.empty()) return 0;
    const std::vector<uint32_t> &sub = plan.sub, &first = plan.first;
    const std::vector<uint64_t> &strip_len = plan.strip;

    const uint64_t t0 = toff[0], tbytes = toff[nt] - t0;
    dbuf<uint8_t> d_t, d_q;
    dbuf<align_pair> d_pairs;
    dbuf<uint4> d_strip;
    dbuf<int32_t> d_rec;
    hbuf<align_pair> h_pairs;
    hbuf<int32_t> h_rec;
    RT_TRY(d_t.reserve(tbytes));
    RT_HIP(hipMemcpyAsync(d_t.p, tseq + t0, tbytes, hipMemcpyHostToDevice, ctx->stream));
    for (size_t c = 0; c + 1 < first.size(); ++c) {
        const uint32_t a = first[c], n = first[c + 1] - a;
        // the chunk's reads: one span of the caller's buffer, from its first submitted read to its last
        const uint64_t q0 = roff[sub[a]], qbytes = roff[sub[a + n - 1] + 1] - q0;
        RT_TRY(h_pairs.reserve(n));
        uint64_t strip_recs = 0, seq_bytes = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t r = sub[a + i];
            const uint32_t x = (uint32_t)target[r];
            align_pair &P = h_pairs.p[i];
            P.q = roff[r] - q0; P.t = toff[x] - t0; P.strip = strip_recs;
            P.lq = (uint32_t)(roff[r + 1] - roff[r]); P.lt = (uint32_t)(toff[x + 1] - toff[x]); P.rev = rev[r]; P.pad = 0;
            strip_recs += strip_len[a + i];
            seq_bytes += (uint64_t)P.lq + P.lt;
        }
        RT_TRY(d_q.reserve(qbytes));
        RT_TRY(d_pairs.reserve(n));
        RT_TRY(d_strip.reserve(std::max<uint64_t>(1, scoring ? (strip_recs * (AL_AFFINE_STRIP_BYTES / 8) + 1) / 2 : strip_recs)));      // (uint4s)
        RT_TRY(d_rec.reserve((size_t)n * AL_REC_WORDS));
        RT_TRY(h_rec.reserve((size_t)n * AL_REC_WORDS));
        RT_HIP(hipMemcpyAsync(d_q.p, rseq + q0, qbytes, hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(hipMemcpyAsync(d_pairs.p, h_pairs.p, (size_t)n * sizeof(align_pair), hipMemcpyHostToDevice, ctx->stream));
        {
            ktimer kt(ctx, scoring ? K_ALIGN_AFFINE : K_ALIGN, seq_bytes + (uint64_t)n * AL_REC_WORDS * 4);
            if (scoring) pair_align_affine_launch(ctx->stream, d_pairs.p, n, d_q.p, d_t.p, (uint2 *)d_strip.p, d_rec.p, *scoring);
            else hipLaunchKernelGGL(pair_align_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_pairs.p, n, d_q.p, d_t.p, d_strip.p, d_rec.p);
            RT_HIP(hipGetLastError());
        }
        RT_HIP(hipMemcpyAsync(h_rec.p, d_rec.p, (size_t)n * AL_REC_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));                   // (also: h_pairs is free for the next chunk)
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t r = sub[a + i];
            const int32_t *R = h_rec.p + (size_t)i * AL_REC_WORDS;
            A->status[r] = (uint8_t)R[0]; A->score[r] = R[1];
            A->q_start[r] = (uint32_t)R[2]; A->q_end[r] = (uint32_t)R[3]; A->t_start[r] = (uint32_t)R[4]; A->t_end[r] = (uint32_t)R[5];
            A->matches[r] = (uint32_t)R[6]; A->mismatches[r] = (uint32_t)R[7]; A->q_gap[r] = (uint32_t)R[8]; A->t_gap[r] = (uint32_t)R[9];
        }
        if (cigars) {
            // kernel F on the chunk's rectangles, while d_q and d_t hold its sequences: rows (q_start, q_end] of the read as given, taken from
            // its far end on the reverse strand, and columns (t_start, t_end] of the target
            std::vector<cigar_in> in(n);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t r = sub[a + i];
                const align_pair &P = h_pairs.p[i];
                cigar_in &I = in[i];
                I.status = A->status[r]; I.rev = rev[r]; I.read = r;
                I.rows = A->q_end[r] - A->q_start[r]; I.cols = A->t_end[r] - A->t_start[r];
                I.q = P.q + (P.rev ? (uint64_t)A->q_end[r] - (I.rows ? 1 : 0) : (uint64_t)A->q_start[r]); I.t = P.t + A->t_start[r];
            }
            RT_TRY(pair_cigar_chunk(ctx, d_q.p, d_t.p, in.data(), n, AP->pair_chunk ? AP->pair_chunk : 32768u, *cigars, scoring));
        }
    }
    return 0;
}

}  // namespace rattle
