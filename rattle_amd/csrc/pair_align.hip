// Kernel E: the local alignment of every placed read on its one transcript (include/rattle_hip.h, "align_pairs" and "align_pairs_scored";
// DESIGN.md, "Kernel E" and "Kernels E and F with three states").  One templated kernel in two forms.
//
// pair_align_kernel<false>: Smith-Waterman with LINEAR gaps (match +5, mismatch -4, gap -8 per gapped column) over the letters A, C, G, T = U:
//   H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), H[i-1][j] - 8, H[i][j-1] - 8),  H[0][*] = H[*][0] = 0,  i over the read, j over the transcript
// pair_align_kernel<true>: Gotoh's recurrence with AFFINE gaps, the four magnitudes m, x, o, e as a kernel argument (scalars;
// tests/align_affine_ref.py is the contract):
//   U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)      L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)
//   H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])      H[0][*] = H[*][0] = 0,  U[0][*] = L[*][0] = -inf
// A cell with H == 0 begins a new alignment; in H ties go diagonal, then up (U), then left (L); in U and in L open wins a tie with extend;
// the end cell is the largest H, ties to the smallest i, then the smallest j.  No traceback: every state of a cell carries (start_i,
// start_j, matches, mismatches) of the path the rule picks for it -- a gap step copies the payload of the state it comes from, a diagonal
// step out of a zero cell starts at the cell's own coordinates -- and the two gap counts follow from the spans (where lane 0 writes the
// record).  The linear form is the same body with both gap states opened from H alone (o = e = 8 makes U = H[i-1][j] - 8 exactly), so U
// and L are never kept or carried; it never reads the mismatch count either (that chain is dead code) and takes X from the score and the
// two spans.
//
// Shape: one wavefront per pair, four pairs per block, no LDS, the skewed form.  The read goes through in blocks of 64 rows, lane l owning
// row 64 b + l.  At step s lane l computes column s - l: `left` (H, and L with three states) is the lane's own previous cell, `up` (H,
// and U) is lane l - 1's previous cell and `diag` the H before that, both by the DPP wave_shr:1 -- five moves per step in the linear
// form, eleven in the affine -- and the transcript's letter slides down the lanes the same way.  Lane 0's `up` -- the last row of the
// block before -- comes from the pair's hand-over strip in device memory.  Linear: 16 bytes per column (H's score and start_i, start_j,
// matches), written by lane 63 with one 16-byte vector store per step.  Affine: 40 bytes per column (five uint2: H, its payload, U, its
// payload), five 8-byte stores.  The strip is read back 64 columns at a time, one record per lane and one refill ahead of its use, so no
// step waits on a load; the record of column s then reaches lane 0 by v_readlane.  The strip is updated in place: column c is read one
// refill before step 64 floor(c / 64) and written at step c + 63 of the same block, after the load's data has been consumed.  On the
// first block lane 0's U is PW_NEG, and a U or L that is kept is at least the H it was opened from less o: >= -64 in the local mode (o <= 64,
// H >= 0), above -2^29 - 64 in the read mode, where H goes down to -(o + e (Lq - 1)) -- never near PW_NEG (pair_wave.h).  Lanes whose cell is off the
// matrix keep their state frozen.  A lane keeps its best cell with a strict `>` over its rows in order (smallest i, then smallest j, per
// lane); the lanes are reduced once, at the end, by (score desc, i asc, j asc).  No wavefront waits for another; every load and store
// lies inside the pair's own two sequences, its own strip and its own record.
//
// The second template argument is the MODE (include/rattle_hip.h, "align_pairs_mode"; tests/align_ends_ref.py is the contract): <*, false>
// is the local alignment above, <*, true> (RATTLE_ALIGN_READ) aligns the read from its first base to its last with the transcript's
// ends free: H[0][j] = 0, H[i][0] = U[i][0] = -(o + (i - 1) e), no zero floor, the end cell the largest H of the last row (the smallest
// j).  In the same body: a lane starts with its row's border as `left` (lane 0 of a later block with the border of the row above as
// `diag`; the other lanes receive theirs from lane l - 1's frozen state); a path begins in row 0 alone -- the refill registers carry the
// payload (0, j, 0, 0) above the first block -- and a zero is an ordinary cell; only the lane that owns the last row keeps a best cell,
// from PW_NEG; every submitted pair has status 0.  The host keeps o + e (Lq - 1) below 2^29 (abi.hip), so PW_NEG is below every score.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "pair_wave.h"

namespace rattle {

namespace {

// a state of a cell: its score and the payload of its path
struct al_cell {
    int32_t s, i, j, m, x;
};

__device__ __forceinline__ al_cell al_pick(bool first, const al_cell &a, const al_cell &b) {
    al_cell r;
    r.s = first ? a.s : b.s; r.i = first ? a.i : b.i; r.j = first ? a.j : b.j; r.m = first ? a.m : b.m; r.x = first ? a.x : b.x;
    return r;
}

// A column of the strip in registers, as words: H {s, i, j, m} and with AFFINE H.x, U {s, i, j, m, x}.  Beyond the strip: H 0, U minus infinity.
template <bool AFFINE>
struct al_strip {
    static constexpr uint32_t WORDS = AFFINE ? AL_AFFINE_STRIP_BYTES / 4 : AL_STRIP_BYTES / 4;
    uint32_t w[WORDS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (uint32_t k = 0; k < WORDS; ++k) w[k] = 0;
        if constexpr (AFFINE) w[5] = (uint32_t)PW_NEG;
    }
    __device__ __forceinline__ void load(const uint32_t *col) {      // one uint4, or five uint2
        if constexpr (AFFINE) {
#pragma unroll
            for (uint32_t k = 0; k < WORDS / 2; ++k) { const uint2 v = reinterpret_cast<const uint2 *>(col)[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
        } else { const uint4 v = *reinterpret_cast<const uint4 *>(col); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    }
    __device__ __forceinline__ void store(uint32_t *col) const {
        if constexpr (AFFINE) {
#pragma unroll
            for (uint32_t k = 0; k < WORDS / 2; ++k) reinterpret_cast<uint2 *>(col)[k] = make_uint2(w[2 * k], w[2 * k + 1]);
        } else *reinterpret_cast<uint4 *>(col) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __device__ __forceinline__ int32_t lane(uint32_t word, uint32_t k) const { return __builtin_amdgcn_readlane((int32_t)w[word], k); }
};

template <bool AFFINE, bool READ>
__global__ __launch_bounds__(256) void pair_align_kernel(const align_pair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qseq,
                                                         const uint8_t *__restrict__ tseq, uint32_t *__restrict__ strips, int32_t *__restrict__ recs,
                                                         const rattle_align_scoring scoring) {
    constexpr uint32_t SW = al_strip<AFFINE>::WORDS;
    const rattle_align_scoring sc = AFFINE ? scoring : PW_LINEAR;    // the linear form's scores are compile-time constants
    const int32_t sm = (int32_t)sc.match, sx = (int32_t)sc.mismatch, so = (int32_t)sc.gap_open, se = (int32_t)sc.gap_extend;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const align_pair P = pairs[p];
    const uint32_t lq = P.lq, lt = P.lt;
    const uint8_t *q = qseq + P.q, *t = tseq + P.t;
    uint32_t *strip = strips + P.strip * SW;

    int32_t bH = READ ? PW_NEG : 0;                                  // the lane's best cell: score, end (i, j) as DP indices, payload
    uint32_t bi = 0, bj = 0, bsi = 0, bsj = 0, bm = 0, bx = 0;

    for (uint32_t r0 = 0; r0 < lq; r0 += AL_ROWS) {
        const uint32_t r = r0 + lane;                                // the lane's row: read base r (of the strand aligned)
        const bool row = r < lq;
        int32_t ql = 4;                                              // (matches nothing)
        if (row) { const uint32_t c = pw_code(q[P.rev ? lq - 1 - r : r]); ql = (int32_t)(P.rev ? 3 - c : c); }
        const bool from_strip = r0 > 0, to_strip = r0 + AL_ROWS < lq;
        const uint32_t n_steps = lt + min(AL_ROWS, lq - r0) - 1;       // the block's last row computes its last column at the last step
        // the lane's previous cell in its states (H and U go down the lanes, L stays), lane - 1's previous H as received one step ago
        // (diag), the sliding letter
        al_cell cH = {0, 0, 0, 0, 0}, cU = {PW_NEG, 0, 0, 0, 0}, cL = {PW_NEG, 0, 0, 0, 0}, dH = {0, 0, 0, 0, 0};
        if constexpr (READ) {
            // column 0 is a gap straight down from (0, 0): H = U = -(o + (i - 1) e) in DP row i = r + 1, start (0, 0).  Lanes l > 0 receive
            // the border of the row above as `diag` one step before their first column, from lane l - 1's frozen state; lane 0 of a
            // block behind the first starts with it
            cH.s = cU.s = -(so + (int32_t)r * se);
            if (from_strip) dH.s = -(so + (int32_t)(r0 - 1) * se);
        }
        int32_t tl = 4;
        // refill in flight: the transcript's letters and the strip's records of columns [S + 64, S + 128)
        int32_t nT = 4;
        al_strip<AFFINE> nR;
        nR.clear();
        if constexpr (READ) nR.w[2] = lane + 1;                      // above the first block lies row 0: column c begins a path at (0, c + 1)
        if (lane < lt) { nT = pw_code(t[lane]); if (from_strip) nR.load(strip + (uint64_t)lane * SW); }
        for (uint32_t S = 0; S < n_steps; S += 64) {
            const int32_t bT = nT;
            const al_strip<AFFINE> bR = nR;
            nT = 4; nR.clear();
            if constexpr (READ) nR.w[2] = S + 64 + lane + 1;
            if (S + 64 + lane < lt) { nT = pw_code(t[S + 64 + lane]); if (from_strip) nR.load(strip + (uint64_t)(S + 64 + lane) * SW); }
            const uint32_t k_end = min(64u, n_steps - S);
            for (uint32_t k = 0; k < k_end; ++k) {
                const uint32_t s = S + k;
                // lane 0's up cell and letter: column s of the buffers (H 0 and U minus infinity on the first block and beyond the transcript's end)
                const int32_t fT = __builtin_amdgcn_readlane(bT, k);
                al_cell uH, uU;
                uH.s = pw_shr1(cH.s, bR.lane(0, k)); uH.i = pw_shr1(cH.i, bR.lane(1, k));
                uH.j = pw_shr1(cH.j, bR.lane(2, k)); uH.m = pw_shr1(cH.m, bR.lane(3, k));
                if constexpr (AFFINE) {
                    uH.x = pw_shr1(cH.x, bR.lane(4, k));
                    uU.s = pw_shr1(cU.s, bR.lane(5, k)); uU.i = pw_shr1(cU.i, bR.lane(6, k)); uU.j = pw_shr1(cU.j, bR.lane(7, k));
                    uU.m = pw_shr1(cU.m, bR.lane(8, k)); uU.x = pw_shr1(cU.x, bR.lane(9, k));
                } else uH.x = 0;
                tl = pw_shr1(tl, fT);
                const uint32_t c = s - lane;                         // the lane's column (wraps below 0: fails the test)
                const bool on = row && c < lt;
                const bool eq = ql == tl;
                // the two gap states: open wins a tie with extend, and the payload is that of the state the step comes from (linear: H alone)
                al_cell nU = uH, nL = cH;
                if constexpr (AFFINE) {
                    nU = al_pick(uH.s - so >= uU.s - se, uH, uU); nL = al_pick(cH.s - so >= cL.s - se, cH, cL);
                    nU.s = max(uH.s - so, uU.s - se); nL.s = max(cH.s - so, cL.s - se);
                } else { nU.s = uH.s - so; nL.s = cH.s - so; }
                const int32_t d = dH.s + (eq ? sm : -sx), u = nU.s, l = nL.s;
                al_cell nH;
                if (d >= u && d >= l) {                              // diagonal first; a zero predecessor begins the alignment at this cell
                    const bool fresh = !READ && dH.s == 0;           // (READ: a path begins in row 0 alone, a zero is an ordinary cell)
                    nH.i = fresh ? (int32_t)r : dH.i; nH.j = fresh ? (int32_t)c : dH.j;
                    nH.m = (fresh ? 0 : dH.m) + (eq ? 1 : 0); nH.x = (fresh ? 0 : dH.x) + (eq ? 0 : 1);
                } else nH = al_pick(u >= l, nU, nL);                 // then up: a read base against a gap; then left: a transcript base against a gap
                nH.s = READ ? max(d, max(u, l)) : max(max(d, 0), max(u, l));
                dH = uH;
                if (on) {
                    cH = nH;                                         // (payload of a zero cell is never read: see `fresh`, and a gap state opened there stays < 0)
                    if constexpr (AFFINE) { cU = nU; cL = nL; }
                    if ((!READ || r + 1 == lq) && nH.s > bH) { bH = nH.s; bi = r + 1; bj = c + 1; bsi = (uint32_t)nH.i; bsj = (uint32_t)nH.j; bm = (uint32_t)nH.m; bx = (uint32_t)nH.x; }
                    if (to_strip && lane == 63) {                    // c < lt: inside the pair's strip
                        al_strip<AFFINE> o;
                        o.w[0] = (uint32_t)nH.s; o.w[1] = (uint32_t)nH.i; o.w[2] = (uint32_t)nH.j; o.w[3] = (uint32_t)nH.m;
                        if constexpr (AFFINE) {
                            o.w[4] = (uint32_t)nH.x;
                            o.w[5] = (uint32_t)nU.s; o.w[6] = (uint32_t)nU.i; o.w[7] = (uint32_t)nU.j; o.w[8] = (uint32_t)nU.m; o.w[9] = (uint32_t)nU.x;
                        }
                        o.store(strip + (uint64_t)c * SW);
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
        if (!READ && bH <= 0) { for (uint32_t f = 0; f < AL_REC_WORDS; ++f) R[f] = f == 0 ? 1 : 0; return; }
        const uint32_t sq = bi - bsi, st = bj - bsj;                 // the spans: sq = M + X + q_gap, st = M + X + t_gap
        // linear: S = 5 M - 4 X - 8 (q_gap + t_gap) with the spans  =>  12 X = 8 (sq + st) - 21 M + S
        const uint32_t X = AFFINE ? bx : (uint32_t)((8ll * ((long long)sq + st) - 21ll * bm + bH) / 12);
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
// (rattle_hip_align_*_scored) the form is GAP_AFFINE, the launches are those of the <true> kernels; the plan, the uploads and the records are the
// same, the strip's records are 40 bytes.  With mode RATTLE_ALIGN_READ (rattle_hip_align_*_mode) the launches are those of the <*, true>
// kernels under the ids of their gap form; every submitted pair comes back with status 0 and the rectangle (0, Lq] x (t_start, t_end].
// With cigars->want_pileup (rattle_hip_align_pileup) the call also owns kernel G's table (pair_pileup.hip): eight planes over the uploaded
// targets on the device, zeroed here, added to by every sub-chunk of pair_cigar_chunk, copied once into cigars->h_pileup at the end.
int align_pairs_run(rattle_ctx *ctx, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff, uint32_t nr,
                    const int32_t *target, const uint8_t *rev, const rattle_align_params *AP, rattle_alignment *A, cigar_run *cigars, const rattle_align_scoring *scoring,
                    int mode) {
    phase_timer T_all("align_pairs: total");
    const gap_form &F = scoring ? GAP_AFFINE : GAP_LINEAR;
    align_plan plan;
    plan_align(toff, roff, nr, target, AP->max_cells, AP->pair_chunk ? AP->pair_chunk : 32768u, (1ull << 30) / F.strip_bytes /* 1 GiB of records */, plan);
    for (uint32_t r = 0; r < nr; ++r) A->status[r] = plan.status[r];
    const bool pileup = cigars && cigars->want_pileup;
    if (pileup) {                                                    // the host table: zero wherever nothing is counted
        cigars->h_pileup = (uint32_t *)calloc(std::max<uint64_t>(1, 8 * toff[nt]), 4);
        if (!cigars->h_pileup) { set_error("align_pileup: out of memory (the table of " + std::to_string(toff[nt]) + " positions)"); return RATTLE_ERR_HIP; }
    }
    if (plan.sub.empty()) return 0;
    const std::vector<uint32_t> &sub = plan.sub, &first = plan.first;
    const std::vector<uint64_t> &strip_len = plan.strip;

    const uint64_t t0 = toff[0], tbytes = toff[nt] - t0;
    dbuf<uint8_t> d_t, d_q;
    dbuf<align_pair> d_pairs;
    dbuf<uint32_t> d_strip;
    dbuf<int32_t> d_rec;
    hbuf<align_pair> h_pairs;
    hbuf<int32_t> h_rec;
    RT_TRY(d_t.reserve(tbytes));
    RT_HIP(hipMemcpyAsync(d_t.p, tseq + t0, tbytes, hipMemcpyHostToDevice, ctx->stream));
    dbuf<uint32_t> d_pile;                                           // kernel G's table: zeroed once, added to by every sub-chunk, copied back once
    if (pileup) {
        RT_TRY(d_pile.reserve(8 * tbytes));
        RT_HIP(hipMemsetAsync(d_pile.p, 0, 8 * tbytes * 4, ctx->stream));
        cigars->d_pileup = d_pile.p; cigars->pileup_n = tbytes;
    }
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
        RT_TRY(d_strip.reserve(std::max<uint64_t>(1, strip_recs * (F.strip_bytes / 4))));      // (words)
        RT_TRY(d_rec.reserve((size_t)n * AL_REC_WORDS));
        RT_TRY(h_rec.reserve((size_t)n * AL_REC_WORDS));
        RT_HIP(hipMemcpyAsync(d_q.p, rseq + q0, qbytes, hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(hipMemcpyAsync(d_pairs.p, h_pairs.p, (size_t)n * sizeof(align_pair), hipMemcpyHostToDevice, ctx->stream));
        {
            ktimer kt(ctx, F.k_align, seq_bytes + (uint64_t)n * AL_REC_WORDS * 4);
            const auto kernel = mode == RATTLE_ALIGN_READ ? (scoring ? pair_align_kernel<true, true> : pair_align_kernel<false, true>)
                                                          : (scoring ? pair_align_kernel<true, false> : pair_align_kernel<false, false>);
            hipLaunchKernelGGL(kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_pairs.p, n, d_q.p, d_t.p, d_strip.p, d_rec.p, scoring ? *scoring : PW_LINEAR);
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
                if (A->q_start[r] > A->q_end[r] || A->q_end[r] > P.lq || A->t_start[r] > A->t_end[r] || A->t_end[r] > P.lt) {
                    set_error("align_cigars: a record of kernel E lies outside its pair");      // (never: kernel F must not be handed such a rectangle)
                    return RATTLE_ERR_HIP;
                }
                I.rows = A->q_end[r] - A->q_start[r]; I.cols = A->t_end[r] - A->t_start[r];
                I.q = P.q + (P.rev ? (uint64_t)A->q_end[r] - (I.rows ? 1 : 0) : (uint64_t)A->q_start[r]); I.t = P.t + A->t_start[r];
            }
            RT_TRY(pair_cigar_chunk(ctx, d_q.p, d_t.p, in.data(), n, AP->pair_chunk ? AP->pair_chunk : 32768u, *cigars, scoring, mode));
        }
    }
    if (pileup) {
        // plane k of the device table is positions [t0, t0 + tbytes) of plane k of the caller's; the ins adds of id 11's alg_bytes, 4 bytes each
        const uint64_t N = toff[nt];
        cigars->d_pileup = nullptr;
        for (uint32_t k = 0; k < 8; ++k)
            RT_HIP(hipMemcpyAsync(cigars->h_pileup + k * N + t0, d_pile.p + k * tbytes, tbytes * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
        uint64_t ins = 0;
        for (uint64_t i = 0; i < N; ++i) ins += cigars->h_pileup[5 * N + i];
        ctx->stats[K_PILEUP].bytes += 4 * ins;
    }
    return 0;
}

}  // namespace rattle
