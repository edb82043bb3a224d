// Kernel F: the CIGAR of every pair kernel E aligned (include/rattle_hip.h, "align_cigars" and "align_cigars_scored"; DESIGN.md, "Kernel F"
// and "Kernels E and F with three states").  One templated kernel in the two forms of kernel E (pair_align.hip): pair_cigar_kernel<false>
// with linear gaps at 5,4,8,8, pair_cigar_kernel<true> with affine gaps and the caller's scoring (tests/align_affine_ref.py is the contract).
//
// Kernel E's record gives a pair its rectangle on the aligned strand: `rows` read bases from the alignment's first to its last, `cols`
// transcript bases likewise.  The same recurrence over the rectangle alone (H' = 0, and U' = L' = -inf, on its top row and left column)
// reproduces the full matrices on every (cell, state) of the chosen path and is nowhere larger (DESIGN.md states the lemmas,
// tests/test_cigar_ref.py and tests/test_align_affine_ref.py check them), so a walk back from H' of the rectangle's last cell is the walk
// of the full matrices and ends at the rectangle's first cell.
//
// Forward pass: one wavefront per pair, kernel E's skewed form (pair_wave.h) with the scores alone: what crosses a row -- H, and U with
// three states -- and the sliding letter by the DPP wave_shr:1, L stays in the lane; lane 0's `up` from the pair's hand-over strip (one
// 4-byte word per column, two with three states: H and U; read 64 columns at a time one refill ahead, updated in place behind the reads as
// in kernel E).  Each cell's decision is H's 2-bit code (0 zero cell: the path stops, 1 diagonal, 2 up / U, 3 left / L), from kernel E's
// selects, and with three states two more bits, "U extends" and "L extends" (open wins a tie, so a bit is set only where extend is
// strictly larger).  One ballot per bit and step makes the record of (block, step), an anti-diagonal of 64 cells: one uint4 (the code's
// low and high bit), with three states a second one (the U and the L bit).  Lane k keeps the record of step S + k of the current 64
// steps, and the 64 records go out as one coalesced store; lane 63's scores for the strip leave the same way.  A block's records lie
// cols + 63 apart.
//
// Walk: the same wavefront, after a device-scope fence.  The position (block, lane, column) is wave-uniform, and so is the state
// H | U | L of the affine form (the linear form is always in H).  A window holds 64 consecutive records of one block, one per lane; every
// lane shifts the walk's row out of its own record, and v_readlane by the step's index fetches the code: a diagonal move goes back two
// steps, up and left one, up out of lane 0 goes to lane 63 of the block above (a new window).  In H a code of 1 emits = / X and moves
// diagonally; the letters come from two windows of the same kind (the block's 64 read bases, 64 transcript bases).  A code of 2 or 3
// emits I or D and moves at once in the linear form; in the affine form it switches to U or L WITHOUT moving.  In U the walk emits I and
// moves up, and the U bit OF THE CELL IT LEFT says whether it stays in U (that cell's U came from the U above) or lands in H; L is the
// same with D, moving left.  Runs are merged in scalar registers; lane 0 writes a finished run as len << 4 | op (BAM's numbers) from the
// end of the pair's ops region backwards, so the ops lie in start-to-end order, and the run count beside them.
//
// Bounds: every loop runs over the pair's own lengths.  An emitting move lowers the row or the column and the walk ends at row 0 or
// column 0, so at most rows + cols moves emit; a switch of state is followed by an emitting move, and the loop is cut at rows + cols
// (affine: twice that) iterations whatever the codes say.  The window index is step - window start in [0, 64) by construction; the ops
// cursor is checked before every store.  Every load and store lies in the pair's own sequences, strip, records, ops region or count.  A
// wrong code gives a wrong string, never a hang or a store out of range.
//
// The second template argument is kernel E's MODE.  <*, true> (RATTLE_ALIGN_READ): the rectangle is every row of the read and columns
// (t_start, t_end], its borders are the mode's -- top row H' = 0, U' = L' = -inf; left column H' = U' = -(o + (i - 1) e), L' = -inf (DESIGN.md,
// "The read mode", has the lemma, tests/test_align_ends_ref.py checks it) -- there is no zero floor and code 0 means a cell off the matrix
// alone.  The walk is the same loop, and may begin with a switch into U; when it leaves through the left column with rows above it,
// those rows are the border's gap: one I run of that many rows, whatever blocks they span, added to the run at hand behind the loop in a
// bounded number of rounds, through the same checked ops cursor.  A pair without a column never comes here (cigar_no_column, below).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.h"
#include "pair_wave.h"

namespace rattle {

namespace {

constexpr uint32_t CG_H = 0, CG_U = 1, CG_L = 2;                              // the walk's state

template <bool AFFINE, bool READ>
__global__ __launch_bounds__(256) void pair_cigar_kernel(const cigar_pair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qseq,
                                                         const uint8_t *__restrict__ tseq, uint4 *__restrict__ codes, int32_t *__restrict__ strips,
                                                         uint32_t *__restrict__ ops, uint32_t *__restrict__ counts, const rattle_align_scoring scoring) {
    constexpr uint32_t RW = AFFINE ? CG_AFFINE_REC_BYTES / 16 : CG_REC_BYTES / 16;      // uint4s of a record
    const rattle_align_scoring sc = AFFINE ? scoring : PW_LINEAR;    // the linear form's scores are compile-time constants
    const int32_t sm = (int32_t)sc.match, sx = (int32_t)sc.mismatch, so = (int32_t)sc.gap_open, se = (int32_t)sc.gap_extend;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n_pairs) return;                                        // wave-uniform
    const cigar_pair P = pairs[p];
    const uint32_t sq = pw_uniform(P.rows), st = pw_uniform(P.cols), rev = pw_uniform(P.rev);
    // row r of the rectangle is read base q[r] (forward) or the complement of q[-r] (reverse: q points at the last base of the span)
    const uint8_t *q = qseq + P.q, *t = tseq + P.t;
    uint4 *code = codes + RW * P.codes;
    int32_t *strip = strips + P.strip;                               // (the plan counts words: AFFINE two per column, H and U)
    uint32_t *op = ops + P.ops;
    const uint64_t stride = (uint64_t)st + CG_ROWS - 1;               // records of one block
    auto strip_load = [&](uint32_t col, int32_t &h, int32_t &u) {
        if constexpr (AFFINE) { const int2 v = reinterpret_cast<const int2 *>(strip)[col]; h = v.x; u = v.y; }
        else h = strip[col];
    };

    // ---- forward: the codes of every cell of the rectangle ----
    for (uint32_t r0 = 0, b = 0; r0 < sq; r0 += CG_ROWS, ++b) {
        const uint32_t r = r0 + lane;                                // the lane's row
        const bool row = r < sq;
        int32_t ql = 4;                                              // (matches nothing)
        if (row) ql = rev ? 3 - pw_code(*(q - r)) : pw_code(q[r]);
        const bool from_strip = r0 > 0, to_strip = r0 + CG_ROWS < sq;
        const uint32_t n_steps = st + min(CG_ROWS, sq - r0) - 1;     // the block's last row computes its last column at the last step
        uint4 *rec_b = code + RW * ((uint64_t)b * stride);
        int32_t cH = 0, cU = PW_NEG, cL = PW_NEG, dH = 0, tl = 4;    // the lane's previous cell in its states, lane - 1's H as received one step ago (diag)
        if constexpr (READ) {                                        // the left border is a gap straight down: kernel E's values (pair_align.hip)
            cH = cU = -(so + (int32_t)r * se);
            if (from_strip) dH = -(so + (int32_t)(r0 - 1) * se);
        }
        // refill in flight: the transcript's letters and the strip's scores (H, U) of columns [S + 64, S + 128)
        int32_t nT = 4, nH = 0, nU = PW_NEG;
        if (lane < st) { nT = pw_code(t[lane]); if (from_strip) strip_load(lane, nH, nU); }
        for (uint32_t S = 0; S < n_steps; S += 64) {
            const int32_t bT = nT, bH = nH, bU = nU;
            nT = 4; nH = 0; nU = PW_NEG;
            if (S + 64 + lane < st) { nT = pw_code(t[S + 64 + lane]); if (from_strip) strip_load(S + 64 + lane, nH, nU); }
            const uint32_t k_end = min(64u, n_steps - S);
            uint4 rec0 = make_uint4(0, 0, 0, 0), rec1 = make_uint4(0, 0, 0, 0);      // lane k: the record of step S + k
            int32_t lastH = 0, lastU = PW_NEG;                       // lane k: lane 63's H and U after step S + k, column S + k - 63
            for (uint32_t k = 0; k < k_end; ++k) {
                const uint32_t s = S + k;
                // lane 0's up cell and letter: column s of the buffers (H 0 and U minus infinity on the first block and beyond the transcript's end)
                const int32_t fT = __builtin_amdgcn_readlane(bT, k);
                const int32_t uH = pw_shr1(cH, __builtin_amdgcn_readlane(bH, k));
                tl = pw_shr1(tl, fT);
                const uint32_t c = s - lane;                         // the lane's column (wraps below 0: fails the test)
                const bool on = row && c < st;
                const int32_t uo = uH - so, lo_ = cH - so;           // the gap states opened from H: all there is in the linear form
                int32_t ue = 0, le = 0;                              // ... and extended, with three states
                if constexpr (AFFINE) { ue = pw_shr1(cU, __builtin_amdgcn_readlane(bU, k)) - se; le = cL - se; }
                const int32_t u = AFFINE ? max(uo, ue) : uo, l = AFFINE ? max(lo_, le) : lo_;
                const int32_t d = dH + (ql == tl ? sm : -sx);
                const int32_t h = READ ? max(d, max(u, l)) : max(max(d, 0), max(u, l));
                // diagonal, then up, then left; READ: no zero cells, code 0 is a cell off the matrix alone
                const uint32_t cd = !on || (!READ && h == 0) ? 0u : d >= u && d >= l ? 1u : u >= l ? 2u : 3u;
                dH = uH;
                if (on) { cH = h; cU = u; cL = l; }
                const bool mine = lane == k;
                const uint64_t b0 = __ballot(cd & 1u), b1 = __ballot(cd & 2u);
                rec0.x = mine ? (uint32_t)b0 : rec0.x; rec0.y = mine ? (uint32_t)(b0 >> 32) : rec0.y;
                rec0.z = mine ? (uint32_t)b1 : rec0.z; rec0.w = mine ? (uint32_t)(b1 >> 32) : rec0.w;
                if constexpr (AFFINE) {
                    const uint64_t b2 = __ballot(on && ue > uo), b3 = __ballot(on && le > lo_);
                    rec1.x = mine ? (uint32_t)b2 : rec1.x; rec1.y = mine ? (uint32_t)(b2 >> 32) : rec1.y;
                    rec1.z = mine ? (uint32_t)b3 : rec1.z; rec1.w = mine ? (uint32_t)(b3 >> 32) : rec1.w;
                }
                if (to_strip) {
                    const int32_t h63 = __builtin_amdgcn_readlane(cH, 63);
                    lastH = mine ? h63 : lastH;
                    if constexpr (AFFINE) { const int32_t u63 = __builtin_amdgcn_readlane(cU, 63); lastU = mine ? u63 : lastU; }
                }
            }
            if (lane < k_end) {
                rec_b[RW * (uint64_t)(S + lane)] = rec0;             // S + lane < n_steps <= stride
                if constexpr (AFFINE) rec_b[RW * (uint64_t)(S + lane) + 1] = rec1;
                const uint32_t cc = S + lane - 63;                   // lane 63's column at that step (wraps below 0: fails the test)
                if (to_strip && S + lane >= 63 && cc < st) {         // behind every read of the strip: columns <= S were loaded a refill ago
                    if constexpr (AFFINE) reinterpret_cast<int2 *>(strip)[cc] = make_int2(lastH, lastU);
                    else strip[cc] = lastH;
                }
            }
        }
        __threadfence();                                             // the strip's stores of this block before the next block's loads; the records before the walk
    }

    // ---- walk: from H of the rectangle's last cell back to its first ----
    uint32_t b = (sq - 1) >> 6, L = (sq - 1) & 63u, c = st - 1;      // block, lane (row 64 b + L), column
    const uint32_t region = sq + st;                                 // words of the ops region = the most moves that emit
    uint32_t pos = region, run_op = 0, run_len = 0, state = CG_H;
    uint32_t left_rows = 0;                                          // READ: rows above the walk when it leaves through the left column
    uint32_t wb = ~0u, W = 0, qb = ~0u, T0 = ~0u;                    // the windows: block and first step of the records, block of the read bases, first column
    uint4 win0 = make_uint4(0, 0, 0, 0), win1 = make_uint4(0, 0, 0, 0);
    int32_t qw = 4, tw = 4;
    using iter_t = std::conditional_t<AFFINE, uint64_t, uint32_t>;   // (twice the region need not fit 32 bits)
    for (iter_t it = 0; it < (iter_t)(AFFINE ? 2 : 1) * region; ++it) {
        const uint32_t s = c + L;
        if (b != wb || s < W || s - W >= 64) {                       // records [W, W + 64) of block b, W + 63 = s unless the block begins before
            wb = b; W = s >= 63 ? s - 63 : 0;
            win0 = make_uint4(0, 0, 0, 0); win1 = make_uint4(0, 0, 0, 0);
            if (W + lane <= s) {
                win0 = code[RW * ((uint64_t)b * stride + W + lane)];
                if constexpr (AFFINE) win1 = code[RW * ((uint64_t)b * stride + W + lane) + 1];
            }
        }
        const uint32_t sh = L & 31u;
        uint32_t mine = (((L < 32 ? win0.x : win0.y) >> sh) & 1u) | ((((L < 32 ? win0.z : win0.w) >> sh) & 1u) << 1);
        if constexpr (AFFINE) mine |= ((((L < 32 ? win1.x : win1.y) >> sh) & 1u) << 2) | ((((L < 32 ? win1.z : win1.w) >> sh) & 1u) << 3);
        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int32_t)mine, s - W);
        uint32_t mv;                                                 // the move, as H's code: 1 diagonal, 2 up, 3 left
        if (!AFFINE || state == CG_H) {
            mv = AFFINE ? cd & 3u : cd;
            if (mv == 0) break;                                      // a zero cell: the path begins behind it
            if (AFFINE && mv != 1) { state = mv == 2 ? CG_U : CG_L; continue; }      // into a gap state of the same cell: no move
        } else if (state == CG_U) {
            mv = 2;
            if (!(cd & 4u)) state = CG_H;                            // this cell's U was opened from the H above
        } else {
            mv = 3;
            if (!(cd & 8u)) state = CG_H;
        }
        uint32_t o = mv == 2 ? PW_OP_I : PW_OP_D;
        if (mv == 1) {
            if (b != qb) {
                qb = b; qw = 4;
                const uint32_t r = b * CG_ROWS + lane;
                if (r < sq) qw = rev ? 3 - pw_code(*(q - r)) : pw_code(q[r]);
            }
            if (c < T0 || c - T0 >= 64) {
                T0 = c >= 63 ? c - 63 : 0; tw = 4;
                if (T0 + lane <= c) tw = pw_code(t[T0 + lane]);
            }
            o = __builtin_amdgcn_readlane(qw, L) == __builtin_amdgcn_readlane(tw, c - T0) ? PW_OP_EQ : PW_OP_X;
        }
        if (o == run_op && run_len < PW_MAX_RUN) ++run_len;
        else {
            if (run_len && pos) { --pos; if (lane == 0) op[pos] = run_len << 4 | run_op; }
            run_op = o; run_len = 1;
        }
        bool done = false;
        if (mv != 3) { if (L) --L; else if (b) { --b; L = 63; } else done = true; }      // up out of lane 0: lane 63 of the block above
        if (mv != 2) {
            if (c) --c;
            else {
                if constexpr (READ) if (!done) left_rows = b * CG_ROWS + L + 1;      // in the left column with rows above: (b, L) is the row the walk stands in
                done = true;
            }
        }
        if (done) break;                                             // the rectangle's top row or left column
    }
    if constexpr (READ) {
        // the left column is the border, a gap straight down from the corner: the rows left are one I run, whatever blocks they span,
        // merged into the run at hand and cut at PW_MAX_RUN as every run is.  A round adds to the run or closes a full (or other) one, so
        // left_rows < 2^31 is spent within 2 * 9 rounds
        for (uint32_t round = 0; round < 18 && left_rows; ++round) {
            if (run_op == PW_OP_I && run_len < PW_MAX_RUN) {
                const uint32_t take = min(left_rows, PW_MAX_RUN - run_len);
                run_len += take; left_rows -= take;
            } else {
                if (run_len && pos) { --pos; if (lane == 0) op[pos] = run_len << 4 | run_op; }
                run_op = PW_OP_I; run_len = 0;
            }
        }
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

// RATTLE_ALIGN_READ: an aligned pair whose rectangle has no column (t_end == t_start: the whole read against a gap) is not planned, so
// kernel F never sees it; its CIGAR is one I run of `rows`, written here, in pieces of at most PW_MAX_RUN with the short piece first as
// kernel F leaves them.  The ops the chunk appended behind ops[before] lie in the order of the pairs that went to the device; they are
// merged with the written ones into the order of the chunk's pairs.  Nothing is counted in the kernel stats.
static void cigar_no_column(const cigar_in *in, uint32_t n, cigar_run &R, size_t before) {
    bool any = false;
    for (uint32_t i = 0; i < n && !any; ++i) any = in[i].status == 0 && in[i].rows && !in[i].cols;
    if (!any) return;
    const std::vector<uint32_t> dev(R.ops.begin() + before, R.ops.end());
    R.ops.resize(before);
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (in[i].status == 0 && in[i].rows && !in[i].cols) {
            const uint32_t head = in[i].rows % PW_MAX_RUN, full = in[i].rows / PW_MAX_RUN;
            if (head) R.ops.push_back(head << 4 | PW_OP_I);
            for (uint32_t k = 0; k < full; ++k) R.ops.push_back(PW_MAX_RUN << 4 | PW_OP_I);
            R.count[in[i].read] = full + (head ? 1 : 0);
        } else {
            const size_t cnt = std::min<size_t>(R.count[in[i].read], dev.size() - at);      // (0 for a pair that did not go on)
            R.ops.insert(R.ops.end(), dev.begin() + at, dev.begin() + at + cnt);
            at += cnt;
        }
    }
}

// The pairs `in` of one chunk of kernel E, whose sequences lie in d_q and d_t: the ops of every pair with status 0 appended to R.ops, their
// number to R.count[read].  Sub-chunks as cigar_plan.h plans them; per sub-chunk one launch of kernel F (id 7 of the stats), the counts to
// the host, offsets from them, one gather launch, and the compact ops back.  With `scoring` the form is GAP_AFFINE (id 9): the <true>
// kernel, 32-byte records, two strip words per column; everything around it is the same.  With R.d_pileup (rattle_hip_align_pileup) one
// launch of kernel G (pair_pileup.hip, id 11) follows the gather of every sub-chunk that has an op, and without R.keep_ops the compact
// ops are not copied back; the align_cigars calls set neither and launch, allocate and copy what they always did.
int pair_cigar_chunk(rattle_ctx *ctx, const uint8_t *d_q, const uint8_t *d_t, const cigar_in *in, uint32_t n, uint32_t pair_chunk, cigar_run &R,
                     const rattle_align_scoring *scoring, int mode) {
    const gap_form &F = scoring ? GAP_AFFINE : GAP_LINEAR;
    const size_t ops_before = R.ops.size();
    std::vector<uint8_t> status(n);
    std::vector<uint32_t> rows(n), cols(n);
    for (uint32_t i = 0; i < n; ++i) { status[i] = in[i].status; rows[i] = in[i].rows; cols[i] = in[i].cols; }
    cigar_plan plan;
    plan_cigar(status.data(), rows.data(), cols.data(), n, pair_chunk, R.code_cap, plan, F.rec_bytes, F.strip_words);
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
            alg += (uint64_t)I.rows + I.cols + F.rec_bytes * (blocks * ((uint64_t)I.cols - 1) + I.rows) + 4;
        }
        if (recs > (~0ull >> 8)) { set_error("align_cigars: out of memory (the code records of one pair)"); return RATTLE_ERR_HIP; }
        RT_TRY(R.d_pairs.reserve(m));
        RT_TRY(R.d_codes.reserve(recs * (F.rec_bytes / sizeof(uint4))));
        RT_TRY(R.d_strip.reserve(std::max<uint64_t>(1, strip)));
        RT_TRY(R.d_ops.reserve(words));
        RT_TRY(R.d_count.reserve(m));
        RT_TRY(R.h_count.reserve(m));
        RT_TRY(R.d_off.reserve((size_t)m + 1));
        RT_TRY(R.h_off.reserve((size_t)m + 1));
        RT_HIP(hipMemcpyAsync(R.d_pairs.p, R.h_pairs.p, (size_t)m * sizeof(cigar_pair), hipMemcpyHostToDevice, ctx->stream));
        {
            ktimer kt(ctx, F.k_cigar, alg);
            const auto kernel = mode == RATTLE_ALIGN_READ ? (scoring ? pair_cigar_kernel<true, true> : pair_cigar_kernel<false, true>)
                                                          : (scoring ? pair_cigar_kernel<true, false> : pair_cigar_kernel<false, false>);
            hipLaunchKernelGGL(kernel, dim3((m + 3) / 4), dim3(256), 0, ctx->stream, R.d_pairs.p, m, d_q, d_t, R.d_codes.p, R.d_strip.p, R.d_ops.p,
                               R.d_count.p, scoring ? *scoring : PW_LINEAR);
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
        ctx->stats[F.k_cigar].bytes += 4 * total;                    // ... and 4 bytes per op
        if (!total) continue;
        RT_TRY(R.d_out.reserve(total));
        if (R.keep_ops) RT_TRY(R.h_out.reserve(total));
        RT_HIP(hipMemcpyAsync(R.d_off.p, R.h_off.p, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(cigar_gather_kernel, dim3((m + 3) / 4), dim3(256), 0, ctx->stream, R.d_pairs.p, m, R.d_off.p, R.d_ops.p, R.d_out.p);
        RT_HIP(hipGetLastError());
        if (R.d_pileup) {
            // kernel G (pair_pileup.hip, id 11) behind the gather: per pair the ops and read bases read, the adds made -- one per column
            // with a target base (= cols of a path that ends in the rectangle's corners) and two for starts and ends; the ins adds are
            // counted when the table is back (align_pairs_run).  Every rectangle's columns lie inside a plane, or nothing is launched
            uint64_t g = 4 * total;
            for (uint32_t i = 0; i < m; ++i) {
                const cigar_in &I = in[plan.sub[a + i]];
                if (I.t > R.pileup_n || I.cols > R.pileup_n - I.t) { set_error("align_pileup: a rectangle lies outside the table"); return RATTLE_ERR_HIP; }
                g += (uint64_t)I.rows + 4 * ((uint64_t)I.cols + 2);
            }
            RT_TRY(pair_pileup_launch(ctx, R, m, d_q, g));
        }
        if (R.keep_ops) RT_HIP(hipMemcpyAsync(R.h_out.p, R.d_out.p, total * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
        if (R.keep_ops) R.ops.insert(R.ops.end(), R.h_out.p, R.h_out.p + total);
    }
    if (mode == RATTLE_ALIGN_READ && R.keep_ops) cigar_no_column(in, n, R, ops_before);
    return 0;
}

}  // namespace rattle
