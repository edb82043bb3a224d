// Host orchestration of `rattle correct`, the reference's correct.cpp:311-563, over kernels C and D.
//
// The reference runs a queue of packs through worker threads, two POAs per pack
// (correct.cpp:398-405, 428-436) plus one per multi-pack cluster (:520-532).  Packs are
// independent, so here each POA stage is ONE device pass over all packs, and the post-MSA logic
// (fix_msa_ends :32-92, column vote :94-193, per-read correction :196-309) is kernel D
// (post_msa.hip), one workgroup per pack.  Sequences, qualities, MSA columns and row matrices stay
// in HBM from the upload of the reads to the download of the corrected reads; between stages the
// host only sees lengths (pack widths, corrected read lengths, trim counts) and the pack consensi
// (a few MB), from which it plans the next stage (pack order, length-sorted order for POA #2,
// gather descriptors).
//
// One job over several GPUs: the pack list is the same on every rank (plan_packs); packs
// are LPT-assigned to ranks, both POAs of a pack stay on one GPU, pack consensi are all-gathered (the
// only data-path exchange, a few MB), POA #3 groups are LPT-assigned again.  A rank returns its own
// packs' reads and all consensi; correction_gather reassembles the single-GPU result on the root.
//
// Packs that do not fit the device are skipped and reported, never fatal (rattle_skip_list).
//
// One call is a `correct_job`: the state the steps share, and one member function per step.  correct_driver() at the end
// of the file is the list of stages:
//   plan      packs from ids and lengths (correct.cpp:328-370), this rank's share of them
//   stage 1   POA #1 of every pack (:398-405) + fix ends + correction (:407-409); the corrected reads are compacted on
//             the device and downloaded by a helper thread behind the later stages
//   stage 2   POA #2 over the corrected reads of a pack, stably sorted by length desc (:427-445), + consensus vote
//   stage 3   per-cluster consensus (:489-556): POA #3 over the pack consensi of a cluster with more than one pack
// A POA #3 group is sequential in its number of packs, so the clusters with many packs would leave the device to one
// workgroup each at the end.  When there are enough of them ("big" clusters), their packs go through POA #2 first (stage 2a)
// and their POA #3 (3a) shares a device pass with the POA #2 of all other packs (2b); the remaining small POA #3 groups
// follow (3b).  With several ranks each pass covers this rank's packs / groups and ends with an all-gather of its consensi.
// (Round 4 also ran the big clusters' chain as a second flow on a helper context; round 5 removed it -- byte-identical but
// slower, two stage-1 passes have two tails -- for the row loop of a lone workgroup, poa.hip: dp_rows_mt.)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "common.h"
#include "wire.h"

namespace rattle {

// ---- pure host planning (also behind rattle_hip_plan_packs / rattle_hip_lpt_assign) ---------------------
void lpt_assign(const std::vector<uint64_t> &cost, int nranks, std::vector<uint32_t> &owner) {
    const size_t n = cost.size();
    owner.assign(n, 0);
    if (nranks <= 1 || n == 0) return;
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    std::vector<uint64_t> load((size_t)nranks, 0);
    for (uint32_t i : order) {
        int best = 0;
        for (int r = 1; r < nranks; ++r) if (load[r] < load[best]) best = r;
        owner[i] = (uint32_t)best;
        load[best] += std::max<uint64_t>(cost[i], 1);
    }
}

int plan_packs(const uint64_t *off, uint32_t n_reads, uint32_t n_clusters, const uint32_t *coff, const int32_t *mid, const uint8_t *mrev,
               const rattle_correct_params *P, int nranks, pack_plan &out) {
    const int split = P->split > 0 ? P->split : 200;
    out = pack_plan();
    out.first.assign(1, 0);
    out.cl_p0.assign(n_clusters, 0); out.cl_np.assign(n_clusters, 0);
    for (uint32_t c = 0; c < n_clusters; ++c) {
        const uint32_t a = coff[c], b = coff[c + 1];
        const int n = (int)(b - a);
        out.cl_p0[c] = (uint32_t)out.pk_cid.size();
        if (n <= 0) continue;
        const int n_files = (n - 1) / split + 1;                                  // correct.cpp:331
        for (int nf = 0; nf < n_files; ++nf) {
            const size_t start = out.members.size();
            uint64_t sum = 0, longest = 0;
            for (int j = nf; j < n; j += n_files) {                               // :335 strided sub-packs
                const int32_t rid = mid[a + j];
                if (rid < 0 || (uint32_t)rid >= n_reads) { set_error("cluster member id out of range"); return RATTLE_ERR_ARG; }
                out.members.push_back(sref{rid, (uint8_t)(mrev[a + j] ? 1 : 0)});
                const uint64_t L = off[rid + 1] - off[rid];
                sum += L; longest = std::max(longest, L);
            }
            const bool queued = (int)(out.members.size() - start) > P->min_reads;  // :360 strict
            const bool too_big = queued && P->max_pack_cells && (6 * longest + 64) * longest > P->max_pack_cells;
            if (queued && !too_big) {
                out.pk_cid.push_back((int32_t)c);
                out.pk_local.push_back(out.cl_np[c]);
                out.pk_cost.push_back(longest * sum);
                out.first.push_back((uint32_t)out.members.size());
                ++out.cl_np[c];
            } else {
                for (size_t t = start; t < out.members.size(); ++t) {
                    out.small.push_back(out.members[t]); out.small_cid.push_back((int32_t)c);
                    out.small_why.push_back(too_big ? 1 : 0); out.small_pack.push_back((uint32_t)nf);
                }
                out.members.resize(start);
            }
        }
    }
    lpt_assign(out.pk_cost, nranks, out.pk_owner);
    return 0;
}

namespace {

struct hread {
    std::string seq, qual;
    int32_t rid;
};

inline char comp_base(char c) {                                                  // utils.hpp:8-14
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'T': return 'A';
        case 'G': return 'C';
        case 'U': return 'A';
    }
    return c;
}

// pack member in the orientation the reference aligns it in (correct.cpp:343-346), trimmed by [tf, len - tb)
hread oriented_read(const uint8_t *seq, const uint8_t *qual, const uint64_t *off, sref r, uint32_t tf, uint32_t tb) {
    hread h;
    h.rid = r.rid;
    h.seq.assign((const char *)seq + off[r.rid], (const char *)seq + off[r.rid + 1]);
    h.qual.assign((const char *)qual + off[r.rid], (const char *)qual + off[r.rid + 1]);
    if (r.rev) {
        std::string rc(h.seq.size(), 'A');
        for (size_t t = 0; t < h.seq.size(); ++t) rc[t] = comp_base(h.seq[h.seq.size() - 1 - t]);
        h.seq.swap(rc);
        std::reverse(h.qual.begin(), h.qual.end());
    }
    if (tf || tb) {
        const size_t n = h.seq.size();
        const size_t a = std::min<size_t>(tf, n), b = n - std::min<size_t>(tb, n - a);
        h.seq = h.seq.substr(a, b - a);
        h.qual = h.qual.substr(a, b - a);
    }
    return h;
}

// an array of the result for n entries (never a null pointer: at least one entry)
template <typename T>
T *result_array(size_t n) { return (T *)malloc(std::max<size_t>(1, n) * sizeof(T)); }

void fill_set(rattle_read_set &S, const std::vector<hread> &v, const std::vector<int32_t> &cid, const std::vector<int32_t> &nr) {
    uint64_t tot = 0;
    for (const hread &h : v) tot += h.seq.size();
    alloc_read_set(S, (uint32_t)v.size(), tot);
    tot = 0;
    for (size_t i = 0; i < v.size(); ++i) { S.off[i] = tot; tot += v[i].seq.size(); }
    S.off[v.size()] = tot;
    for (size_t i = 0; i < v.size(); ++i) {
        S.read_id[i] = v[i].rid; S.cluster_id[i] = cid[i]; S.n_reads[i] = nr.empty() ? 0 : nr[i];
        const uint64_t p = S.off[i];
        memcpy(S.seq + p, v[i].seq.data(), v[i].seq.size());
        const size_t ql = std::min(v[i].qual.size(), v[i].seq.size());
        memcpy(S.qual + p, v[i].qual.data(), ql);
        if (ql < v[i].seq.size()) memset(S.qual + p + ql, '!', v[i].seq.size() - ql);
    }
}

// constants of kernel D: phred_symbol thresholds (host libm) and phred_err per quality byte (utils.cpp:10-13)
int ensure_post_constants(rattle_ctx *ctx) {
    if (ctx->phred_ready) return 0;
    build_phred_table(ctx->phred);
    const phred_table &T = ctx->phred;
    double perr[256];
    for (int c = 0; c < 256; ++c) { double q = (char)c - 33; perr[c] = pow(10.0, -q / 10.0); }
    RT_TRY(ctx->d_phred_lo.reserve(T.lo.size())); RT_TRY(ctx->d_perr.reserve(256));
    RT_TRY(ctx->d_exc_bits.reserve(T.exc_bits.size() + 1)); RT_TRY(ctx->d_exc_val.reserve(T.exc_val.size() + 1));
    RT_HIP(hipMemcpy(ctx->d_phred_lo.p, T.lo.data(), T.lo.size() * 8, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(ctx->d_perr.p, perr, sizeof(perr), hipMemcpyHostToDevice));
    if (!T.exc_bits.empty()) {
        RT_HIP(hipMemcpy(ctx->d_exc_bits.p, T.exc_bits.data(), T.exc_bits.size() * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(ctx->d_exc_val.p, T.exc_val.data(), T.exc_val.size() * 4, hipMemcpyHostToDevice));
    }
    ctx->phred_ready = true;
    return 0;
}

// One POA stage + kernel D over device-resident sequences.
struct stage {
    std::vector<uint64_t> off;          // [n+1] host copy of the sequence offsets
    std::vector<uint32_t> first;        // [n_packs+1]
    std::vector<uint32_t> width;        // [n_packs] MSA width (after the POA)
    std::vector<uint8_t> skipped;       // [n_packs] the pack did not fit the device
    std::vector<uint64_t> moff, coff;   // per pack: matrix byte offset / column-array offset
    uint64_t cells = 0, cols = 0;
    dbuf<uint8_t> seq, qual, rowc, rowq, ccons, cflag, csym, cons_out;
    dbuf<uint64_t> d_off, d_moff, d_coff;
    dbuf<uint32_t> col, d_width, d_first, tfront, tback, olen, cons_len;
    dbuf<uint32_t> rep;                 // mode 1 with the correction report on: kernel D's REP_KERNEL counters, counter f of sequence q at rep[f * n() + q]
    dbuf<int32_t> rfirst, rlast;
    dbuf<double> cerr;
    // mode 2 with the consensus support on.  The first n_composed packs are POA #3 packs: h_sup / h_dep are the support and the depth of
    // every base of their sequences (the caller fills them; they lie first in seq), in_sup / in_dep their device copies, msup / mdep the
    // cell matrices.  ccnt / ocnt: kernel D's four values per column / per consensus base, field f at f * cnt_stride
    uint32_t n_composed = 0;
    std::vector<uint32_t> h_sup, h_dep;
    dbuf<uint32_t> in_sup, in_dep, msup, mdep, ccnt, ocnt;
    uint64_t cnt_stride = 0;
    uint32_t n() const { return (uint32_t)off.size() - 1; }
    uint32_t n_packs() const { return (uint32_t)first.size() - 1; }
    void release() {
        seq.release(); qual.release(); rowc.release(); rowq.release(); ccons.release(); cflag.release(); csym.release();
        cons_out.release(); d_off.release(); d_moff.release(); d_coff.release(); col.release(); d_width.release();
        d_first.release(); tfront.release(); tback.release(); olen.release(); cons_len.release(); rfirst.release();
        rlast.release(); cerr.release(); rep.release();
        in_sup.release(); in_dep.release(); msup.release(); mdep.release(); ccnt.release(); ocnt.release();
    }
};

// where a run of gather descriptors reads from
struct gather_part { uint32_t begin, count; const uint8_t *src_seq, *src_qual; };

// The POA arena is cached in the context between stages and sized by what was free when its pass began (85 % of it).  The buffers the
// stages allocate BESIDE it grow with the job: the MSA rows of a stage (two bytes per cell) and the compacted corrected reads (two bytes per
// base, + 25 % of dbuf's slack).  At 5e6 mixed reads (10 Gb) the corrected reads no longer fitted beside a 230 GB arena.  So before a
// large allocation: if it does not fit into what is free, the idle arena goes (the next POA pass allocates one that fits; ~20 ms per GB).
static void make_room(rattle_ctx *ctx, uint64_t bytes) {
    static const bool always = getenv("RATTLE_MAKE_ROOM_ALWAYS") != nullptr;      // (tests: the arena goes at every such point)
    if (!ctx->poa_arena || (!always && bytes < (4ull << 30))) return;             // (a job of the bench's size never asks the driver anything here)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    const uint64_t need = bytes + bytes / 4 + (1ull << 30);
    if (free_b >= need && !always) return;
    (void)hipDeviceSynchronize();
    (void)hipFree(ctx->poa_arena);
    ctx->poa_arena = nullptr; ctx->poa_arena_bytes = 0;
}

// Kernel D over a stage whose sequences (S.seq, S.qual in mode 1, S.d_off), packs (S.first, S.d_first), MSA columns (S.col) and
// widths (S.width, S.d_width) are in place: the layout of the row matrices and per-column arrays, their buffers, the launch.
// The results stay on the device (S.rowc / S.rowq at S.moff, the per-column arrays at S.coff, the per-sequence arrays).
int run_post_msa(rattle_ctx *ctx, stage &S, int mode, const rattle_correct_params *P, const char *order) {
    hipStream_t st = ctx->stream;
    const uint32_t n = S.n(), np = S.n_packs();
    // layout of the row matrices and per-column arrays
    S.moff.assign(np, 0); S.coff.assign(np, 0);
    uint64_t cells = 0, cols = 0;
    for (uint32_t p = 0; p < np; ++p) {
        S.moff[p] = cells; S.coff[p] = cols;
        cells += ((uint64_t)(S.first[p + 1] - S.first[p]) * S.width[p] + 15) & ~(uint64_t)15;
        cols += S.width[p];
    }
    S.cells = cells; S.cols = cols;
    phase_timer T("  stage: post-MSA kernel");
    const bool support = mode == 2 && ctx->consensus_support;
    const uint64_t ccells = !support ? 0 : S.n_composed < np ? S.moff[S.n_composed] : cells;      // cells of the composed packs
    if (support && S.h_sup.size() != (S.n_composed ? S.off[S.first[S.n_composed]] : 0)) { set_error("consensus support: one support and depth per base of the composed packs"); return RATTLE_ERR_ARG; }
    S.cnt_stride = cols + 64;
    make_room(ctx, (mode == 1 ? 2 : 1) * (cells + 64) + 4 * (cols + 64) + 20ull * (n + 1) + (support ? 8 * (ccells + 64) + 32 * S.cnt_stride + 8 * (S.h_sup.size() + 64) : 0));
    RT_TRY(S.rowc.reserve(cells + 64)); RT_TRY(S.d_moff.reserve(np)); RT_TRY(S.d_coff.reserve(np));
    RT_TRY(S.rfirst.reserve(n + 1)); RT_TRY(S.rlast.reserve(n + 1)); RT_TRY(S.ccons.reserve(cols + 64));
    if (mode == 1) {
        RT_TRY(S.rowq.reserve(cells + 64)); RT_TRY(S.tfront.reserve(n + 1)); RT_TRY(S.tback.reserve(n + 1)); RT_TRY(S.olen.reserve(n + 1));
        RT_TRY(S.cflag.reserve(cols + 64)); RT_TRY(S.csym.reserve(cols + 64)); RT_TRY(S.cerr.reserve(cols + 8));
        if (ctx->correction_report) RT_TRY(S.rep.reserve((size_t)REP_KERNEL * n + REP_KERNEL));
    } else {
        RT_TRY(S.cons_out.reserve(cols + 64)); RT_TRY(S.cons_len.reserve(np));
        if (support) {
            RT_TRY(S.ccnt.reserve(4 * S.cnt_stride)); RT_TRY(S.ocnt.reserve(4 * S.cnt_stride));
            RT_TRY(S.msup.reserve(ccells + 64)); RT_TRY(S.mdep.reserve(ccells + 64));
            RT_TRY(S.in_sup.reserve(S.h_sup.size() + 64)); RT_TRY(S.in_dep.reserve(S.h_dep.size() + 64));
            if (!S.h_sup.empty()) {
                RT_HIP(hipMemcpyAsync(S.in_sup.p, S.h_sup.data(), S.h_sup.size() * 4, hipMemcpyHostToDevice, st));
                RT_HIP(hipMemcpyAsync(S.in_dep.p, S.h_dep.data(), S.h_dep.size() * 4, hipMemcpyHostToDevice, st));
            }
        }
    }
    RT_HIP(hipMemcpyAsync(S.d_moff.p, S.moff.data(), (size_t)np * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(S.d_coff.p, S.coff.data(), (size_t)np * 8, hipMemcpyHostToDevice, st));
    RT_TRY(ensure_post_constants(ctx));
    post_args A;
    memset(&A, 0, sizeof(A));
    A.seq = S.seq.p; A.qual = S.qual.p; A.off = S.d_off.p; A.pack_first = S.d_first.p; A.col = S.col.p; A.width = S.d_width.p;
    A.moff = S.d_moff.p; A.coff = S.d_coff.p; A.rowc = S.rowc.p; A.rowq = S.rowq.p; A.rfirst = S.rfirst.p; A.rlast = S.rlast.p;
    A.tfront = S.tfront.p; A.tback = S.tback.p; A.olen = S.olen.p; A.ccons = S.ccons.p; A.cflag = S.cflag.p; A.csym = S.csym.p;
    A.cerr = S.cerr.p; A.cons_out = S.cons_out.p; A.cons_len = S.cons_len.p; A.perr = ctx->d_perr.p; A.phred_lo = ctx->d_phred_lo.p;
    A.exc_bits = ctx->d_exc_bits.p; A.exc_val = ctx->d_exc_val.p; A.phred_n0 = ctx->phred.n0; A.phred_cnt = (int32_t)ctx->phred.lo.size();
    A.n_exc = (uint32_t)ctx->phred.exc_bits.size();
    memcpy(A.order, order, 6);
    A.min_occ = P->min_occ; A.gap_occ = P->gap_occ; A.err_ratio = P->err_ratio;
    A.rep = mode == 1 && ctx->correction_report ? S.rep.p : nullptr; A.rep_stride = n;      // with A.rep the launch takes the report form
    if (support) {                                                                          // with A.ccnt the launch takes the report form
        A.ccnt = S.ccnt.p; A.ocnt = S.ocnt.p; A.cnt_stride = S.cnt_stride; A.n_composed = S.n_composed;
        A.in_sup = S.in_sup.p; A.in_dep = S.in_dep.p; A.msup = S.msup.p; A.mdep = S.mdep.p;
    }
    RT_TRY(launch_post_msa(ctx, A, np, mode));
    return 0;
}

// gather the stage's sequences (descriptors built by the caller, dst offsets = st.off) and run POA + kernel D
int run_stage(rattle_ctx *ctx, stage &S, const std::vector<gather_desc> &desc, const std::vector<gather_part> &parts,
              int mode, const rattle_correct_params *P, const char *order, uint64_t *counters) {
    hipStream_t st = ctx->stream;
    const uint32_t n = S.n(), np = S.n_packs();
    const uint64_t total = S.off[n];
    S.width.assign(np, 0);
    S.skipped.assign(np, 0);
    if (np == 0) return 0;
    dbuf<gather_desc> d_desc;
    make_room(ctx, (uint64_t)(n + 1) * sizeof(gather_desc) + (mode == 1 ? 3 : 2) * (total + 64));
    RT_TRY(d_desc.reserve(n + 1));
    RT_TRY(S.seq.reserve(total + 64)); RT_TRY(S.d_off.reserve(n + 1)); RT_TRY(S.col.reserve(total + 64));
    RT_TRY(S.d_width.reserve(np)); RT_TRY(S.d_first.reserve(np + 1));
    if (mode == 1) RT_TRY(S.qual.reserve(total + 64));
    if (n) RT_HIP(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)n * sizeof(gather_desc), hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(S.d_off.p, S.off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(S.d_first.p, S.first.data(), (size_t)(np + 1) * 4, hipMemcpyHostToDevice, st));
    for (const gather_part &g : parts)
        RT_TRY(launch_gather(ctx, d_desc.p + g.begin, g.count, g.src_seq, mode == 1 ? g.src_qual : nullptr, S.seq.p, mode == 1 ? S.qual.p : nullptr));
    unsigned long long h_cnt[POA_CNT_PUBLIC];
    {
        phase_timer T("  stage: POA");
        // POA #2 / #3 align corrected reads / pack consensi: their graphs are almost chains -- rows that depend on each other
        // (teams of wavefronts gain nothing), and per alignment as much serial work as DP (what pays is many packs per CU)
        ctx->poa_shallow_graphs = mode == 2 && !getenv("RATTLE_NO_SHALLOW_HINT");      // (the switch: A/B of the hint itself)
        struct unhint { rattle_ctx *c; ~unhint() { c->poa_shallow_graphs = 0; } } uh{ctx};
        RT_TRY(poa_device_run(ctx, S.seq.p, S.d_off.p, S.off.data(), n, S.first.data(), np, S.col.p, S.d_width.p, S.width.data(), h_cnt, &S.skipped));
    }
    d_desc.release();
    counters[0] += h_cnt[POA_CNT_CELLS];
    counters[1] += h_cnt[POA_CNT_SEQS];
    counters[5] += h_cnt[POA_CNT_CELLS_DONE]; counters[6] += h_cnt[POA_CNT_BAND_OK]; counters[7] += h_cnt[POA_CNT_BAND_FAIL];      // DP cells computed; alignments with a certified band / a failed certificate
    return run_post_msa(ctx, S, mode, P, order);
}

// Consensus stage (POA #2 of packs, POA #3 of clusters) whose input sequences come from the host: the pack
// consensi are a few MB and, with several ranks, arrive through the exchange.
struct cons_stage {
    stage S;
    std::vector<uint8_t> h_in;                 // concatenated input sequences (host-sourced groups)
    std::vector<uint32_t> len;                 // [n_packs] consensus length
    std::vector<uint8_t> cons;                 // consensi at S.coff
    std::vector<uint32_t> cnt;                 // the consensus support: field f of the base at cons[x] at cnt[f * S.cnt_stride + x]
};

int fetch_consensi(rattle_ctx *ctx, cons_stage &C) {
    const uint32_t np = C.S.n_packs();
    C.len.assign(np + 1, 0);
    C.cons.assign(C.S.cols + 1, 0);
    if (!np) return 0;
    RT_HIP(hipMemcpyAsync(C.len.data(), C.S.cons_len.p, (size_t)np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (C.S.cols) RT_HIP(hipMemcpyAsync(C.cons.data(), C.S.cons_out.p, C.S.cols, hipMemcpyDeviceToHost, ctx->stream));
    if (C.S.ocnt.p && ctx->consensus_support) {
        C.cnt.assign(4 * C.S.cnt_stride, 0);
        RT_HIP(hipMemcpyAsync(C.cnt.data(), C.S.ocnt.p, C.cnt.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

struct skip_t { int32_t cid; uint32_t pack, stage; std::vector<int32_t> rids; };

// One `correct` call: what its steps share, and the steps in the order correct_driver() runs them.
struct correct_job {
    rattle_ctx *const ctx;
    const uint8_t *const seq, *const qual;           // the reads (host)
    const uint64_t *const off;
    const uint32_t n_reads, n_clusters;
    const rattle_correct_params *const P;
    const char *const order;                         // vote slot order
    rattle_correction *const R;
    const int rank, nranks;
    const hipStream_t st;
    uint64_t counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    pack_plan PL;
    uint32_t n_packs = 0, nm = 0;
    std::vector<std::vector<uint32_t>> cl_perm;      // the order a cluster's pack consensi enter POA #3 in (default: pack order)
    std::vector<uint32_t> mine;                      // my packs, in pack order (all of them on one rank); k below is an index in here
    std::vector<uint8_t> big;                        // per cluster: its packs go through stage 2a, its POA #3 through 3a
    bool any_big = false;

    // stage 1: first[k] .. first[k + 1] of S1 are the members of pack mine[k]
    stage S1;
    std::vector<sref> r;                             // my packs' members, pack after pack
    std::vector<uint32_t> olen, tfront, tback;       // per member
    const bool report = ctx->correction_report;      // the correction report is on for this call
    std::vector<uint32_t> rep;                       // ... kernel D's counters, counter f of member q at rep[f * r.size() + q]
    dbuf<uint8_t> d_rseq, d_rqual;                   // the reads in HBM, unless they are staged there already
    const uint8_t *dev_seq = nullptr, *dev_qual = nullptr;
    dbuf<uint8_t> d_os, d_oq;                        // corrected reads, compacted on the device
    std::thread d2h;                                 // ... and their download
    hipError_t d2h_err = hipSuccess;
    std::vector<uint32_t> cor_pack;

    std::vector<uint8_t> pk_dead;                    // stage at which a pack was given up (this rank's packs: exact; others: from the exchange)
    std::vector<std::string> pk_cons, cl_cons;       // pack consensus (POA #2) / cluster consensus, filled by the exchanges
    std::vector<uint8_t> pk_has, cl_has;
    const bool support = ctx->consensus_support;     // the consensus support is on for this call (one rank: abi.hip refuses it on several)
    std::vector<std::vector<uint32_t>> pk_sup, pk_dep;      // ... per base of pk_cons: winner's count / rows that voted in POA #2's MSA (reads)
    std::vector<std::vector<uint32_t>> cl_sup[SUP_FIELDS];  // ... per base of cl_cons
    std::vector<uint8_t> cl_level;
    std::vector<skip_t> skips;                       // skip list (this rank's share; unqueued entries on rank 0)
    std::vector<hread> uncorrected;
    std::vector<int32_t> unc_cid;
    std::vector<uint32_t> unc_pack;

    // Several ranks: the plan depends on the arguments alone (the same on every rank).  After it a rank works on its own packs,
    // and a failure of its own (a bad base in one of ITS reads, a HIP error, an allocation) must not leave the other ranks
    // blocked in the next all-gather: the rank remembers the error, keeps joining the exchanges with a failure record, and
    // every rank returns an error after the exchange that carried it.
    int local_rc = 0;
    std::string local_msg;

    ~correct_job() { if (d2h.joinable()) d2h.join(); }      // on every way out, before d_os / d_oq go

    // the result of a step of this rank's own work: a single rank returns its error at once, one of several remembers its first
    int own_error(int rc) {
        if (rc == 0 || nranks == 1) return rc;
        if (local_rc == 0) { local_rc = rc; local_msg = rattle_hip_last_error(); }
        return 0;
    }

    int set_pack_orders() {
        cl_perm.resize(P->n_pack_orders ? n_clusters : 0);
        for (uint32_t i = 0; i < P->n_pack_orders; ++i) {
            if (!P->pack_order_cluster || !P->pack_order_offsets || !P->pack_order_perm) { set_error("pack order arrays missing"); return RATTLE_ERR_ARG; }
            const uint32_t c = P->pack_order_cluster[i];
            if (c >= n_clusters) { set_error("pack order: cluster out of range"); return RATTLE_ERR_ARG; }
            const uint32_t a = P->pack_order_offsets[i], b = P->pack_order_offsets[i + 1];
            std::vector<uint32_t> perm(P->pack_order_perm + a, P->pack_order_perm + b), chk(perm);
            std::sort(chk.begin(), chk.end());
            bool ok = b - a == PL.cl_np[c];
            for (uint32_t t = 0; ok && t < chk.size(); ++t) ok = chk[t] == t;
            if (!ok) { set_error("pack order of cluster " + std::to_string(c) + " is not a permutation of its " + std::to_string(PL.cl_np[c]) + " packs"); return RATTLE_ERR_ARG; }
            cl_perm[c] = perm;
        }
        return 0;
    }

    // ---- correct.cpp:328-370 pack building: ids and strands only, the bases stay where they are; then this rank's share
    int plan(const uint32_t *coff, const int32_t *mid, const uint8_t *mrev) {
        RT_TRY(plan_packs(off, n_reads, n_clusters, coff, mid, mrev, P, nranks, PL));
        n_packs = (uint32_t)PL.pk_cid.size();
        counters[2] = n_packs;
        RT_TRY(set_pack_orders());
        pk_dead.assign(n_packs, 0); pk_cons.resize(n_packs); pk_has.assign(n_packs, 0);
        cl_cons.resize(n_clusters); cl_has.assign(n_clusters, 0);
        if (support) {
            pk_sup.resize(n_packs); pk_dep.resize(n_packs); cl_level.assign(n_clusters, 0);
            for (auto &v : cl_sup) v.resize(n_clusters);
        }
        S1.first.assign(1, 0);
        for (uint32_t p = 0; p < n_packs; ++p) {
            if ((int)PL.pk_owner[p] != rank) continue;
            mine.push_back(p);
            r.insert(r.end(), PL.members.begin() + PL.first[p], PL.members.begin() + PL.first[p + 1]);
            S1.first.push_back((uint32_t)r.size());
        }
        nm = (uint32_t)mine.size();
        // (RATTLE_BIG_CLUSTER_PACKS / RATTLE_BIG_MIN_PACKS override the two thresholds: tests force the split on small inputs)
        const uint32_t BIG = std::max(2, getenv("RATTLE_BIG_CLUSTER_PACKS") ? atoi(getenv("RATTLE_BIG_CLUSTER_PACKS")) : 48);
        const uint64_t big_min = getenv("RATTLE_BIG_MIN_PACKS") ? (uint64_t)atoll(getenv("RATTLE_BIG_MIN_PACKS")) : 1024;
        big.assign(n_clusters, 0);
        uint64_t big_packs = 0;
        for (uint32_t c = 0; c < n_clusters; ++c) if (PL.cl_np[c] >= BIG) big_packs += PL.cl_np[c];
        if (big_packs >= big_min) for (uint32_t c = 0; c < n_clusters; ++c) { big[c] = PL.cl_np[c] >= BIG; any_big |= big[c] != 0; }
        return 0;
    }

    // only A, C, G, T, U are defined for the vote (an unordered_map key set in the reference)
    int check_bases() {
        bool ok[256] = {false};
        ok['A'] = ok['C'] = ok['G'] = ok['T'] = ok['U'] = true;
        std::atomic<int> bad(0);
        const size_t chunk = 4096, n1 = r.size();
        parallel_for((n1 + chunk - 1) / chunk, P->n_threads, [&](size_t c) {
            for (size_t q = c * chunk; q < std::min<size_t>(n1, (c + 1) * chunk); ++q)
                for (uint64_t b = off[r[q].rid]; b < off[r[q].rid + 1]; ++b)
                    if (!ok[seq[b]]) { bad = 1; return; }
        });
        if (bad) { set_error("correct: read contains a base other than A, C, G, T, U"); return RATTLE_ERR_ARG; }
        return 0;
    }

    // members of packs that are never queued: uncorrected as they are (rank 0), those of the max_pack_cells rule reported
    void unqueued_reads() {
        if (rank != 0) return;
        for (size_t i = 0; i < PL.small.size(); ++i) {
            uncorrected.push_back(oriented_read(seq, qual, off, PL.small[i], 0, 0));
            unc_cid.push_back(PL.small_cid[i]); unc_pack.push_back(0xFFFFFFFFu);
            if (PL.small_why[i]) {
                if (skips.empty() || skips.back().stage != 0 || skips.back().cid != PL.small_cid[i] || skips.back().pack != PL.small_pack[i])
                    skips.push_back(skip_t{PL.small_cid[i], PL.small_pack[i], 0u, {}});
                skips.back().rids.push_back(PL.small[i].rid);
            }
        }
    }

    // ---- reads -> HBM once
    int upload_reads() {
        const uint64_t total_in = off[n_reads];
        if (ctx->staged_seq_key == seq && ctx->staged_qual_key == qual && ctx->staged_n == n_reads && ctx->staged_total == total_in && off[0] == 0) {
            dev_seq = ctx->d_staged_seq.p; dev_qual = ctx->d_staged_qual.p;       // resident (rattle_hip_stage_reads)
        } else {
            phase_timer T("correct: upload");
            RT_TRY(d_rseq.reserve(total_in + 64)); RT_TRY(d_rqual.reserve(total_in + 64));
            RT_HIP(hipMemcpyAsync(d_rseq.p, seq, total_in, hipMemcpyHostToDevice, st));
            RT_HIP(hipMemcpyAsync(d_rqual.p, qual, total_in, hipMemcpyHostToDevice, st));
            dev_seq = d_rseq.p; dev_qual = d_rqual.p;
        }
        return 0;
    }

    // ---- stage 1: oriented pack members gathered (:343-346), POA #1 (correct.cpp:398-405) + fix ends + correction (:407-409);
    // lengths back to the host
    int stage1() {
        const uint32_t n1 = (uint32_t)r.size();
        olen.assign(n1 + 1, 0); tfront.assign(n1 + 1, 0); tback.assign(n1 + 1, 0);
        std::vector<gather_desc> desc(n1);
        S1.off.assign(n1 + 1, 0);
        for (uint32_t q = 0; q < n1; ++q) {
            const uint32_t len = (uint32_t)(off[r[q].rid + 1] - off[r[q].rid]);
            desc[q] = gather_desc{off[r[q].rid], S1.off[q], len, r[q].rev};
            S1.off[q + 1] = S1.off[q] + len;
        }
        phase_timer T("correct: stage 1", &ctx->stage_ms[1]);
        RT_TRY(run_stage(ctx, S1, desc, {gather_part{0, n1, dev_seq, dev_qual}}, 1, P, order, counters));
        RT_HIP(hipMemcpyAsync(olen.data(), S1.olen.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, st));
        RT_HIP(hipMemcpyAsync(tfront.data(), S1.tfront.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, st));
        RT_HIP(hipMemcpyAsync(tback.data(), S1.tback.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, st));
        if (report) {
            rep.assign((size_t)REP_KERNEL * n1 + 1, 0);
            if (n1) RT_HIP(hipMemcpyAsync(rep.data(), S1.rep.p, (size_t)REP_KERNEL * n1 * 4, hipMemcpyDeviceToHost, st));
        }
        RT_HIP(hipStreamSynchronize(st));
        S1.seq.release(); S1.qual.release(); S1.col.release();
        for (uint32_t k = 0; k < nm; ++k)
            if (S1.skipped[k]) {                      // POA #1 did not fit: the pack's reads stay as they are
                pk_dead[mine[k]] = 1;
                for (uint32_t q = S1.first[k]; q < S1.first[k + 1]; ++q) { olen[q] = 0; tfront[q] = 0; tback[q] = 0; }
            }
        return 0;
    }

    // where member q of my pack k lies in the stage-1 row matrix: kernel D left the corrected read at the start of its row
    uint64_t row_of(uint32_t k, uint32_t q) const { return S1.moff[k] + (uint64_t)(q - S1.first[k]) * S1.width[k]; }

    // ---- after stage 1: skip entries, corrected reads in pack order (:413-425) compacted on the device and downloaded
    // behind the later stages, reads whose corrected sequence came out empty
    int stage1_finish() {
        for (uint32_t k = 0; k < nm; ++k) {
            if (!S1.skipped[k]) continue;
            skips.push_back(skip_t{PL.pk_cid[mine[k]], PL.pk_local[mine[k]], 1u, {}});
            for (uint32_t q = S1.first[k]; q < S1.first[k + 1]; ++q) skips.back().rids.push_back(r[q].rid);
        }
        {
            phase_timer T("correct: corrected reads D2H");
            std::vector<gather_desc> od;
            std::vector<int32_t> o_rid, o_cid;
            std::vector<uint32_t> o_q;
            uint64_t tot = 0;
            for (uint32_t k = 0; k < nm; ++k)
                for (uint32_t q = S1.first[k]; q < S1.first[k + 1]; ++q) {
                    if (olen[q] == 0) continue;
                    od.push_back(gather_desc{row_of(k, q), tot, olen[q], 0u});
                    o_rid.push_back(r[q].rid); o_cid.push_back(PL.pk_cid[mine[k]]);
                    o_q.push_back(q);
                    cor_pack.push_back(mine[k]);
                    tot += olen[q];
                }
            rattle_read_set &C = R->corrected;
            const size_t nc = od.size();
            alloc_read_set(C, (uint32_t)nc, tot);
            for (size_t i = 0; i < nc; ++i) { C.off[i] = od[i].dst; C.read_id[i] = o_rid[i]; C.cluster_id[i] = o_cid[i]; C.n_reads[i] = 0; }
            C.off[nc] = tot;
            if (report) {                            // the report of record i: the lengths, the trim counts and kernel D's counters of its member
                correction_box *B = box_of(R);
                alloc_report(B, nc);
                const size_t n1 = r.size();
                for (size_t i = 0; i < nc; ++i) {
                    const uint32_t q = o_q[i];
                    B->rep[REP_IN][i] = (uint32_t)(off[r[q].rid + 1] - off[r[q].rid]); B->rep[REP_OUT][i] = olen[q];
                    B->rep[REP_TFRONT][i] = tfront[q]; B->rep[REP_TBACK][i] = tback[q];
                    for (int f = 0; f < REP_KERNEL; ++f) B->rep[REP_MATCH + f][i] = rep[f * n1 + q];
                }
            }
            if (nc) {
                make_room(ctx, 2 * (tot + 64) + nc * sizeof(gather_desc));
                RT_TRY(d_os.reserve(tot + 64)); RT_TRY(d_oq.reserve(tot + 64));
                dbuf<gather_desc> d_od;
                RT_TRY(d_od.reserve(nc));
                RT_HIP(hipMemcpyAsync(d_od.p, od.data(), nc * sizeof(gather_desc), hipMemcpyHostToDevice, st));
                RT_TRY(launch_gather(ctx, d_od.p, (uint32_t)nc, S1.rowc.p, S1.rowq.p, d_os.p, d_oq.p));
                RT_HIP(hipStreamSynchronize(st));
                d_od.release();
                // the download (2 GB at 1e6 reads, pageable destination) runs on a helper thread and the
                // copy engine while the following POA stages compute
                // (nothing it reads -- the set, d_os / d_oq, cor_pack -- changes before it is joined)
                d2h = std::thread([this, tot]() {
                    const rattle_read_set &C = R->corrected;
                    hipError_t e = hipSetDevice(ctx->device);
                    if (e == hipSuccess) e = hipMemcpy(C.seq, d_os.p, tot, hipMemcpyDeviceToHost);
                    if (e == hipSuccess) e = hipMemcpy(C.qual, d_oq.p, tot, hipMemcpyDeviceToHost);
                    d2h_err = e;
                    // the corrected reads are final from here on: the caller may start writing them out while POA #2 / #3 run
                    if (e == hipSuccess && P->corrected_ready) P->corrected_ready(P->corrected_ready_user, &C, cor_pack.data());
                });
            }
        }
        // reads whose corrected sequence came out empty: uncorrected, as fix_msa_ends left them (:289-293)
        for (uint32_t k = 0; k < nm; ++k)
            for (uint32_t q = S1.first[k]; q < S1.first[k + 1]; ++q)
                if (olen[q] == 0) {
                    uncorrected.push_back(oriented_read(seq, qual, off, r[q], tfront[q], tback[q]));
                    unc_cid.push_back(PL.pk_cid[mine[k]]); unc_pack.push_back(mine[k]);
                }
        return 0;
    }

    // the download is over (the stage-1 rows are no longer needed once it is)
    int join_download() {
        if (d2h.joinable()) d2h.join();
        if (d2h_err == hipSuccess) return 0;
        set_error(std::string("corrected reads download: ") + hipGetErrorString(d2h_err));
        return RATTLE_ERR_HIP;
    }

    // the live packs of a cluster in the order their consensi enter POA #3
    void group_of(uint32_t c, std::vector<uint32_t> &g) const {
        g.clear();
        for (uint32_t t = 0; t < PL.cl_np[c]; ++t) {
            const uint32_t p = PL.cl_p0[c] + (cl_perm.empty() || cl_perm[c].empty() ? t : cl_perm[c][t]);
            if (pk_has[p]) g.push_back(p);
        }
    }

    // The POA #3 groups of the big (or of the other) clusters that fall to this rank, once their pack consensi are in: a
    // group is sequential in its g packs, cost g^2 x length, LPT over ranks.  A cluster with one live pack takes that pack's
    // consensus as it is.  n_all: the groups of all ranks.
    std::vector<uint32_t> poa3_groups(bool of_big, size_t *n_all = nullptr) {
        std::vector<uint32_t> all, own, g, my;
        std::vector<uint64_t> cost;
        for (uint32_t c = 0; c < n_clusters; ++c) {
            if ((big[c] != 0) != of_big || PL.cl_np[c] == 0) continue;
            group_of(c, g);
            if (g.size() > 1) { all.push_back(c); cost.push_back((uint64_t)g.size() * g.size() * pk_cons[g[0]].size()); }
            else if (g.size() == 1) {
                cl_cons[c] = pk_cons[g[0]]; cl_has[c] = 1;
                if (support) {                       // ... and its support with it: rows of POA #2's MSA are reads
                    cl_sup[SUP_SUPPORT][c] = cl_sup[SUP_PACK_SUPPORT][c] = pk_sup[g[0]];
                    cl_sup[SUP_DEPTH][c] = cl_sup[SUP_PACK_DEPTH][c] = pk_dep[g[0]];
                    cl_level[c] = 2;
                }
            }
        }
        lpt_assign(cost, nranks, own);
        for (size_t i = 0; i < all.size(); ++i) if ((int)own[i] == rank) my.push_back(all[i]);
        if (n_all) *n_all = all.size();
        return my;
    }

    // exchange the results of one stage: pack consensi (kind 0) and cluster consensi (kind 1), dead flags included; a rank
    // that has failed sends the failure record instead, and every rank returns an error
    int exchange_stage(std::vector<uint8_t> &mine_bytes) {
        std::vector<std::vector<uint8_t>> all;
        if (nranks > 1) {
            if (local_rc) { mine_bytes.clear(); write_stage_failure(mine_bytes); }
            RT_TRY(xchg_allgatherv(ctx, mine_bytes, all));
            if (local_rc) { set_error(local_msg); return local_rc; }
            for (int rk = 0; rk < nranks; ++rk)
                if (is_stage_failure(all[rk].data(), all[rk].size())) { set_error("correct_reads failed on rank " + std::to_string(rk)); return RATTLE_ERR_HIP; }
        } else if (xchg_recording(ctx)) RT_TRY(xchg_allgatherv(ctx, mine_bytes, all));      // (measurement aid, common.h)
        else { all.resize(1); all[0].swap(mine_bytes); }
        for (size_t rk = 0; rk < all.size(); ++rk) {
            wire_reader W(all[rk].data(), all[rk].size());
            stage_rec rec;
            while (next_stage_rec(W, n_packs, n_clusters, rec)) {
                if (rec.kind() == 0) { if (rec.dead()) pk_dead[rec.id] = (uint8_t)rec.dead(); else { pk_cons[rec.id].assign(rec.s, rec.len); pk_has[rec.id] = 1; } }
                else if (!rec.dead()) { cl_cons[rec.id].assign(rec.s, rec.len); cl_has[rec.id] = 1; }
            }
            if (!W.ok()) { set_error(wire_error("correct stage exchange", (int)rk, W)); return RATTLE_ERR_HIP; }
        }
        return 0;
    }

    // POA #3 over a list of clusters (groups of pack consensi, from the host) + POA #2 over a list of my packs (indices in `mine`;
    // their corrected reads, from the stage-1 rows) in one device pass, timed into stage_ms[ms_slot]; results into `bytes`,
    // skipped groups and packs onto the skip list -- in the order the sequential flow meets them: 2a, then 3a before 2b, then 3b
    int cons_pass(const char *name, int ms_slot, const std::vector<uint32_t> &slots2, const std::vector<uint32_t> &clusters3, std::vector<uint8_t> &bytes) {
        if (slots2.empty() && clusters3.empty()) return 0;
        phase_timer T(name, &ctx->stage_ms[ms_slot]);
        cons_stage C;
        stage &S = C.S;
        std::vector<gather_desc> d;
        S.first.assign(1, 0); S.off.assign(1, 0);
        std::vector<uint32_t> g, rows;
        for (uint32_t c : clusters3) {
            group_of(c, g);
            for (uint32_t p : g) {
                d.push_back(gather_desc{(uint64_t)C.h_in.size(), S.off.back(), (uint32_t)pk_cons[p].size(), 0u});
                C.h_in.insert(C.h_in.end(), pk_cons[p].begin(), pk_cons[p].end());
                if (support) { S.h_sup.insert(S.h_sup.end(), pk_sup[p].begin(), pk_sup[p].end()); S.h_dep.insert(S.h_dep.end(), pk_dep[p].begin(), pk_dep[p].end()); }
                S.off.push_back(S.off.back() + pk_cons[p].size());
            }
            S.first.push_back((uint32_t)S.off.size() - 1);
        }
        const uint32_t n3 = (uint32_t)d.size();
        S.n_composed = (uint32_t)clusters3.size();
        for (uint32_t k : slots2) {                  // my pack k's corrected reads, length-sorted
            rows.clear();
            for (uint32_t q = S1.first[k]; q < S1.first[k + 1]; ++q) if (olen[q]) rows.push_back(q);
            std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return olen[a] > olen[b]; });
            for (uint32_t q : rows) {
                d.push_back(gather_desc{row_of(k, q), S.off.back(), olen[q], 0u});
                S.off.push_back(S.off.back() + olen[q]);
            }
            S.first.push_back((uint32_t)S.off.size() - 1);
        }
        dbuf<uint8_t> d_in;
        make_room(ctx, C.h_in.size() + 64);
        RT_TRY(d_in.reserve(C.h_in.size() + 64));
        if (!C.h_in.empty()) RT_HIP(hipMemcpyAsync(d_in.p, C.h_in.data(), C.h_in.size(), hipMemcpyHostToDevice, st));
        RT_TRY(run_stage(ctx, S, d, {gather_part{0, n3, d_in.p, nullptr}, gather_part{n3, (uint32_t)d.size() - n3, slots2.empty() ? nullptr : S1.rowc.p, nullptr}},
                         2, P, order, counters));
        RT_TRY(fetch_consensi(ctx, C));
        uint32_t slot = 0;
        auto counts = [&](uint32_t sl, int f) {      // field f of the consensus of slot sl
            const uint32_t *b = C.cnt.data() + (size_t)f * S.cnt_stride + S.coff[sl];
            return std::vector<uint32_t>(b, b + C.len[sl]);
        };
        for (uint32_t c : clusters3) {
            if (S.skipped[slot]) {
                skips.push_back(skip_t{(int32_t)c, 0u, 3u, {}});
                write_stage_rec(bytes, c, 1u | (3u << 1), nullptr, 0);
            } else {
                write_stage_rec(bytes, c, 1u, (const char *)C.cons.data() + S.coff[slot], C.len[slot]);
                if (support) { for (int f = 0; f < SUP_FIELDS; ++f) cl_sup[f][c] = counts(slot, f); cl_level[c] = 3; }
            }
            ++slot;
        }
        for (uint32_t k : slots2) {
            const uint32_t p = mine[k];
            if (S.skipped[slot]) {
                skips.push_back(skip_t{PL.pk_cid[p], PL.pk_local[p], 2u, {}});
                for (uint32_t q = S1.first[k]; q < S1.first[k + 1]; ++q) skips.back().rids.push_back(r[q].rid);
                write_stage_rec(bytes, p, 2u << 1, nullptr, 0);
            } else {
                write_stage_rec(bytes, p, 0u, (const char *)C.cons.data() + S.coff[slot], C.len[slot]);
                if (support) { pk_sup[p] = counts(slot, SUP_SUPPORT); pk_dep[p] = counts(slot, SUP_DEPTH); }
            }
            ++slot;
        }
        return 0;
    }

    // ---- the three read sets, the pack of every read, the skip list, the counters
    void assemble() {
        if (!nm) fill_set(R->corrected, {}, {}, {});      // (else: stage1_finish)
        if (report && !box_of(R)->has_report) alloc_report(box_of(R), 0);
        std::vector<hread> consensi;
        std::vector<int32_t> con_cid, con_n;
        for (uint32_t c = 0; c < n_clusters; ++c) {
            if (!cl_has[c]) continue;
            int total = 0;
            for (uint32_t p = PL.cl_p0[c]; p < PL.cl_p0[c] + PL.cl_np[c]; ++p) if (pk_has[p]) total += (int)(PL.first[p + 1] - PL.first[p]);
            const std::string &s = cl_cons[c];
            consensi.push_back(hread{s, std::string(s.size(), 'K'), -1});
            con_cid.push_back((int32_t)c);
            con_n.push_back(total);
        }
        fill_set(R->uncorrected, uncorrected, unc_cid, {});
        fill_set(R->consensi, consensi, con_cid, con_n);
        if (support) {                               // per base of the consensi, in their order
            correction_box *B = box_of(R);
            const rattle_read_set &S = R->consensi;
            alloc_support(B, S.n, S.off[S.n]);
            for (uint32_t i = 0; i < S.n; ++i) {
                const uint32_t c = (uint32_t)con_cid[i];
                B->sup_level[i] = cl_level[c];
                for (int f = 0; f < SUP_FIELDS; ++f)
                    if (S.off[i + 1] > S.off[i]) memcpy(B->sup[f] + S.off[i], cl_sup[f][c].data(), (S.off[i + 1] - S.off[i]) * 4);
            }
        }
        R->corrected_pack = result_array<uint32_t>(cor_pack.size());
        if (!cor_pack.empty()) memcpy(R->corrected_pack, cor_pack.data(), cor_pack.size() * 4);
        R->uncorrected_pack = result_array<uint32_t>(unc_pack.size());
        if (!unc_pack.empty()) memcpy(R->uncorrected_pack, unc_pack.data(), unc_pack.size() * 4);
        rattle_skip_list &K = R->skipped;
        const size_t n = skips.size();
        K.n = (uint32_t)n;
        K.cluster_id = result_array<int32_t>(n); K.pack = result_array<uint32_t>(n); K.stage = result_array<uint32_t>(n);
        K.read_off = (uint64_t *)malloc((n + 1) * 8);
        uint64_t tot = 0;
        for (size_t i = 0; i < n; ++i) { K.cluster_id[i] = skips[i].cid; K.pack[i] = skips[i].pack; K.stage[i] = skips[i].stage; K.read_off[i] = tot; tot += skips[i].rids.size(); }
        K.read_off[n] = tot;
        K.read_id = result_array<int32_t>(tot);
        for (size_t i = 0; i < n; ++i) if (!skips[i].rids.empty()) memcpy(K.read_id + K.read_off[i], skips[i].rids.data(), skips[i].rids.size() * 4);
        counters[3] = n;
        counters[4] = tot;
        memcpy(R->counters, counters, sizeof(counters));
    }
};

// the vote slot order of a call: the caller's, or the reference's
int vote_order_of(const rattle_correct_params *P, char order[8]) {
    memset(order, 0, 8);
    memcpy(order, P->vote_order[0] ? P->vote_order : "U-GTCA", 6);
    for (int i = 0; i < 6; ++i)
        if (!order[i] || !strchr("ACGTU-", order[i])) { set_error("vote_order must be a permutation of ACGTU-"); return RATTLE_ERR_ARG; }
    return 0;
}

}  // namespace

// Test hook: kernel D alone on a given MSA (sequences + the column of every base, as kernel C leaves them), through the
// stage and the launch path of the driver (run_post_msa), and everything it wrote.  The input was validated by the caller
// (abi.hip): columns strictly increasing and below the width in every pack of width > 0, bases in ACGTU.
static int debug_stage_upload(rattle_ctx *ctx, stage &S, int mode, const rattle_debug_msa *in) {
    hipStream_t st = ctx->stream;
    const uint32_t np = in->n_packs, n = in->pack_first[np];
    S.first.assign(in->pack_first, in->pack_first + np + 1);
    S.off.assign(in->off, in->off + n + 1);
    S.width.assign(in->width, in->width + np);
    S.skipped.assign(np, 0);
    const uint64_t total = S.off[n];
    RT_TRY(S.seq.reserve(total + 64)); RT_TRY(S.d_off.reserve(n + 1)); RT_TRY(S.col.reserve(total + 64));
    RT_TRY(S.d_width.reserve(np + 1)); RT_TRY(S.d_first.reserve(np + 1));
    if (mode == 1) RT_TRY(S.qual.reserve(total + 64));
    if (total) {
        RT_HIP(hipMemcpyAsync(S.seq.p, in->seq, total, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(S.col.p, in->col, total * 4, hipMemcpyHostToDevice, st));
        if (mode == 1) RT_HIP(hipMemcpyAsync(S.qual.p, in->qual, total, hipMemcpyHostToDevice, st));
    }
    RT_HIP(hipMemcpyAsync(S.d_off.p, S.off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(S.d_first.p, S.first.data(), (size_t)(np + 1) * 4, hipMemcpyHostToDevice, st));
    if (np) RT_HIP(hipMemcpyAsync(S.d_width.p, S.width.data(), (size_t)np * 4, hipMemcpyHostToDevice, st));
    return 0;
}

int debug_post_msa(rattle_ctx *ctx, const rattle_correct_params *P, int mode, const rattle_debug_msa *in, rattle_debug_post **out) {
    char order[8];
    RT_TRY(vote_order_of(P, order));
    hipStream_t st = ctx->stream;
    const uint32_t np = in->n_packs, n = in->pack_first[np];
    stage S;
    RT_TRY(debug_stage_upload(ctx, S, mode, in));
    RT_TRY(run_post_msa(ctx, S, mode, P, order));

    rattle_debug_post *D = (rattle_debug_post *)calloc(1, sizeof(rattle_debug_post));
    *out = D;
    D->n_packs = np; D->n_rows = n; D->n_cols = S.cols; D->mode = mode;
    D->moff = result_array<uint64_t>(np); D->coff = result_array<uint64_t>(np);
    if (np) { memcpy(D->moff, S.moff.data(), (size_t)np * 8); memcpy(D->coff, S.coff.data(), (size_t)np * 8); }
    D->rfirst = result_array<int32_t>(n); D->rlast = result_array<int32_t>(n);
    D->cons = result_array<uint8_t>(S.cols);
    std::vector<uint8_t> rowc, rowq;
    auto fetch = [st](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    if (np) {
        RT_HIP(fetch(D->rfirst, S.rfirst.p, (size_t)n * 4)); RT_HIP(fetch(D->rlast, S.rlast.p, (size_t)n * 4));
        RT_HIP(fetch(D->cons, S.ccons.p, S.cols));
    }
    if (mode == 1) {
        D->tfront = result_array<uint32_t>(n); D->tback = result_array<uint32_t>(n); D->olen = result_array<uint32_t>(n);
        D->flag = result_array<uint8_t>(S.cols); D->sym = result_array<uint8_t>(S.cols); D->err = result_array<double>(S.cols);
        rowc.resize(S.cells + 1); rowq.resize(S.cells + 1);
        if (np) {
            RT_HIP(fetch(D->tfront, S.tfront.p, (size_t)n * 4)); RT_HIP(fetch(D->tback, S.tback.p, (size_t)n * 4));
            RT_HIP(fetch(D->olen, S.olen.p, (size_t)n * 4));
            RT_HIP(fetch(D->flag, S.cflag.p, S.cols)); RT_HIP(fetch(D->sym, S.csym.p, S.cols)); RT_HIP(fetch(D->err, S.cerr.p, S.cols * 8));
            RT_HIP(fetch(rowc.data(), S.rowc.p, S.cells)); RT_HIP(fetch(rowq.data(), S.rowq.p, S.cells));
        }
        if (ctx->correction_report) {
            uint32_t **dst[REP_KERNEL] = {&D->match, &D->substituted, &D->mismatch_kept, &D->inserted, &D->deleted, &D->gap_kept};
            for (int f = 0; f < REP_KERNEL; ++f) {
                *dst[f] = result_array<uint32_t>(n);
                if (np) RT_HIP(fetch(*dst[f], S.rep.p + (size_t)f * n, (size_t)n * 4));
            }
        }
    } else {
        D->cons_len = result_array<uint32_t>(np); D->consensus = result_array<uint8_t>(S.cols);
        if (np) { RT_HIP(fetch(D->cons_len, S.cons_len.p, (size_t)np * 4)); RT_HIP(fetch(D->consensus, S.cons_out.p, S.cols)); }
    }
    RT_HIP(hipStreamSynchronize(st));
    // a pack of width 0 (or without rows) leaves the kernel before the windows are written: reported as the empty window
    for (uint32_t p = 0; p < np; ++p)
        if (S.width[p] == 0) for (uint32_t q = S.first[p]; q < S.first[p + 1]; ++q) { D->rfirst[q] = 0; D->rlast[q] = -1; }
    if (mode == 1) {
        // the corrected read lies at the start of its row, as stage1_finish gathers it (row_of)
        D->out_off = (uint64_t *)malloc(((size_t)n + 1) * 8);
        uint64_t tot = 0;
        for (uint32_t q = 0; q < n; ++q) { D->out_off[q] = tot; tot += D->olen[q]; }
        D->out_off[n] = tot;
        D->out_seq = result_array<uint8_t>(tot); D->out_qual = result_array<uint8_t>(tot);
        for (uint32_t p = 0; p < np; ++p)
            for (uint32_t q = S.first[p]; q < S.first[p + 1]; ++q) {
                if (D->olen[q] > S.width[p]) { set_error("debug_post_msa: a corrected read is longer than its row"); return RATTLE_ERR_HIP; }
                const uint64_t at = S.moff[p] + (uint64_t)(q - S.first[p]) * S.width[p];
                memcpy(D->out_seq + D->out_off[q], rowc.data() + at, D->olen[q]);
                memcpy(D->out_qual + D->out_off[q], rowq.data() + at, D->olen[q]);
            }
    }
    return 0;
}

// Test hook: the mode-2 report form of kernel D alone on given MSAs (validated by the caller like debug_post_msa's), through
// run_post_msa and fetch_consensi.  With in->sup / in->dep every pack is a composed (POA #3) pack.
int debug_consensus_support(rattle_ctx *ctx, const rattle_correct_params *P, const rattle_debug_support_msa *in, rattle_debug_support **out) {
    char order[8];
    RT_TRY(vote_order_of(P, order));
    const uint32_t np = in->n_packs, n = in->pack_first[np];
    const rattle_debug_msa M = {np, in->pack_first, in->width, in->off, in->seq, nullptr, in->col};
    cons_stage C;
    stage &S = C.S;
    RT_TRY(debug_stage_upload(ctx, S, 2, &M));
    if (in->sup && ctx->consensus_support) {
        S.n_composed = np;
        S.h_sup.assign(in->sup, in->sup + S.off[n]); S.h_dep.assign(in->dep, in->dep + S.off[n]);
    }
    RT_TRY(run_post_msa(ctx, S, 2, P, order));
    RT_TRY(fetch_consensi(ctx, C));
    rattle_debug_support *D = (rattle_debug_support *)calloc(1, sizeof(rattle_debug_support));
    *out = D;
    D->n_packs = np; D->n_cols = S.cols; D->level = in->sup ? 3 : 2;
    D->coff = result_array<uint64_t>(np); D->cons_len = result_array<uint32_t>(np); D->consensus = result_array<uint8_t>(S.cols);
    if (np) { memcpy(D->coff, S.coff.data(), (size_t)np * 8); memcpy(D->cons_len, C.len.data(), (size_t)np * 4); }
    if (S.cols) memcpy(D->consensus, C.cons.data(), S.cols);
    if (!ctx->consensus_support) return 0;
    uint32_t **dst[SUP_FIELDS] = {&D->support, &D->depth, &D->pack_support, &D->pack_depth};
    for (int f = 0; f < (in->sup ? SUP_FIELDS : 2); ++f) {
        *dst[f] = result_array<uint32_t>(S.cols);
        if (S.cols) memcpy(*dst[f], C.cnt.data() + (size_t)f * S.cnt_stride, S.cols * 4);
    }
    return 0;
}

// a step of this rank's own work: not run after an earlier one failed
#define LOCAL_TRY(call) do { if (J.local_rc == 0) RT_TRY(J.own_error(call)); } while (0)

int correct_driver(rattle_ctx *ctx, const uint8_t *seq, const uint8_t *qual, const uint64_t *off, uint32_t n_reads,
                   uint32_t n_clusters, const uint32_t *coff, const int32_t *mid, const uint8_t *mrev,
                   const rattle_correct_params *P, rattle_correction **out) {
    char order[8] = {0};
    RT_TRY(vote_order_of(P, order));
    rattle_correction *R = new_correction();
    *out = R;
    phase_timer T_all("correct: total");
    correct_job J{ctx, seq, qual, off, n_reads, n_clusters, P, order, R, ctx->xchg.rank, ctx->xchg.nranks, ctx->stream};
    RT_TRY(J.plan(coff, mid, mrev));
    LOCAL_TRY(ensure_post_constants(ctx));
    LOCAL_TRY(J.check_bases());
    J.unqueued_reads();
    if (J.nm) {
        LOCAL_TRY(J.upload_reads());
        LOCAL_TRY(J.stage1());
        LOCAL_TRY(J.stage1_finish());                // starts the download of the corrected reads
    }
    J.d_rseq.release(); J.d_rqual.release();
    std::vector<uint8_t> bytes, bytes_3b;
    std::vector<uint32_t> s2a, s2b;                  // my live packs of the big clusters / of all others
    for (uint32_t k = 0; k < J.nm; ++k) {
        const uint32_t p = J.mine[k];
        if (J.pk_dead[p]) write_stage_rec(bytes, p, 1u << 1, nullptr, 0);      // given up in stage 1: announced with the first exchange
        else (J.big[J.PL.pk_cid[p]] ? s2a : s2b).push_back(k);
    }
    // stage 2a: my packs of the big clusters
    LOCAL_TRY(J.cons_pass("correct: stage 2a", 2, s2a, {}, bytes));
    if (J.any_big) { RT_TRY(J.exchange_stage(bytes)); bytes.clear(); }
    // stage 2b+3a: POA #3 groups of the big clusters, my packs of all other clusters
    const std::vector<uint32_t> g3a = J.poa3_groups(true);
    LOCAL_TRY(J.cons_pass("correct: stage 2b+3a", 3, s2b, g3a, bytes));
    RT_TRY(J.exchange_stage(bytes));
    RT_TRY(J.own_error(J.join_download()));
    J.S1.release();                                  // the stage-1 rows are no longer needed once the download is done
    // stage 3b: POA #3 of the other clusters with more than one live pack
    size_t n3b = 0;
    const std::vector<uint32_t> g3b = J.poa3_groups(false, &n3b);
    LOCAL_TRY(J.cons_pass("correct: stage 3b", 4, {}, g3b, bytes_3b));
    // several ranks: this exchange always takes place, so that every rank leaves with the same verdict (the caller's
    // next collective is the gather of the corrected reads)
    if (n3b || J.nranks > 1 || xchg_recording(ctx)) RT_TRY(J.exchange_stage(bytes_3b));
    J.d_os.release(); J.d_oq.release();
    J.assemble();
    print_support_totals(R);
    print_report_totals(R, J.nranks > 1 ? "correction report (this rank's packs)" : "correction report");
    return 0;
}
#undef LOCAL_TRY

}  // namespace rattle
