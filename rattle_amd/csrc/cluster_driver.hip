// Host orchestration of the greedy clustering, /root/reference/cluster.cpp:93-259, over the
// device kernels A (bv_filter) and B (pair_score).
//
// The reference walks seeds one at a time and, per seed, spawns n_threads tasks over the
// remaining reads (cluster.cpp:138-158).  cluster_together(i,j) is a pure function of
// (i, j, threshold), and read j joins seed i iff j is still un-clustered when i is
// processed.  So a BATCH of the next B un-clustered items can be evaluated in one launch
// and resolved afterwards in index order with an identical result:
//   level 1: seeds x seeds  -> which seeds are absorbed by an earlier seed (exact founders)
//   level 2: founders x all remaining items -> each item joins the FIRST founder that accepts it
// The merge passes (cluster.cpp:171-256) are the same procedure over cluster representatives.
//
// One job over several GPUs: the reference cuts the candidate loop of a seed over its threads
// (cluster.cpp:138-158: thread t takes candidates t, t+T, ...).  Here rank r of R scores the candidates at
// positions r, r+R, ... of every level-2 evaluation (level 1, 256 x 256, is replicated), the accepted
// (seed, candidate, strand) triples are all-gathered and every rank resolves them identically.
//
// Many independent clusterings at once (`--iso`: one per gene cluster, main.cpp:281-318, which the reference
// runs one after another): every clustering is a small state machine (`job`) that stops whenever it needs a
// rectangle of cluster_together verdicts; the rectangles of all jobs that are waiting go to the device in ONE
// evaluation (kernel A over the rectangle list, kernel B over the union of the surviving pairs), the verdicts
// are dealt back and the jobs advance.  A round costs a handful of launches whatever the number of genes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "wire.h"

namespace rattle {

// survivor list (seed_slot<<1|strand, cand_slot) -> explicit (read i, read j, strand) pairs
__global__ void expand_pairs_kernel(const uint32_t *__restrict__ surv, uint32_t n, const uint32_t *__restrict__ seed_ids,
                                    const uint32_t *__restrict__ cand_ids, uint32_t *__restrict__ pi, uint32_t *__restrict__ pj,
                                    uint8_t *__restrict__ ps) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t a = surv[2 * (uint64_t)t], c = surv[2 * (uint64_t)t + 1];
    pi[t] = seed_ids[a >> 1];
    pj[t] = cand_ids[c];
    ps[t] = (uint8_t)(a & 1u);
}

// cluster.cpp:23-27 turned into an exact rejection on |common| (see evaluator::count_pass): pairs that can still reach t_s are compacted
// for the full comparison; survivors / matches per rectangle and the algorithmic bytes are summed on the way.
// stats: [0] pairs kept, [1] algorithmic bytes, then per rectangle (survivors, matches, pairs kept)
__global__ __launch_bounds__(256) void count_bound_kernel(const uint32_t *__restrict__ surv, const int32_t *__restrict__ common, uint32_t n,
                                                          const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj, const uint8_t *__restrict__ ps,
                                                          const uint32_t *__restrict__ len, uint32_t kk, double t_s,
                                                          const uint32_t *__restrict__ seed_rect, unsigned long long *__restrict__ stats,
                                                          uint32_t *__restrict__ pi2, uint32_t *__restrict__ pj2, uint8_t *__restrict__ ps2,
                                                          uint32_t *__restrict__ slot2) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < n;
    uint32_t a = 0, c = 0, ri = 0, rj = 0, rect = 0;
    unsigned long long M = 0, bytes = 0;
    bool keep = false;
    if (live) {
        a = surv[2 * (uint64_t)p]; c = surv[2 * (uint64_t)p + 1];
        M = (uint32_t)common[p];
        ri = pi[p]; rj = pj[p];
        const uint32_t li = len[ri], lj = len[rj];
        bytes = 8ull * ((li > kk ? li - kk : 0) + (lj > kk ? lj - kk : 0));
        const double mn = (double)(li < lj ? li : lj);
        keep = (double)(M * kk) / mn >= t_s;
        rect = seed_rect ? seed_rect[a >> 1] : 0u;
    }
    // one atomic per wavefront where its lanes agree on the rectangle (always, with a single rectangle)
    const uint32_t rect0 = __shfl(rect, 0, 64);
    const bool uniform = __all(!live || rect == rect0);
    unsigned long long mm = M, bb = bytes, one = live ? 1ull : 0ull;
    for (int d = 32; d; d >>= 1) { bb += __shfl_down(bb, d, 64); if (uniform) { mm += __shfl_down(mm, d, 64); one += __shfl_down(one, d, 64); } }
    const int lane = threadIdx.x & 63;
    if (lane == 0) atomicAdd(&stats[1], bb);
    if (uniform) {
        if (lane == 0 && one) { atomicAdd(&stats[2 + 3 * (size_t)rect0], one); atomicAdd(&stats[3 + 3 * (size_t)rect0], mm); }
    } else if (live) {
        atomicAdd(&stats[2 + 3 * (size_t)rect], 1ull); atomicAdd(&stats[3 + 3 * (size_t)rect], M);
    }
    const unsigned long long mask = __ballot(keep);
    if (mask) {
        if (uniform) { if (lane == 0) atomicAdd(&stats[4 + 3 * (size_t)rect0], (unsigned long long)__popcll(mask)); }
        else if (keep) atomicAdd(&stats[4 + 3 * (size_t)rect], 1ull);
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&stats[0], (unsigned long long)__popcll(mask));
        base = __shfl(base, 0, 64);
        if (keep) {
            const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            pi2[at] = ri; pj2[at] = rj; ps2[at] = ps[p];
            slot2[2 * at] = a; slot2[2 * at + 1] = c;
        }
    }
}

// cluster.cpp:23-36 / :47-61 on the device, in the reference's double arithmetic (an IEEE division and two comparisons, the same
// expression the host evaluated until round 3): the accepted pairs are compacted as (seed slot << 1 | strand, candidate slot), so
// the host sees the few accepted pairs instead of four integers and a double for every full comparison (10 M of them in the
// --iso level at 1e6 reads).  Pairs whose match list did not fit LDS are listed for the oversize pass (out[0] = count, out[1] =
// oversize pairs, out[2] = their largest match count) and judged by a second launch over that list.
//
// The report form (REPORT, the cluster report: rattle_hip_set_cluster_report) also writes what the full comparison computed for every
// accepted pair -- bases, hc_bases, the variance's 64 bits: one 16-byte vector store -- at the pair's compacted position, so evid[at]
// belongs to hits[2 * at ..] whichever of the two launches accepted it.
template <bool REPORT>
__device__ __forceinline__ void verdict_body(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                             const uint32_t *__restrict__ remap, const uint32_t *__restrict__ pi,
                                             const uint32_t *__restrict__ pj, const uint32_t *__restrict__ slot2,
                                             const uint32_t *__restrict__ len, int use_hc, double t_s, double t_v,
                                             unsigned long long *__restrict__ out, uint32_t *__restrict__ hits,
                                             uint32_t *__restrict__ big, uint4 *__restrict__ evid) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool ok = false, over = false;
    uint32_t q = 0, m_over = 0;
    if (t < n) {
        q = remap ? remap[t] : t;
        const int32_t *r = res + 4 * (size_t)q;
        if (r[0] == INT32_MIN) { over = true; m_over = (uint32_t)r[3]; }
        else {
            const uint32_t li = len[pi[q]], lj = len[pj[q]];
            const double mn = (double)(li < lj ? li : lj);
            const double score = use_hc ? (double)r[1] / mn : (double)r[0] / mn;
            ok = score >= t_s && var[q] < t_v;
        }
    }
    const unsigned long long mo = __ballot(over);
    if (mo) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&out[1], (unsigned long long)__popcll(mo));
        base = __shfl(base, 0, 64);
        if (over) { big[base + (uint64_t)__popcll(mo & ((1ull << lane) - 1ull))] = q; atomicMax(&out[2], (unsigned long long)m_over); }
    }
    const unsigned long long mk = __ballot(ok);
    if (mk) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&out[0], (unsigned long long)__popcll(mk));
        base = __shfl(base, 0, 64);
        if (ok) {
            const uint64_t at = base + (uint64_t)__popcll(mk & ((1ull << lane) - 1ull));
            hits[2 * at] = slot2[2 * (size_t)q]; hits[2 * at + 1] = slot2[2 * (size_t)q + 1];
            if (REPORT) {
                const int32_t *r = res + 4 * (size_t)q;
                const unsigned long long vb = (unsigned long long)__double_as_longlong(var[q]);
                evid[at] = make_uint4((uint32_t)r[0], (uint32_t)r[1], (uint32_t)vb, (uint32_t)(vb >> 32));
            }
        }
    }
}

__global__ __launch_bounds__(256) void verdict_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                      const uint32_t *__restrict__ remap, const uint32_t *__restrict__ pi,
                                                      const uint32_t *__restrict__ pj, const uint32_t *__restrict__ slot2,
                                                      const uint32_t *__restrict__ len, int use_hc, double t_s, double t_v,
                                                      unsigned long long *__restrict__ out, uint32_t *__restrict__ hits,
                                                      uint32_t *__restrict__ big) {
    verdict_body<false>(res, var, n, remap, pi, pj, slot2, len, use_hc, t_s, t_v, out, hits, big, nullptr);
}

__global__ __launch_bounds__(256) void verdict_report_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                             const uint32_t *__restrict__ remap, const uint32_t *__restrict__ pi,
                                                             const uint32_t *__restrict__ pj, const uint32_t *__restrict__ slot2,
                                                             const uint32_t *__restrict__ len, int use_hc, double t_s, double t_v,
                                                             unsigned long long *__restrict__ out, uint32_t *__restrict__ hits,
                                                             uint32_t *__restrict__ big, uint4 *__restrict__ evid) {
    verdict_body<true>(res, var, n, remap, pi, pj, slot2, len, use_hc, t_s, t_v, out, hits, big, evid);
}

namespace {

struct hit_t { uint32_t seed, cand; uint8_t rev; };

struct cseq { int32_t id; uint8_t rev; };

// one rectangle of cluster_together(i, j) evaluations a job waits for
struct request {
    std::vector<uint32_t> seeds, cands;       // loaded-read ids; triangular: candidates = the seeds, pairs (s, c > s) only
    bool triangular = false;
    double thr = 0.0;                         // bit-vector threshold of the pass (cluster.cpp:19,43)
    uint64_t *counters = nullptr;             // the job's work counters
    uint32_t tag = 0;                         // the test hook's rectangle number (eval_sink)
    std::vector<hit_t> hits;                  // out: accepted (seed index, candidate index, strand); sorted if triangular
    std::vector<hit_evidence> ev;             // out, only when the context reports (else empty): the evidence of hits[i]
    uint32_t n_cands() const { return (uint32_t)(triangular ? seeds.size() : cands.size()); }
    uint64_t n_pairs() const {
        const uint64_t s = seeds.size();
        return triangular ? s * (s - 1) / 2 : s * (uint64_t)cands.size();
    }
};

// What one evaluation computed on its way, for the test hook (rattle_hip_debug_evaluate): pairs as (request tag, seed index,
// candidate index, strand), the count pass's result of every survivor.  The greedy driver runs without one.
struct eval_sink {
    struct pair { uint32_t rect, seed, cand; uint8_t strand; int32_t count; };
    std::vector<pair> surv, kept;
    int count_pass = 0;                       // bit 0: the seed-major pass ran, bit 1: the per-pair search, bit 2: the seed-batch index
    uint64_t filter_launches = 0, oversize = 0;
};

// Every pair can survive the filter, and in the thr == 0 pass every pair does (cluster.cpp:19,43): one launch keeps its
// pairs x strands below the 32-bit survivor counter, and below 64 M where all of them survive.
constexpr uint64_t LAUNCH_PAIRS = 1ull << 31, LAUNCH_PAIRS_SURE = 64ull << 20;
// the seeds of a batch of `want` whose seeds x candidates x strands stay below these bounds even if every pair survives
uint32_t max_seeds_per_launch(uint64_t want, uint64_t cands, uint64_t strands, double thr) {
    const uint64_t per_seed = cands * strands, cap = thr == 0.0 ? LAUNCH_PAIRS_SURE : LAUNCH_PAIRS;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, cap / std::max<uint64_t>(per_seed, 1)));
}

// ---- device evaluation of a set of rectangles -------------------------------------------------------------
// what one evaluation (evaluator::run_local) hands from step to step
struct evaluation {
    rattle_ctx *ctx;
    request **reqs;
    size_t nreq;
    uint64_t ns = 0, nc = 0, npairs = 0;      // seeds, candidates and pairs of all rectangles side by side
    uint32_t tiles = 0, nrect = 0;
    bool many = false;                        // more than one request: the statistics go by seed_req
    std::vector<uint32_t> rect_req;           // rectangle -> its request (empty requests get no rectangle)
    uint32_t nsurv = 0, n2 = 0;               // survivors of the filter, pairs the count bound kept
    int form = 0;                             // the count pass: 1 seed-major, 2 search, 3 index
    // full_pass on: d_surv (free since the count pass compacted it into d_slot2) takes the accepted pairs, the tail of the statistics
    // buffer the three counters (device, host), d_pi2 (= the swapped-out d_pi: n2 <= nsurv words) the oversize list
    unsigned long long *vout = nullptr, *hv = nullptr;
    uint32_t *d_hits = nullptr, *d_big = nullptr;
    // the cluster report: the evidence of the accepted pairs (at most n2 of them over both verdict launches) beside them
    bool report = false;
    uint4 *d_ev = nullptr;
    // the launchers read d_pi / d_pj / d_ps: full_pass puts the kept pairs there, and they go back on every way out
    bool swapped = false;
    void swap_pairs() { ctx->d_pi.swap(ctx->d_pi2); ctx->d_pj.swap(ctx->d_pj2); ctx->d_ps.swap(ctx->d_ps2); swapped = !swapped; }
    ~evaluation() { if (swapped) swap_pairs(); }
};

struct evaluator {
    rattle_ctx *ctx;
    const rattle_cluster_params *P;
    uint64_t launches = 0;
    int count_mode = 0;                       // 0: RATTLE_PAIR_COUNT, else the nsurv >= 64 ns rule; 1: seed-major; 2: search; 3: index
    uint64_t n_form[3] = {0, 0, 0};           // evaluations whose count pass was seed-major / search / index (RATTLE_TIMING)
    eval_sink *sink = nullptr;                // test hook only
    // `assign`: the evaluation ends in the per-read reduction of assign.hip instead of the hit list (one rectangular request per
    // evaluation: target batch x reads); the batch's state and the index of the batch's first target
    const assign_dev *best = nullptr;
    uint32_t best_base = 0;
    const top_dev *top = nullptr;             // the batch's candidate list, if the call asks for one (assign_*_top)
    // RATTLE_TIMING: where the host's wall time of a clustering goes, by run_local's laps.  Lap 3 is the crediting of the count bound's
    // statistics to the jobs (the line prints it as "host bound test": the test itself has run on the device since round 3).
    double t_split[5] = {0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t_mark;
    void mark() { t_mark = std::chrono::steady_clock::now(); }
    void lap(int i) { const auto now = std::chrono::steady_clock::now(); t_split[i] += std::chrono::duration<double, std::milli>(now - t_mark).count(); t_mark = now; }
    std::vector<double> lut_thr;              // row r of the device table belongs to threshold lut_thr[r]
    std::vector<uint16_t> luts;
    std::vector<uint32_t> h_seed, h_cand, h_first, seed_req;
    std::vector<bvf_rect> rects;

    // min_common_lut[m] = smallest c with double(c)/double(m) >= thr  (cluster.cpp:19,43)
    int lut_row(double thr, uint32_t &row) {
        for (size_t r = 0; r < lut_thr.size(); ++r) if (lut_thr[r] == thr) { row = (uint32_t)r; return 0; }
        row = (uint32_t)lut_thr.size();
        lut_thr.push_back(thr);
        luts.resize((size_t)(row + 1) * 4097);
        uint16_t *lut = luts.data() + (size_t)row * 4097;
        for (int m = 0; m <= 4096; ++m) {
            double mmax = (double)m;
            int need = 0xFFFF;
            int lo = 0, hi = 4096;               // predicate is monotone in c for m > 0
            if (m > 0 && (double)(size_t)hi / mmax >= thr) {
                while (lo < hi) {
                    int mid = (lo + hi) / 2;
                    if ((double)(size_t)mid / mmax >= thr) hi = mid; else lo = mid + 1;
                }
                need = lo;
            }
            lut[m] = (uint16_t)need;
        }
        RT_TRY(ctx->d_lut.reserve(luts.size()));
        RT_HIP(hipMemcpyAsync(ctx->d_lut.p, luts.data(), luts.size() * 2, hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));   // luts may move on the next push
        return 0;
    }

    // The piece a rank contributes to the hit exchange of a sharded evaluation: the three counter deltas since `before`, then the hits as
    // (seed, candidate position, strand) triples.  A rank that scored the candidates at positions r, r + R, ... gives its stride and
    // offset, so that the positions are the whole request's; the whole request itself takes (1, 0).
    static std::vector<uint8_t> pack_piece(const uint64_t *counters, const uint64_t *before, const std::vector<hit_t> &hits, uint32_t R, uint32_t r) {
        const uint64_t deltas[3] = {counters[0] - before[0], counters[1] - before[1], counters[2] - before[2]};
        std::vector<wire_hit> t(hits.size());
        for (size_t i = 0; i < hits.size(); ++i) t[i] = wire_hit{hits[i].seed, hits[i].cand * R + r, hits[i].rev};
        std::vector<uint8_t> pay;
        write_hit_list(pay, deltas, t.data(), t.size());
        return pay;
    }

    // ... and the piece of rank `from` read back and checked against the request it answers: its deltas added to counters (unless
    // nullptr), its hits appended, except those at the candidate positions drop, drop + R, ... (drop < 0: none)
    static int unpack_piece(const std::vector<uint8_t> &b, int from, const request &q, uint64_t *counters, std::vector<hit_t> &hits, uint32_t R, int drop) {
        wire_reader W(b.data(), b.size());
        hit_list_view V;
        if (!parse_hit_list(W, q.seeds.size(), q.cands.size(), V)) { set_error(wire_error("cluster hit exchange", from, W)); return RATTLE_ERR_HIP; }
        if (counters) for (int i = 0; i < 3; ++i) counters[i] += V.deltas[i];
        for (size_t i = 0; i < V.n; ++i) {
            const wire_hit &t = V.hits[i];
            if (drop >= 0 && t.cand % R == (uint32_t)drop) continue;
            hits.push_back(hit_t{t.seed, t.cand, (uint8_t)t.rev});
        }
        return 0;
    }

    // All requests of one greedy step.  shard: this rank scores the candidates at positions rank, rank + nranks, ...
    // of the (single, rectangular) request and the hits of all ranks are all-gathered.
    int run(std::vector<request *> &reqs, bool shard) {
        const int R = ctx->xchg.nranks, r = ctx->xchg.rank;
        const bool sharded = shard && R > 1;
        if (!sharded && !(shard && xchg_recording(ctx))) return run_chunks(reqs);
        if (reqs.size() != 1 || reqs[0]->triangular) { set_error("sharded evaluation takes one rectangular request"); return RATTLE_ERR_STATE; }
        request &q = *reqs[0];
        const uint64_t before[3] = {q.counters[0], q.counters[1], q.counters[2]};
        std::vector<std::vector<uint8_t>> all;
        if (!sharded) {
            // single rank, recording: the same payload a sharded job exchanges here, for the whole request
            RT_TRY(run_chunks(reqs));
            return xchg_allgatherv(ctx, pack_piece(q.counters, before, q.hits, 1, 0), all);
        }
        request mine;
        mine.seeds = q.seeds; mine.thr = q.thr; mine.counters = q.counters;
        for (uint32_t c = (uint32_t)r; c < q.cands.size(); c += (uint32_t)R) mine.cands.push_back(q.cands[c]);
        std::vector<request *> one{&mine};
        RT_TRY(run_chunks(one));
        const std::vector<uint8_t> pay = pack_piece(q.counters, before, mine.hits, (uint32_t)R, (uint32_t)r);
        for (int i = 0; i < 3; ++i) q.counters[i] = before[i];       // every rank's deltas, this one's among them, come back below
        RT_TRY(xchg_allgatherv(ctx, pay, all));
        q.hits.clear();
        const bool replay = xchg_replaying(ctx);      // (measurement aid, common.h: the piece beside this rank's own is the WHOLE job's hit list)
        for (int p = 0; p < R; ++p) {
            const std::vector<uint8_t> &b = all[(size_t)p];
            if (replay && b.empty()) continue;
            // replaying: this rank's own counters and hits arrived in its own piece
            RT_TRY(unpack_piece(b, p, q, replay && p == r ? nullptr : q.counters, q.hits, (uint32_t)R, replay && p != r ? r : -1));
        }
        return 0;
    }

    static void sort_hits(request &Q) {
        std::vector<hit_t> &hits = Q.hits;
        auto before = [](const hit_t &a, const hit_t &b) {
            return a.seed != b.seed ? a.seed < b.seed : (a.cand != b.cand ? a.cand < b.cand : a.rev < b.rev);
        };
        if (Q.ev.empty()) { std::sort(hits.begin(), hits.end(), before); return; }
        // reporting: the evidence moves with its hit
        std::vector<uint32_t> at(hits.size());
        for (uint32_t i = 0; i < at.size(); ++i) at[i] = i;
        std::sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return before(hits[a], hits[b]); });
        std::vector<hit_t> h2(hits.size());
        std::vector<hit_evidence> e2(hits.size());
        for (size_t i = 0; i < at.size(); ++i) { h2[i] = hits[at[i]]; e2[i] = Q.ev[at[i]]; }
        hits.swap(h2); Q.ev.swap(e2);
    }

    // the requests in runs that stay below the per-launch bounds, one evaluation each
    int run_chunks(std::vector<request *> &reqs) {
        const uint64_t strands = ctx->idx.both ? 2u : 1u;
        size_t a = 0;
        while (a < reqs.size()) {
            uint64_t all_pairs = 0, sure = 0;
            size_t b = a;
            while (b < reqs.size()) {
                const uint64_t p = reqs[b]->n_pairs() * strands;
                const uint64_t s = reqs[b]->thr == 0.0 ? p : 0;
                if (b > a && (all_pairs + p > LAUNCH_PAIRS || sure + s > LAUNCH_PAIRS_SURE)) break;
                all_pairs += p; sure += s;
                ++b;
            }
            RT_TRY(run_local(reqs.data() + a, b - a));
            a = b;
        }
        return 0;
    }

    // one evaluation: the hits of every request (or, with `best` set, the batch's reduction) from the device
    int run_local(request **reqs, size_t nreq) {
        evaluation V{ctx, reqs, nreq};
        mark();
        RT_TRY(lay_out(V));
        if (V.ns == 0 || V.nc == 0) return 0;
        lap(0);
        RT_TRY(filter(V));
        lap(1);
        if (V.nsurv == 0) return 0;
        RT_TRY(count_pass(V));
        lap(2);
        RT_TRY(credit(V));
        lap(3);
        if (V.n2 == 0) return 0;
        RT_TRY(full_pass(V));
        RT_TRY(best ? reduce_best(V) : verdicts(V));
        lap(4);
        return 0;
    }

    // the rectangles side by side in one seed array and one candidate array, and on the device
    int lay_out(evaluation &V) {
        hipStream_t st = ctx->stream;
        for (size_t q = 0; q < V.nreq; ++q) {
            V.reqs[q]->hits.clear(); V.reqs[q]->ev.clear();
            if (V.reqs[q]->seeds.empty() || V.reqs[q]->n_cands() == 0) continue;
            V.ns += V.reqs[q]->seeds.size(); V.nc += V.reqs[q]->n_cands();
        }
        const uint64_t ns = V.ns, nc = V.nc;
        if (ns == 0 || nc == 0) return 0;
        if (ns >= (1u << 31) || nc >= 0xFFFFFFF0ull) { set_error("cluster evaluation: too many seeds or candidates in one step"); return RATTLE_ERR_ARG; }
        h_seed.resize(ns); h_first.resize(ns); h_cand.resize(nc);
        rects.clear();
        V.many = V.nreq > 1;
        if (V.many) seed_req.resize(ns);
        uint32_t sb = 0, cb = 0;
        for (size_t q = 0; q < V.nreq; ++q) {
            request &Q = *V.reqs[q];
            const uint32_t qs = (uint32_t)Q.seeds.size(), qc = Q.n_cands();
            if (qs == 0 || qc == 0) continue;
            uint32_t row = 0;
            RT_TRY(lut_row(Q.thr, row));
            memcpy(h_seed.data() + sb, Q.seeds.data(), (size_t)qs * 4);
            memcpy(h_cand.data() + cb, Q.triangular ? Q.seeds.data() : Q.cands.data(), (size_t)qc * 4);
            for (uint32_t s = 0; s < qs; ++s) h_first[sb + s] = cb + (Q.triangular ? s + 1 : 0u);
            if (V.many) for (uint32_t s = 0; s < qs; ++s) seed_req[sb + s] = (uint32_t)rects.size();
            rects.push_back(bvf_rect{sb, qs, cb, qc, V.tiles, row * 4097u, Q.thr == 0.0 ? 1u : 0u, 0u});
            V.rect_req.push_back((uint32_t)q);
            V.tiles += ((qc + 255u) / 256u) * ((qs + 31u) / 32u);
            const uint64_t p = Q.n_pairs();
            Q.counters[0] += p;
            V.npairs += p;
            sb += qs; cb += qc;
        }
        V.nrect = (uint32_t)rects.size();
        RT_TRY(ctx->d_seed.reserve(ns)); RT_TRY(ctx->d_first.reserve(ns)); RT_TRY(ctx->d_cand.reserve(nc));
        RT_TRY(ctx->d_rect.reserve(V.nrect));
        RT_TRY(ctx->d_counter.reserve(4)); RT_TRY(ctx->h_counter.reserve(4));
        RT_HIP(hipMemcpyAsync(ctx->d_seed.p, h_seed.data(), ns * 4, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(ctx->d_first.p, h_first.data(), ns * 4, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(ctx->d_cand.p, h_cand.data(), nc * 4, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(ctx->d_rect.p, rects.data(), (size_t)V.nrect * sizeof(bvf_rect), hipMemcpyHostToDevice, st));
        return 0;
    }

    // kernel A over the rectangle list.  Survivor capacity: grow and retry on overflow (the count is exact even when truncated)
    int filter(evaluation &V) {
        hipStream_t st = ctx->stream;
        size_t cap = std::max<size_t>(ctx->d_surv.cap / 2, 1u << 20);
        while (true) {
            RT_TRY(ctx->d_surv.reserve(cap * 2));
            cap = ctx->d_surv.cap / 2;
            RT_HIP(hipMemsetAsync(ctx->d_counter.p, 0, 16, st));
            RT_TRY(launch_bv_filter_rects(ctx, V.nrect, V.tiles, V.npairs, false, true, (uint32_t)std::min<size_t>(cap, 0xFFFFFFF0u)));
            ++launches;
            if (sink) ++sink->filter_launches;
            RT_HIP(hipMemcpyAsync(ctx->h_counter.p, ctx->d_counter.p, 4, hipMemcpyDeviceToHost, st));
            RT_HIP(hipStreamSynchronize(st));
            V.nsurv = ctx->h_counter.p[0];
            if ((uint64_t)V.nsurv > V.npairs * 2) { set_error("bv_filter: survivor counter overflow"); return RATTLE_ERR_HIP; }
            if (V.nsurv <= cap) return 0;
            cap = (size_t)V.nsurv + V.nsurv / 8;
        }
    }

    // Three count passes.  "seed" (1): survivors sorted by seed, the seed's k-mer set as a bit set in LDS, its candidates' lists
    // streamed past it (pair_count.hip) -- pays where a seed has many surviving candidates (gene level: hundreds).
    // "search" (2): one wavefront per pair, binary searches in the candidate's list (pair_score.hip) -- better for the short
    // runs of the --iso level.  "index" (3): an inverted k-mer index over the seeds, every candidate's list streamed once
    // (pair_index.hip) -- for long reads, where the bit-vector filter lets every pair through.  RATTLE_PAIR_COUNT=
    // seed|search|index forces one of them (any other value: search); the automatic rule picks between the first two.
    int choose_form(uint64_t nsurv, uint64_t ns) const {
        static const char *force = getenv("RATTLE_PAIR_COUNT");
        return count_mode ? count_mode
               : force    ? (!strcmp(force, "seed") ? 1 : !strcmp(force, "index") ? 3 : 2)
                          : nsurv >= 64ull * ns ? 1 : 2;
    }

    // pass 1: |common| of every surviving pair.  bases <= k * |LIS| <= k * |common| (similarity.cpp:52-85), so a pair
    // with double(k * |common|) / min_len < t_s cannot pass cluster.cpp:23-27 whatever its chain looks like: exact
    // rejection without the patience search.  In the low-threshold merge passes that is nearly every pair.  The test
    // (same double expression) and the compaction of the pairs that pass run on the device (count_bound_kernel).
    int count_pass(evaluation &V) {
        hipStream_t st = ctx->stream;
        const uint32_t nsurv = V.nsurv;
        const size_t nstat = 2 + 3 * (size_t)V.nrect;
        RT_TRY(ctx->d_pi.reserve(nsurv));
        RT_TRY(ctx->d_pj.reserve(nsurv));
        RT_TRY(ctx->d_ps.reserve(nsurv));
        RT_TRY(ctx->d_res.reserve((size_t)nsurv * 4));
        RT_TRY(ctx->d_pi2.reserve(nsurv)); RT_TRY(ctx->d_pj2.reserve(nsurv)); RT_TRY(ctx->d_ps2.reserve(nsurv)); RT_TRY(ctx->d_slot2.reserve((size_t)nsurv * 2));
        RT_TRY(ctx->d_bound_stats.reserve(nstat + 4)); RT_TRY(ctx->h_bound_stats.reserve(nstat + 4));
        if (V.many) {
            RT_TRY(ctx->d_seed_rect.reserve(V.ns));
            RT_HIP(hipMemcpyAsync(ctx->d_seed_rect.p, seed_req.data(), V.ns * 4, hipMemcpyHostToDevice, st));
        }
        RT_HIP(hipMemsetAsync(ctx->d_bound_stats.p, 0, (nstat + 4) * 8, st));
        V.form = choose_form(nsurv, V.ns);
        if (sink) sink->count_pass |= 1 << (V.form - 1);
        ++n_form[V.form - 1];
        if (V.form == 1) RT_TRY(sort_survivors_by_seed(ctx, nsurv, V.ns));
        if (V.form == 3) RT_TRY(group_survivors_by_cand(ctx, nsurv, V.nc));
        hipLaunchKernelGGL(expand_pairs_kernel, dim3((nsurv + 255) / 256), dim3(256), 0, st, ctx->d_surv.p, nsurv,
                           ctx->d_seed.p, ctx->d_cand.p, ctx->d_pi.p, ctx->d_pj.p, ctx->d_ps.p);
        if (V.form == 1) RT_TRY(launch_pair_count_seed(ctx, nsurv));
        else if (V.form == 3) RT_TRY(launch_pair_count_index(ctx, nsurv, h_seed.data(), (uint32_t)V.ns, (uint32_t)V.nc, V.many));
        else RT_TRY(launch_pair_count(ctx, nsurv));
        hipLaunchKernelGGL(count_bound_kernel, dim3((nsurv + 255) / 256), dim3(256), 0, st, ctx->d_surv.p, ctx->d_res.p, nsurv,
                           ctx->d_pi.p, ctx->d_pj.p, ctx->d_ps.p, ctx->idx.len.p, (uint32_t)ctx->idx.k, P->t_s,
                           V.many ? ctx->d_seed_rect.p : (const uint32_t *)nullptr,
                           ctx->d_bound_stats.p, ctx->d_pi2.p, ctx->d_pj2.p, ctx->d_ps2.p, ctx->d_slot2.p);
        launches += 3;
        RT_HIP(hipMemcpyAsync(ctx->h_bound_stats.p, ctx->d_bound_stats.p, nstat * 8, hipMemcpyDeviceToHost, st));
        RT_HIP(hipStreamSynchronize(st));
        V.n2 = (uint32_t)ctx->h_bound_stats.p[0];
        return 0;
    }

    // the count bound's statistics to the jobs' counters
    int credit(evaluation &V) {
        if (sink) RT_TRY(take_pairs(V.reqs, V.rect_req, V.nsurv, V.n2));      // before pass 2 overwrites d_res
        ctx->stats[K_SCORE].bytes += ctx->h_bound_stats.p[1];
        for (uint32_t j = 0; j < V.nrect; ++j) {
            uint64_t *cn = V.reqs[V.rect_req[j]]->counters;
            cn[1] += ctx->h_bound_stats.p[2 + 3 * (size_t)j]; cn[2] += ctx->h_bound_stats.p[3 + 3 * (size_t)j];
            cn[5] += ctx->h_bound_stats.p[4 + 3 * (size_t)j];                  // full comparisons (cluster.cpp:20 / :44 calls that ran)
        }
        return 0;
    }

    // pass 2: the reference's full comparison for the pairs that can still be accepted
    int full_pass(evaluation &V) {
        RT_TRY(ctx->d_res.reserve((size_t)V.n2 * 4));
        RT_TRY(ctx->d_var.reserve(V.n2));
        V.swap_pairs();
        V.vout = ctx->d_bound_stats.p + 2 + 3 * (size_t)V.nrect; V.hv = ctx->h_bound_stats.p + 2 + 3 * (size_t)V.nrect;
        V.d_hits = ctx->d_surv.p; V.d_big = ctx->d_pi2.p;
        RT_TRY(launch_pair_score(ctx, V.n2));
        ++launches;
        return 0;
    }

    // cluster.cpp:23-36 / :47-61 for all n kept pairs (remap == nullptr) or the n listed in remap: the one verdict launch
    int judge(evaluation &V, uint32_t n, const uint32_t *remap) {
        const dim3 grid((n + 255) / 256), block(256);
        const int use_hc = P->use_hc ? 1 : 0;
        if (V.report)
            hipLaunchKernelGGL(verdict_report_kernel, grid, block, 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, remap, ctx->d_pi.p, ctx->d_pj.p,
                               ctx->d_slot2.p, ctx->idx.len.p, use_hc, P->t_s, P->t_v, V.vout, V.d_hits, V.d_big, V.d_ev);
        else
            hipLaunchKernelGGL(verdict_kernel, grid, block, 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, remap, ctx->d_pi.p, ctx->d_pj.p,
                               ctx->d_slot2.p, ctx->idx.len.p, use_hc, P->t_s, P->t_v, V.vout, V.d_hits, V.d_big);
        ++launches;
        return 0;
    }

    // Both endings' first judging launch listed the pairs whose match list did not fit LDS (hv[1] of them in d_big, the longest list
    // hv[2]): rerun them through the global-scratch variant, which fills their res / var in place, and judge the list again.
    template <class Judge>
    int oversize_pass(evaluation &V, Judge again) {
        hipStream_t st = ctx->stream;
        const uint32_t nbig = (uint32_t)V.hv[1], big_m = (uint32_t)V.hv[2];
        if (V.hv[1] > V.n2) { set_error("evaluation: more oversize pairs than full comparisons"); return RATTLE_ERR_HIP; }
        std::vector<uint32_t> big(nbig);
        RT_HIP(hipMemcpyAsync(big.data(), V.d_big, (size_t)nbig * 4, hipMemcpyDeviceToHost, st));
        RT_HIP(hipStreamSynchronize(st));
        RT_TRY(launch_pair_score_oversize(ctx, big, big_m));
        ++launches;
        if (sink) sink->oversize += nbig;
        RT_HIP(hipMemsetAsync(V.vout + 1, 0, 16, st));
        RT_TRY(again(nbig, (const uint32_t *)V.d_big));
        RT_HIP(hipMemcpyAsync(V.hv, V.vout, 24, hipMemcpyDeviceToHost, st));
        RT_HIP(hipStreamSynchronize(st));
        if (V.hv[1]) { set_error("pair_score: a pair is still oversize after the oversize pass"); return RATTLE_ERR_HIP; }
        return 0;
    }

    // the first n accepted pairs, and their evidence, to the host; the three counters with them if asked
    int fetch_hits(evaluation &V, uint32_t n, bool counters) {
        hipStream_t st = ctx->stream;
        RT_TRY(ctx->h_surv.reserve((size_t)n * 2 + 2));
        if (counters) RT_HIP(hipMemcpyAsync(V.hv, V.vout, 24, hipMemcpyDeviceToHost, st));
        if (n) RT_HIP(hipMemcpyAsync(ctx->h_surv.p, V.d_hits, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        if (V.report && n) {
            RT_TRY(ctx->h_hit_ev.reserve(n));
            RT_HIP(hipMemcpyAsync(ctx->h_hit_ev.p, V.d_ev, (size_t)n * sizeof(hit_evidence), hipMemcpyDeviceToHost, st));
        }
        RT_HIP(hipStreamSynchronize(st));
        return 0;
    }

    // accepted pairs back to their rectangle
    void deal_hits(evaluation &V, uint32_t nhit) {
        for (uint32_t q = 0; q < nhit; ++q) {
            const uint32_t a = ctx->h_surv.p[2 * (size_t)q], c = ctx->h_surv.p[2 * (size_t)q + 1];
            const uint32_t rj = V.many ? seed_req[a >> 1] : 0;
            const bvf_rect &J = rects[rj];
            request &Q = *V.reqs[V.rect_req[rj]];
            Q.hits.push_back(hit_t{(a >> 1) - J.s_base, c - J.c_base, (uint8_t)(a & 1u)});
            if (V.report) Q.ev.push_back(ctx->h_hit_ev.p[q]);
        }
        for (uint32_t j = 0; j < V.nrect; ++j) if (V.reqs[V.rect_req[j]]->triangular) sort_hits(*V.reqs[V.rect_req[j]]);      // level 2 takes them in any order
    }

    // The ending of a clustering's evaluation: the verdicts on the device, the accepted pairs as each request's hit list.
    int verdicts(evaluation &V) {
        V.report = ctx->cluster_report;
        if (V.report) { RT_TRY(ctx->d_hit_ev.reserve(V.n2)); V.d_ev = (uint4 *)ctx->d_hit_ev.p; }
        RT_TRY(judge(V, V.n2, nullptr));
        // the first accepted pairs travel with the counters (one synchronisation per evaluation instead of two: the --iso level
        // runs ~1000 evaluations of ~1000 accepted pairs each)
        const uint32_t spec = std::min<uint32_t>(V.n2, 8192u);
        RT_TRY(fetch_hits(V, spec, true));
        const bool nbig_seen = V.hv[1] != 0;
        if (nbig_seen) RT_TRY(oversize_pass(V, [&](uint32_t n, const uint32_t *remap) { return judge(V, n, remap); }));
        const uint32_t nhit = (uint32_t)V.hv[0];
        if (V.hv[0] > V.n2) { set_error("verdicts: more accepted pairs than full comparisons"); return RATTLE_ERR_HIP; }
        // more than came along (or the oversize pass appended some): fetch them all
        if (nhit > spec || nbig_seen) RT_TRY(fetch_hits(V, nhit, false));
        deal_hits(V, nhit);
        return 0;
    }

    // The other ending (`assign`): no hit list; every accepted pair goes into the per-read reduction.  Pass 1 also lists the pairs whose
    // match list did not fit LDS, as the verdict kernel does, and takes them in again after the oversize pass, before passes 2 and 3
    // run over all n2 pairs.  The host reads the three counters (and the oversize slots).
    int reduce_best(evaluation &V) {
        if (V.nrect != 1 || rects[0].s_base != 0 || rects[0].c_base != 0) { set_error("assign: one rectangular request per evaluation"); return RATTLE_ERR_STATE; }
        const int use_hc = P->use_hc ? 1 : 0;
        auto pass1 = [&](uint32_t n, const uint32_t *remap) {
            RT_TRY(launch_assign_max(ctx, n, remap, use_hc, P->t_s, P->t_v, V.vout, V.d_big, *best));
            ++launches;
            return 0;
        };
        RT_TRY(pass1(V.n2, nullptr));
        RT_HIP(hipMemcpyAsync(V.hv, V.vout, 24, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
        if (V.hv[1]) RT_TRY(oversize_pass(V, pass1));
        RT_TRY(launch_assign_pick(ctx, V.n2, use_hc, P->t_s, P->t_v, best_base, *best));
        launches += 2;
        // the candidate list is a further ending over the same pairs, behind the oversize pass like passes 2 and 3 (it starts from their
        // record); it adds no synchronisation
        if (top) {
            RT_TRY(launch_assign_top(ctx, V.n2, (uint32_t)V.nc, use_hc, P->t_s, P->t_v, best_base, *best, *top));
            launches += top->k > 1 ? 2 * top->k : 1;
        }
        return 0;
    }

    // test hook: the survivors with their counts (d_surv / d_res after count_bound_kernel) and the kept pairs (d_slot2)
    int take_pairs(request **reqs, const std::vector<uint32_t> &rect_req, uint32_t nsurv, uint32_t n2) {
        std::vector<uint32_t> surv((size_t)nsurv * 2), slot2((size_t)n2 * 2);
        std::vector<int32_t> cnt(nsurv);
        RT_HIP(hipMemcpyAsync(surv.data(), ctx->d_surv.p, surv.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipMemcpyAsync(cnt.data(), ctx->d_res.p, cnt.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (n2) RT_HIP(hipMemcpyAsync(slot2.data(), ctx->d_slot2.p, slot2.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
        const bool many = rects.size() > 1;
        auto pair_of = [&](uint32_t a, uint32_t c, int32_t count) {
            const uint32_t rj = many ? seed_req[a >> 1] : 0;
            const bvf_rect &J = rects[rj];
            return eval_sink::pair{reqs[rect_req[rj]]->tag, (a >> 1) - J.s_base, c - J.c_base, (uint8_t)(a & 1u), count};
        };
        for (uint32_t p = 0; p < nsurv; ++p) sink->surv.push_back(pair_of(surv[2 * (size_t)p], surv[2 * (size_t)p + 1], cnt[p]));
        for (uint32_t p = 0; p < n2; ++p) sink->kept.push_back(pair_of(slot2[2 * (size_t)p], slot2[2 * (size_t)p + 1], 0));
        return 0;
    }
};

// ---- one clustering (cluster.cpp:93-259) as a state machine ------------------------------------------------
struct job {
    const read_index *X = nullptr;
    const rattle_cluster_params *P = nullptr;
    const uint32_t *subset = nullptr;     // local id -> loaded read id (nullptr = identity)
    uint32_t n = 0;
    bool inner_parallel = true;           // a lone job spreads its representative choice over the host threads
    uint32_t longest = 0;                 // longest read of this job (start()): decides the seed batch
    uint64_t counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    struct cl { cseq main; std::vector<cseq> seqs; };
    std::vector<cl> clusters;
    enum { INITIAL, MERGE, DONE } stage = INITIAL;
    double thr = 0.0;
    bool last = false;

    // the greedy pass in flight: owner[i] = index of the founder item that absorbed i (owner[i] == i for founders),
    // rev[i] = strand of the match
    enum { ROUND, WAIT_L1, FOUNDERS, WAIT_L2 } phase = ROUND;
    std::vector<uint32_t> items, owner, remaining, next, seeds_local, founders, best;
    std::vector<uint8_t> rev, taken;
    // the cluster report: the evidence of the hit that decided owner[i] / rev[i], the winning hit per level-2 candidate, the joins so far
    bool report = false;
    uint32_t pass_no = 0;
    std::vector<hit_evidence> why;
    std::vector<uint32_t> best_at;
    std::vector<cluster_join> joins;
    uint32_t B = 0, batch_now = 0;
    request rq;
    double t_phase[5] = {0, 0, 0, 0, 0};                   // RATTLE_TIMING: round set-up, level-1 resolve, founders + request, level-2 resolve, end of pass

    uint32_t rid(uint32_t local) const { return subset ? subset[local] : local; }
    uint32_t rlen(uint32_t local) const { return X->h_len[rid(local)]; }

    // cluster.cpp:67-91.  The reference's two stable sorts (by id descending, then by length descending) leave the
    // sequences ordered by (length desc, id desc); ids are unique in a cluster, so one sort on that key gives the
    // same order, and a cluster no merge touched is still in it.
    cseq get_main_seq(std::vector<cseq> &seqs, double repr_percentile) const {
        cseq old = seqs[0];
        auto key = [this](const cseq &a) { return ((uint64_t)rlen((uint32_t)a.id) << 32) | (uint32_t)a.id; };
        bool sorted = true;
        for (size_t i = 1; i < seqs.size() && sorted; ++i) sorted = key(seqs[i - 1]) > key(seqs[i]);
        if (!sorted) {
            std::vector<std::pair<uint64_t, uint8_t>> tmp(seqs.size());
            for (size_t i = 0; i < seqs.size(); ++i) tmp[i] = {key(seqs[i]), seqs[i].rev};
            std::sort(tmp.begin(), tmp.end(), [](const std::pair<uint64_t, uint8_t> &a, const std::pair<uint64_t, uint8_t> &b) { return a.first > b.first; });
            for (size_t i = 0; i < seqs.size(); ++i) seqs[i] = cseq{(int32_t)(uint32_t)tmp[i].first, tmp[i].second};
        }
        int nsid = seqs.size() * repr_percentile;
        cseq ns = seqs[nsid];
        while (ns.rev != old.rev && (size_t)nsid < seqs.size() - 1) { nsid++; ns = seqs[nsid]; }
        if ((size_t)nsid == seqs.size() - 1) return old;
        return ns;
    }

    void begin_pass(double t) {
        thr = t;
        const uint32_t m = (uint32_t)items.size();
        owner.resize(m);
        rev.assign(m, 0);
        if (report) why.assign(m, hit_evidence{0, 0, 0.0});
        remaining.resize(m);
        for (uint32_t i = 0; i < m; ++i) { owner[i] = i; remaining[i] = i; }
        phase = ROUND;
        // The outcome does not depend on the batch size (level 1 resolves the seeds exactly), the work does: level 1
        // costs B^2/2 comparisons, which is wasted where a few founders absorb everything (a gene's reads falling into
        // its few isoforms).  Start small on small problems and follow the number of founders the last round produced.
        batch_now = m > 4096 ? max_batch() : std::min<uint32_t>(max_batch(), 16);
    }

    uint32_t max_batch() const {
        // A lone clustering (the gene level): 1024 -- 77 greedy rounds instead of 119 at 1e6 reads (each ends in a handful of stream
        // synchronisations) for twice the level-1 comparisons; measured on one box: 340 ms (512), 314 ms (1024), 337 ms (2048).
        // The many clusterings of the --iso level keep 512: a gene's reads fall into few isoforms and a batch that follows the
        // founders up to 1024 doubled the full comparisons there (10.5 M -> 20.9 M, 0.91 -> 1.28 s).  RATTLE_SEED_BATCH overrides both.
        // Long reads: level 1's B^2 / 2 seed-against-seed comparisons are FULL comparisons of the longest reads of the round, and a round's
        // full pass lasts as long as its longest pair.  5e5 mixed-length reads (150 nt - 98 kb, config 5), `cluster` on one box: 22.8 s
        // (32), 20.7 (64), 19.4 (128), 20.4 (256), 23.3 (512), 32.9 (1024), 52.3 (2048) -- the step from 512 to 1024 was round 4's
        // unexplained 22.8 -> 33.8 s (profiles/round5_bisect_config5_cluster.txt).  So 256 as soon as a read is beyond the packed classes.
        static const uint32_t forced = getenv("RATTLE_SEED_BATCH") ? (uint32_t)std::max(1, atoi(getenv("RATTLE_SEED_BATCH"))) : 0u;
        return forced ? forced : longest > 4096u ? 256u : inner_parallel ? 1024u : 512u;
    }

    void start() {
        rq.counters = counters;
        items.resize(n);
        for (uint32_t i = 0; i < n; ++i) items[i] = i;
        longest = 0;
        for (uint32_t i = 0; i < n; ++i) longest = std::max(longest, rlen(i));
        stage = INITIAL;
        begin_pass(P->bv_threshold);
    }

    void choose_mains() {
        // clusters no merge touched are still in order (one linear check); only the others are sorted, on a few host
        // threads when there is enough of it (spawning a thread per core costs more than most passes' sorting)
        std::vector<uint32_t> big;
        size_t work = 0;
        for (uint32_t i = 0; i < clusters.size(); ++i) {
            if (inner_parallel && clusters[i].seqs.size() >= 4096) { big.push_back(i); work += clusters[i].seqs.size(); continue; }
            clusters[i].main = get_main_seq(clusters[i].seqs, P->repr_percentile);
        }
        parallel_for(big.size(), work >= (1u << 18) ? 16 : 1, [&](size_t t) { cl &c = clusters[big[t]]; c.main = get_main_seq(c.seqs, P->repr_percentile); });
    }

    // the merge loop's head, cluster.cpp:171: `while (thr >= min_bv_threshold || last)`
    void next_merge(double t) {
        if (!(t >= P->min_bv_threshold || last)) { stage = DONE; return; }
        stage = MERGE;
        const uint32_t nc = (uint32_t)clusters.size();
        items.resize(nc);
        for (uint32_t i = 0; i < nc; ++i) items[i] = (uint32_t)clusters[i].main.id;     // main_seq.rev ignored (:197)
        begin_pass(t);
    }

    // one join per absorbed item of the pass that ends, in item order (items: local read ids -- the reads themselves in the initial
    // pass, the clusters' representatives in a merge pass)
    void emit_joins() {
        for (uint32_t i = 0; i < items.size(); ++i) {
            if (owner[i] == i) continue;
            const uint32_t into = items[owner[i]], absorbed = items[i];
            const hit_evidence &e = why[i];
            const uint32_t li = rlen(into), lj = rlen(absorbed);
            const double mn = (double)(li < lj ? li : lj);
            const double score = P->use_hc ? (double)e.hc / mn : (double)e.bases / mn;      // the verdict's expression
            joins.push_back(cluster_join{pass_no, thr, (int32_t)into, (int32_t)absorbed, rev[i], 0, e.bases, e.hc, li < lj ? li : lj, score, e.var});
        }
        ++pass_no;
    }

    void end_pass() {
        if (report) emit_joins();
        if (stage == INITIAL) {                                   // cluster.cpp:124-166
            std::vector<int32_t> slot(n, -1);
            std::vector<uint32_t> size(n, 0);
            for (uint32_t i = 0; i < n; ++i) ++size[owner[i]];
            for (uint32_t i = 0; i < n; ++i)
                if (owner[i] == i) {
                    slot[i] = (int32_t)clusters.size();
                    clusters.push_back(cl{{(int32_t)i, 0}, {}});
                    clusters.back().seqs.reserve(size[i]);
                    clusters.back().seqs.push_back(cseq{(int32_t)i, 0});
                }
            for (uint32_t i = 0; i < n; ++i)
                if (owner[i] != i) clusters[slot[owner[i]]].seqs.push_back(cseq{(int32_t)i, rev[i]});
            choose_mains();
            next_merge(P->bv_threshold - P->bv_falloff);
            return;
        }
        const uint32_t nc = (uint32_t)clusters.size();            // cluster.cpp:171-256
        std::vector<cl> merged;
        std::vector<int32_t> slot(nc, -1);
        for (uint32_t i = 0; i < nc; ++i)
            if (owner[i] == i) { slot[i] = (int32_t)merged.size(); merged.push_back(cl{{0, 0}, {}}); merged.back().seqs = std::move(clusters[i].seqs); }
        for (uint32_t i = 0; i < nc; ++i) {
            if (owner[i] == i) continue;
            cl &dst = merged[slot[owner[i]]];
            for (cseq s : clusters[i].seqs) {                     // :227-238
                if (rev[i]) s.rev = !s.rev;
                dst.seqs.push_back(s);
            }
        }
        clusters.swap(merged);
        choose_mains();
        if (last) { stage = DONE; return; }
        double t = thr - P->bv_falloff;                           // :251-255
        if (t < P->min_bv_threshold && !last) { last = true; t = 0.0; }
        next_merge(t);
    }

    // ---- the four phases of a greedy round (step).  The two that ask for an evaluation fill rq and say so (true).
    // the round's seeds; level 1: seeds x seeds
    bool round_setup() {
        if (remaining.empty()) { end_pass(); return false; }
        counters[3]++;
        // seeds x candidates x strands below the evaluator's per-launch bounds even if every pair survives
        B = max_seeds_per_launch(std::min<size_t>(batch_now, remaining.size()), remaining.size(), X->both ? 2u : 1u, thr);
        seeds_local.resize(B);
        for (uint32_t s = 0; s < B; ++s) seeds_local[s] = items[remaining[s]];
        taken.assign(B, 0);
        if (B == 1) { phase = FOUNDERS; return false; }
        rq.seeds.resize(B);
        for (uint32_t s = 0; s < B; ++s) rq.seeds[s] = rid(seeds_local[s]);
        rq.cands.clear();
        rq.triangular = true; rq.thr = thr;
        phase = WAIT_L1;
        return true;
    }

    // the seeds no earlier seed absorbed; level 2: founders x rest
    bool pick_founders() {
        founders.clear();
        for (uint32_t s = 0; s < B; ++s) if (!taken[s]) founders.push_back(s);
        uint32_t want = 8;
        while (want < 2 * founders.size() && want < max_batch()) want *= 2;
        batch_now = std::min(want, max_batch());
        const uint32_t nrest = (uint32_t)remaining.size() - B;
        next.clear();
        if (nrest == 0) { remaining.swap(next); phase = ROUND; return false; }
        rq.seeds.resize(founders.size());
        for (size_t f = 0; f < founders.size(); ++f) rq.seeds[f] = rid(seeds_local[founders[f]]);
        rq.cands.resize(nrest);
        for (uint32_t c = 0; c < nrest; ++c) rq.cands[c] = rid(items[remaining[B + c]]);
        rq.triangular = false; rq.thr = thr;
        phase = WAIT_L2;
        return true;
    }

    // hits grouped by seed; forward verdict wins over reverse (cluster.cpp:19-40 before :43)
    void resolve_level1() {
        const std::vector<hit_t> &hits = rq.hits;
        size_t h = 0;
        for (uint32_t s = 0; s < B; ++s) {
            while (h < hits.size() && hits[h].seed < s) ++h;
            if (taken[s]) continue;
            for (size_t q = h; q < hits.size() && hits[q].seed == s; ++q) {
                uint32_t c = hits[q].cand;
                if (taken[c]) continue;
                taken[c] = 1;
                owner[remaining[c]] = remaining[s];
                rev[remaining[c]] = hits[q].rev;
                if (report) why[remaining[c]] = rq.ev[q];
            }
        }
        phase = FOUNDERS;
    }

    // founders in order, the first accepting founder wins, forward before reverse: the smallest (founder, strand)
    // key per candidate, whatever order the hits arrive in
    void resolve_level2() {
        const uint32_t nrest = (uint32_t)remaining.size() - B;
        best.assign(nrest, 0xFFFFFFFFu);
        if (!report) for (const hit_t &q : rq.hits) best[q.cand] = std::min(best[q.cand], (q.seed << 1) | q.rev);
        else {                                            // ... and which hit that was (a key occurs once per candidate)
            best_at.resize(nrest);
            for (uint32_t h = 0; h < rq.hits.size(); ++h) {
                const hit_t &q = rq.hits[h];
                const uint32_t key = (q.seed << 1) | q.rev;
                if (key < best[q.cand]) { best[q.cand] = key; best_at[q.cand] = h; }
            }
        }
        for (uint32_t c = 0; c < nrest; ++c) {
            if (best[c] == 0xFFFFFFFFu) { next.push_back(remaining[B + c]); continue; }
            owner[remaining[B + c]] = remaining[founders[best[c] >> 1]];
            rev[remaining[B + c]] = (uint8_t)(best[c] & 1u);
            if (report) why[remaining[B + c]] = rq.ev[best_at[c]];
        }
        remaining.swap(next);
        phase = ROUND;
    }

    // advance until the job needs a rectangle evaluated (true, *out) or is finished (false)
    bool step(request **out) {
        while (stage != DONE) {
            struct lapse { double &acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                           ~lapse() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } };
            const bool ending = phase == ROUND && remaining.empty();
            lapse L{t_phase[ending ? 4 : (int)phase]};
            bool ask = false;
            switch (phase) {
            case ROUND: ask = round_setup(); break;
            case WAIT_L1: resolve_level1(); break;
            case FOUNDERS: ask = pick_founders(); break;
            case WAIT_L2: resolve_level2(); break;
            }
            if (ask) { *out = &rq; return true; }
        }
        return false;
    }

    rattle_cluster_set *flatten() const {
        rattle_cluster_set *R = new_cluster_set();
        if (report) {
            cluster_box *B = cluster_box_of(R);
            B->joins = new std::vector<cluster_join>(joins);
            B->has_report = true;
        }
        size_t nm = 0;
        for (auto &c : clusters) nm += c.seqs.size();
        R->n_clusters = (uint32_t)clusters.size();
        R->main_id = (int32_t *)malloc(sizeof(int32_t) * std::max<size_t>(1, clusters.size()));
        R->main_rev = (uint8_t *)malloc(std::max<size_t>(1, clusters.size()));
        R->offsets = (uint32_t *)malloc(sizeof(uint32_t) * (clusters.size() + 1));
        R->member_id = (int32_t *)malloc(sizeof(int32_t) * std::max<size_t>(1, nm));
        R->member_rev = (uint8_t *)malloc(std::max<size_t>(1, nm));
        uint32_t p = 0;
        for (size_t c = 0; c < clusters.size(); ++c) {
            R->main_id[c] = clusters[c].main.id;
            R->main_rev[c] = clusters[c].main.rev;
            R->offsets[c] = p;
            for (auto &s : clusters[c].seqs) { R->member_id[p] = s.id; R->member_rev[p] = s.rev; ++p; }
        }
        R->offsets[clusters.size()] = p;
        memcpy(R->counters, counters, sizeof(counters));
        return R;
    }
};

// all jobs in lockstep: every turn, the rectangles the unfinished jobs wait for are evaluated together
int run_jobs(rattle_ctx *ctx, const rattle_cluster_params *P, std::vector<job> &jobs, bool shard_level2) {
    evaluator E{ctx, P};
    std::vector<uint32_t> active(jobs.size());
    for (uint32_t i = 0; i < jobs.size(); ++i) { active[i] = i; jobs[i].inner_parallel = jobs.size() == 1; jobs[i].report = ctx->cluster_report; jobs[i].start(); }
    std::vector<request *> want, reqs;
    static const bool timing = getenv("RATTLE_TIMING") != nullptr;
    double t_steps = 0;
    while (!active.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        want.assign(active.size(), nullptr);
        parallel_for(active.size(), active.size() > 64 ? 16 : 1, [&](size_t i) {        // a step is microseconds of host work
            request *q = nullptr;
            if (jobs[active[i]].step(&q)) want[i] = q;
        });
        reqs.clear();
        std::vector<uint32_t> still;
        for (size_t i = 0; i < active.size(); ++i) if (want[i]) { reqs.push_back(want[i]); still.push_back(active[i]); }
        active.swap(still);
        t_steps += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (reqs.empty()) break;
        RT_TRY(E.run(reqs, shard_level2 && jobs.size() == 1 && !reqs[0]->triangular));
    }
    if (!jobs.empty()) jobs[0].counters[4] += E.launches;
    if (timing && jobs.size() == 1)
        fprintf(stderr, "[rattle]   host steps: round set-up %.1f, level-1 resolve %.1f, founders + request %.1f, level-2 resolve %.1f, end of pass %.1f ms\n",
                jobs[0].t_phase[0], jobs[0].t_phase[1], jobs[0].t_phase[2], jobs[0].t_phase[3], jobs[0].t_phase[4]);
    if (timing)
        fprintf(stderr, "[rattle]   %zu job(s): host steps %.1f ms | build+upload %.1f, filter %.1f, count pass %.1f, host bound test %.1f, full pass + verdicts %.1f ms\n",
                jobs.size(), t_steps, E.t_split[0], E.t_split[1], E.t_split[2], E.t_split[3], E.t_split[4]);
    if (timing)
        fprintf(stderr, "[rattle]   count pass of the evaluations with survivors: seed %llu, search %llu, index %llu\n",
                (unsigned long long)E.n_form[0], (unsigned long long)E.n_form[1], (unsigned long long)E.n_form[2]);
    return 0;
}

}  // namespace

int cluster_driver(rattle_ctx *ctx, const rattle_cluster_params *P, const uint32_t *subset, uint32_t n_subset,
                   rattle_cluster_set **out) {
    std::vector<job> jobs(1);
    jobs[0].X = &ctx->idx; jobs[0].P = P; jobs[0].subset = subset;
    jobs[0].n = subset ? n_subset : ctx->idx.n;
    RT_TRY(run_jobs(ctx, P, jobs, true));
    *out = jobs[0].flatten();
    return 0;
}

// subsets which[0..n_which) of (ids, sub_off), clustered independently and in lockstep; outs[which[i]] receives the result
int cluster_driver_many(rattle_ctx *ctx, const rattle_cluster_params *P, const uint32_t *ids, const uint64_t *sub_off,
                        const uint32_t *which, uint32_t n_which, rattle_cluster_set **outs) {
    static const uint32_t none = 0;
    std::vector<job> jobs(n_which);
    for (uint32_t i = 0; i < n_which; ++i) {
        const uint32_t g = which[i];
        jobs[i].X = &ctx->idx; jobs[i].P = P;
        jobs[i].n = (uint32_t)(sub_off[g + 1] - sub_off[g]);
        jobs[i].subset = jobs[i].n ? ids + sub_off[g] : &none;
    }
    RT_TRY(run_jobs(ctx, P, jobs, false));
    for (uint32_t i = 0; i < n_which; ++i) outs[which[i]] = jobs[i].flatten();
    return 0;
}

// cluster_driver_many as one job over the ranks of the context: the subsets (gene clusters, main.cpp:281-318) are independent -> LPT
// over ranks by the pair count proxy n^2, every rank clusters its own, largest first, and the sets are all-gathered at the end
// (wire.h: the cluster sets).  All ranks take part in the exchange even after a local failure, which their piece then announces.
// Every outs[i] is a set on return, or on error none is.
int cluster_subsets_ranked(rattle_ctx *ctx, const rattle_cluster_params *P, const uint32_t *ids, const uint64_t *sub_off, uint32_t n_subsets,
                           rattle_cluster_set **outs) {
    const int R = ctx->xchg.nranks, rk = ctx->xchg.rank;
    std::vector<uint32_t> owner(n_subsets, 0);
    if (R > 1) {
        std::vector<uint64_t> cost(n_subsets);
        for (uint32_t i = 0; i < n_subsets; ++i) { const uint64_t n = sub_off[i + 1] - sub_off[i]; cost[i] = n * n; }
        lpt_assign(cost, R, owner);
    }
    std::vector<uint32_t> order;                                  // my subsets, largest first
    for (uint32_t i = 0; i < n_subsets; ++i) if ((int)owner[i] == rk) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t la = sub_off[a + 1] - sub_off[a], lb = sub_off[b + 1] - sub_off[b];
        return la != lb ? la > lb : a < b;
    });
    auto give_up = [&](int rc) {
        for (uint32_t i = 0; i < n_subsets; ++i) { rattle_hip_cluster_set_free(outs[i]); outs[i] = nullptr; }
        return rc;
    };
    int rc = cluster_driver_many(ctx, P, ids, sub_off, order.data(), (uint32_t)order.size(), outs);
    if (R == 1) return rc ? give_up(rc) : 0;
    const std::string local_msg = rc ? rattle_hip_last_error() : "";
    std::vector<uint8_t> mine;
    if (rc == 0) for (uint32_t i : order) write_cluster_set(mine, i, *outs[i]);
    else write_cluster_sets_failure(mine);
    std::vector<std::vector<uint8_t>> all;
    const int xrc = xchg_allgatherv(ctx, mine, all);
    if (rc) { set_error(local_msg); return give_up(rc); }
    if (xrc) return give_up(xrc);
    std::vector<uint8_t> seen(n_subsets, 0);
    std::vector<cluster_set_view> sets;
    for (int r = 0; r < R; ++r) {
        if (r == rk) continue;
        const std::vector<uint8_t> &b = all[(size_t)r];
        if (is_cluster_sets_failure(b.data(), b.size())) { set_error("cluster_subsets failed on rank " + std::to_string(r)); return give_up(RATTLE_ERR_HIP); }
        wire_reader W(b.data(), b.size());
        sets.clear();
        if (!parse_cluster_sets(W, n_subsets, sub_off, owner.data(), (uint32_t)r, seen, sets)) { set_error(wire_error("cluster_subsets exchange", r, W)); return give_up(RATTLE_ERR_HIP); }
        for (const cluster_set_view &V : sets) {
            rattle_cluster_set *cs = new_cluster_set();
            const size_t nc = V.n_clusters, nm = V.n_members;
            cs->n_clusters = V.n_clusters;
            memcpy(cs->counters, V.counters, sizeof(V.counters));
            cs->main_id = (int32_t *)malloc(std::max<size_t>(1, nc) * 4); cs->offsets = (uint32_t *)malloc((nc + 1) * 4);
            cs->member_id = (int32_t *)malloc(std::max<size_t>(1, nm) * 4);
            cs->main_rev = (uint8_t *)malloc(std::max<size_t>(1, nc)); cs->member_rev = (uint8_t *)malloc(std::max<size_t>(1, nm));
            memcpy(cs->offsets, V.offsets, (nc + 1) * 4);
            if (nc) { memcpy(cs->main_id, V.main_id, nc * 4); memcpy(cs->main_rev, V.main_rev, nc); }
            if (nm) { memcpy(cs->member_id, V.member_id, nm * 4); memcpy(cs->member_rev, V.member_rev, nm); }
            outs[V.subset] = cs;
        }
    }
    // (every piece held exactly its rank's subsets, so with this rank's own every subset is here once)
    for (uint32_t i = 0; i < n_subsets; ++i) if (!outs[i]) { set_error("cluster_subsets exchange: subset " + std::to_string(i) + " never arrived"); return give_up(RATTLE_ERR_HIP); }
    return 0;
}

// Test hook: ONE evaluation of the given rectangles as a greedy step makes it (evaluator::run, unsharded), with the count pass
// chosen by the caller, and what it computed on the way.
int debug_evaluate(rattle_ctx *ctx, const rattle_cluster_params *P, int count_mode, const rattle_debug_rect *R, uint32_t n_rects,
                   rattle_debug_eval **out) {
    std::vector<request> q(n_rects);
    std::vector<uint64_t> counters((size_t)n_rects * 8 + 1, 0);
    std::vector<request *> reqs(n_rects);
    for (uint32_t r = 0; r < n_rects; ++r) {
        q[r].seeds.assign(R[r].seed_ids, R[r].seed_ids + R[r].n_seeds);
        if (!R[r].triangular) q[r].cands.assign(R[r].cand_ids, R[r].cand_ids + R[r].n_cands);
        q[r].triangular = R[r].triangular != 0;
        q[r].thr = R[r].thr;
        q[r].counters = counters.data() + 8 * (size_t)r;
        q[r].tag = r;
        reqs[r] = &q[r];
    }
    evaluator E{ctx, P};
    eval_sink sink;
    E.count_mode = count_mode;
    E.sink = &sink;
    RT_TRY(E.run(reqs, false));
    size_t nh = 0;
    for (auto &x : q) nh += x.hits.size();
    rattle_debug_eval *D = (rattle_debug_eval *)calloc(1, sizeof(rattle_debug_eval));
    auto fill = [](rattle_debug_pairs &d, size_t n) {
        d.n = (uint32_t)n;
        d.rect = (uint32_t *)malloc(4 * std::max<size_t>(n, 1)); d.seed = (uint32_t *)malloc(4 * std::max<size_t>(n, 1));
        d.cand = (uint32_t *)malloc(4 * std::max<size_t>(n, 1)); d.strand = (uint8_t *)malloc(std::max<size_t>(n, 1));
        d.count = (int32_t *)malloc(4 * std::max<size_t>(n, 1));
    };
    fill(D->survivors, sink.surv.size()); fill(D->kept, sink.kept.size()); fill(D->hits, nh);
    auto put = [](rattle_debug_pairs &d, size_t i, const eval_sink::pair &p) {
        d.rect[i] = p.rect; d.seed[i] = p.seed; d.cand[i] = p.cand; d.strand[i] = p.strand; d.count[i] = p.count;
    };
    for (size_t i = 0; i < sink.surv.size(); ++i) put(D->survivors, i, sink.surv[i]);
    for (size_t i = 0; i < sink.kept.size(); ++i) put(D->kept, i, sink.kept[i]);
    size_t h = 0;
    for (uint32_t r = 0; r < n_rects; ++r)
        for (const hit_t &x : q[r].hits) put(D->hits, h++, eval_sink::pair{r, x.seed, x.cand, x.rev, 0});
    if (ctx->cluster_report) {
        D->hit_bases = (int32_t *)malloc(4 * std::max<size_t>(nh, 1)); D->hit_hc_bases = (int32_t *)malloc(4 * std::max<size_t>(nh, 1));
        D->hit_variance = (double *)malloc(8 * std::max<size_t>(nh, 1));
        h = 0;
        for (uint32_t r = 0; r < n_rects; ++r)
            for (const hit_evidence &e : q[r].ev) { D->hit_bases[h] = e.bases; D->hit_hc_bases[h] = e.hc; D->hit_variance[h] = e.var; ++h; }
    }
    D->counters = (uint64_t *)malloc(counters.size() * 8);
    memcpy(D->counters, counters.data(), counters.size() * 8);
    D->count_pass = sink.count_pass;
    D->filter_launches = sink.filter_launches;
    D->oversize_pairs = sink.oversize;
    *out = D;
    return 0;
}

// `assign`: the loaded reads read_ids against the loaded reads target_ids, the targets as seeds in batches against all the reads, every
// batch one evaluation that ends in the per-read reduction; the batches' states are folded on the device in target order and the
// call's state -- 40 bytes per read -- is the only thing copied back.  With C the batches also leave their k best targets per read
// (assign.hip, the candidate list), folded in the same way: 4 + 28 k bytes per read more, in both states and on the way back.
int assign_driver(rattle_ctx *ctx, const rattle_assign_params *AP, const uint32_t *tids, uint32_t nt, const uint32_t *rids, uint32_t nr,
                  rattle_assignment *A, uint32_t out_base, rattle_candidates *C) {
    if (nt == 0 || nr == 0) return 0;                    // (the records start out unassigned)
    hipStream_t st = ctx->stream;
    const read_index &X = ctx->idx;
    rattle_cluster_params CP;
    memset(&CP, 0, sizeof CP);
    CP.t_s = AP->t_s; CP.t_v = AP->t_v; CP.bv_threshold = AP->bv_threshold; CP.use_hc = AP->use_hc; CP.is_rna = AP->is_rna;
    assign_state batch, call;                            // allocated once per call, released when it returns
    RT_TRY(batch.reserve(nr)); RT_TRY(call.reserve(nr));
    RT_TRY(batch.clear(st, nr)); RT_TRY(call.clear(st, nr));
    const assign_dev B = batch.dev(), G = call.dev();
    top_state tbatch, tcall;
    if (C) {
        RT_TRY(tbatch.reserve(nr, C->k)); RT_TRY(tcall.reserve(nr, C->k));
        RT_TRY(tbatch.clear(st, nr)); RT_TRY(tcall.clear(st, nr));
    }
    const top_dev TB = tbatch.dev(), TG = tcall.dev();
    evaluator E{ctx, &CP};
    E.count_mode = AP->count_pass;
    E.best = &B;
    if (C) E.top = &TB;
    uint64_t counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    request rq;
    rq.cands.assign(rids, rids + nr);
    rq.thr = AP->bv_threshold; rq.counters = counters;
    // seeds x reads x strands below the evaluator's per-launch bounds even if every pair survives
    const uint32_t step = max_seeds_per_launch(AP->target_batch ? AP->target_batch : 512u, nr, X.both ? 2u : 1u, rq.thr);
    std::vector<request *> reqs{&rq};
    for (uint32_t t0 = 0; t0 < nt; t0 += step) {
        rq.seeds.assign(tids + t0, tids + std::min<uint64_t>(nt, (uint64_t)t0 + step));
        E.best_base = t0;
        RT_TRY(E.run_chunks(reqs));
        RT_TRY(launch_assign_merge(ctx, nr, B, G));
        if (C) RT_TRY(launch_assign_top_merge(ctx, nr, TB, TG));
    }
    std::vector<unsigned long long> best(nr), second(nr);
    std::vector<uint32_t> key(nr), n(nr);
    std::vector<hit_evidence> ev(nr);
    static_assert(sizeof(hit_evidence) == sizeof(uint4), "the evidence record is one 16-byte store");
    RT_HIP(hipMemcpyAsync(best.data(), G.best, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(second.data(), G.second, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(key.data(), G.key, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(n.data(), G.n, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(ev.data(), G.ev, (size_t)nr * sizeof(uint4), hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    ctx->stats[K_ASSIGN].bytes += 40ull * nr;
    auto score_of = [](unsigned long long pat) { double d; const unsigned long long b = pat - 1; memcpy(&d, &b, 8); return d; };
    for (uint32_t r = 0; r < nr; ++r) {
        if (best[r] == 0) continue;
        const size_t o = (size_t)out_base + r;
        const uint32_t t = key[r] >> 1;
        if (t >= nt) { set_error("assign: a winner outside the targets"); return RATTLE_ERR_HIP; }
        const uint32_t li = X.h_len[tids[t]], lj = X.h_len[rids[r]];
        A->target[o] = (int32_t)t; A->rev[o] = (uint8_t)(key[r] & 1u);
        A->bases[o] = ev[r].bases; A->hc_bases[o] = ev[r].hc; A->variance[o] = ev[r].var;
        A->min_len[o] = li < lj ? li : lj;
        A->score[o] = score_of(best[r]);
        A->second_score[o] = second[r] ? score_of(second[r]) : -1.0;
        A->n_accepted[o] = n[r];
    }
    if (!C) return 0;
    const uint32_t k = C->k;
    std::vector<unsigned long long> pat((size_t)nr * k);
    std::vector<uint32_t> tkey((size_t)nr * k), cnt(nr);
    std::vector<hit_evidence> tev((size_t)nr * k);
    RT_HIP(hipMemcpyAsync(pat.data(), TG.pat, pat.size() * 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(tkey.data(), TG.key, tkey.size() * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(tev.data(), TG.ev, tev.size() * sizeof(uint4), hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(cnt.data(), TG.cnt, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    ctx->stats[K_ASSIGN].bytes += (4ull + 28ull * k) * nr;
    for (uint32_t r = 0; r < nr; ++r) {
        if (cnt[r] > k) { set_error("assign: more candidates than slots"); return RATTLE_ERR_HIP; }
        C->count[(size_t)out_base + r] = cnt[r];
        for (uint32_t j = 0; j < cnt[r]; ++j) {
            const size_t s = (size_t)r * k + j, o = ((size_t)out_base + r) * k + j;
            const uint32_t t = tkey[s] >> 1;
            if (pat[s] == 0 || t >= nt) { set_error("assign: a candidate outside the targets"); return RATTLE_ERR_HIP; }
            const uint32_t li = X.h_len[tids[t]], lj = X.h_len[rids[r]];
            C->target[o] = (int32_t)t; C->rev[o] = (uint8_t)(tkey[s] & 1u);
            C->bases[o] = tev[s].bases; C->hc_bases[o] = tev[s].hc; C->variance[o] = tev[s].var;
            C->min_len[o] = li < lj ? li : lj;
            C->score[o] = score_of(pat[s]);
        }
    }
    return 0;
}

}  // namespace rattle
