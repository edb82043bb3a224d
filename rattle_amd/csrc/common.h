// Internal declarations shared by the HIP translation units of librattle_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rattle_hip.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace rattle {

// RATTLE_TIMING=1: wall-clock of host phases on stderr
struct phase_timer {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    bool on;
    double *keep = nullptr;             // where the elapsed milliseconds are ADDED when the timer stops (rattle_hip_stage_ms), with or without RATTLE_TIMING
    explicit phase_timer(const char *n, double *k = nullptr) : name(n), t0(std::chrono::steady_clock::now()), keep(k) {
        static const bool enabled = getenv("RATTLE_TIMING") != nullptr;
        on = enabled;
    }
    void stop() {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (keep) { *keep += ms; keep = nullptr; }
        if (on) fprintf(stderr, "[rattle] %-28s %8.1f ms\n", name, ms);
        on = false;
    }
    ~phase_timer() { stop(); }
};

void set_error(const std::string &msg);

// Host-side data-parallel loop (post-MSA logic, packing, row expansion): dynamic chunks of one item.
template <typename F>
void parallel_for(size_t n, int n_threads, F f) {
    if (n == 0) return;
    // default width: RATTLE_HOST_THREADS, else all cores (several ranks on one host should split them)
    static const unsigned env_threads = getenv("RATTLE_HOST_THREADS") ? (unsigned)atoi(getenv("RATTLE_HOST_THREADS")) : 0u;
    unsigned hw = env_threads ? env_threads : std::thread::hardware_concurrency();
    size_t T = n_threads > 0 ? (size_t)n_threads : (hw ? hw : 1);
    T = std::min(T, n);
    if (T <= 1) { for (size_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<size_t> next(0);
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&]() { for (size_t i = next++; i < n; i = next++) f(i); });
    for (auto &x : th) x.join();
}

#define RT_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess) {                                                                       \
            ::rattle::set_error(std::string(#call) + ": " + hipGetErrorString(e__) + " (" + __FILE__ + \
                                ":" + std::to_string(__LINE__) + ")");                                 \
            return RATTLE_ERR_HIP;                                                                     \
        }                                                                                              \
    } while (0)

#define RT_TRY(call)            \
    do {                        \
        int r__ = (call);       \
        if (r__ != 0) return r__; \
    } while (0)

// Growable device buffer (never shrinks; contents are not preserved across grow()).  Owns its
// allocation and frees it on destruction, so early error returns do not leak HBM; borrow() makes a
// non-owning view of another buffer (the child contexts of cluster_subsets share the parent's index).
void dev_free(void *p);

template <typename T>
struct dbuf {
    T *p = nullptr;
    size_t cap = 0;
    bool owned = true;
    dbuf() = default;
    dbuf(const dbuf &) = delete;
    dbuf &operator=(const dbuf &) = delete;
    ~dbuf() { release(); }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        release();
        size_t want = n + n / 4 + 64;
        RT_HIP(hipMalloc((void **)&p, want * sizeof(T)));
        cap = want;
        return 0;
    }
    void borrow(const dbuf &o) {
        release();
        p = o.p; cap = o.cap; owned = false;
    }
    void swap(dbuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(owned, o.owned); }
    void release() {
        if (p && owned) dev_free(p);
        p = nullptr;
        cap = 0;
        owned = true;
    }
};

// Pinned host buffer for D2H results.
template <typename T>
struct hbuf {
    T *p = nullptr;
    size_t cap = 0;
    hbuf() = default;
    hbuf(const hbuf &) = delete;
    hbuf &operator=(const hbuf &) = delete;
    ~hbuf() { release(); }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        release();
        size_t want = n + n / 4 + 64;
        RT_HIP(hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

enum { K_KMER = 0, K_FILTER = 1, K_SCORE = 2, K_POA = 3, K_POST = 4, K_ASSIGN = 5, K_ALIGN = 6, K_CIGAR = 7, K_ALIGN_AFFINE = 8, K_CIGAR_AFFINE = 9, K_ABUNDANCE = 10, K_PILEUP = 11, K_COUNT = 12 };

struct kstat {
    double ms = 0;
    uint64_t launches = 0, bytes = 0;
};

// Device-resident read index (output of kernel K).
struct read_index {
    uint32_t n = 0;
    int k = 0;
    int both = 0;
    uint64_t total_bases = 0, total_kmers = 0;
    std::vector<uint64_t> h_off;      // [n+1] base offsets
    std::vector<uint64_t> h_koff;     // [n+1] k-mer list offsets (entries)
    std::vector<uint32_t> h_len;      // [n]
    dbuf<uint8_t> seq;                // ASCII bases
    dbuf<uint64_t> off, koff;         // device copies
    dbuf<uint32_t> len;
    dbuf<uint32_t> uh;                // forward hashes in POSITION order          [total_kmers]
    dbuf<uint32_t> kh[2];             // hashes sorted by (hash,pos), per strand     [total_kmers]
    dbuf<uint32_t> kp[2];             // positions in that order                     [total_kmers]
    dbuf<uint64_t> bv[2];             // bit-vectors, 64 words per read              [n*64]
    dbuf<uint32_t> pc[2];             // popcount of each bit-vector                 [n]
};

// phred_symbol(p) = (char)(-10*log10(p)+33) as a table of thresholds built with the host libm (post_msa.hip)
struct phred_table {
    int n0 = 0;
    std::vector<double> lo;             // lo[t]: smallest p whose symbol value is <= n0 + t
    std::vector<uint64_t> exc_bits;     // doubles (bit patterns, sorted) the table would get wrong
    std::vector<int32_t> exc_val;
};
void build_phred_table(phred_table &T);
int phred_lookup_host(const phred_table &T, double p);

// ---- one job over several GPUs (exchange.hip) ----------------------------------------------------------
// The path shards by independent objects: candidate reads of a seed batch, --iso gene clusters,
// `correct` packs.  A context may be one rank of nranks; the only data-path communication is an
// all-gather(v) of small byte strings (hit lists, cluster sets, pack consensi) plus the final gather of
// the corrected reads.  Two transports: RCCL on device buffers (rattle_hip_comm_init) or a caller-supplied
// host-buffer all-gather (rattle_hip_set_exchange: MPI, gloo, tests).
struct exchange {
    int rank = 0, nranks = 1;
    rattle_allgatherv_fn fn = nullptr;
    void *user = nullptr;
    void *comm = nullptr;               // ncclComm_t
    void *rccl = nullptr;               // dlopen handle of librccl.so
    uint64_t calls = 0, bytes = 0;      // statistics
    // Measurement aid (round 5: the multi-GPU curve measured on ONE GPU, tools/rank_replay.py): what the ranks of a job exchange is
    // recorded by a single-rank run (RATTLE_XCHG_RECORD=<file>: every exchange point appends the job's WHOLE payload), and a context
    // configured as rank r of R with rattle_hip_set_exchange(.., fn = NULL) under RATTLE_XCHG_REPLAY=<file> then runs its own share
    // alone: at every exchange it gets its own piece back plus the recorded whole (its peers' part of it).
    FILE *replay = nullptr;
    std::string replay_path;            // ... the file `replay` was opened from (the gather's piece files live beside it)
    // staging of the RCCL all-gather-v, kept between calls: the sharded cluster driver exchanges a few KB per greedy round
    // (119 rounds at 1e6 reads) and three hipMalloc / hipFree pairs per exchange were three device-wide synchronisations each
    dbuf<uint64_t> d_sz;
    dbuf<uint8_t> d_send, d_recv;
    hbuf<uint64_t> h_sz;
    hbuf<uint8_t> h_send, h_recv;       // pinned: the copies are asynchronous and run at link speed
    void reset() {
        rank = 0; nranks = 1; fn = nullptr; user = nullptr; comm = nullptr; calls = 0; bytes = 0;      // the loader's handle (rccl) stays
        if (replay) { fclose(replay); replay = nullptr; }
        replay_path.clear();
        d_sz.release(); d_send.release(); d_recv.release(); h_sz.release(); h_send.release(); h_recv.release();
    }
};

// `correct` work list: the packs of correct.cpp:328-370 from ids and lengths only, plus the static
// assignment of packs to ranks (LPT by the DP cost proxy L_0 * sum L_j).  Pure host code.
struct sref { int32_t rid; uint8_t rev; };
struct pack_plan {
    std::vector<sref> members;          // members of all queued packs, pack after pack
    std::vector<uint32_t> first;        // [n_packs+1] into members
    std::vector<int32_t> pk_cid;        // cluster of each pack
    std::vector<uint32_t> pk_local;     // index among its cluster's queued packs
    std::vector<uint64_t> pk_cost;
    std::vector<uint32_t> pk_owner;     // rank
    std::vector<uint32_t> cl_p0, cl_np; // per cluster: first pack, number of packs
    std::vector<sref> small;            // members of packs that are never queued, in the reference's order
    std::vector<int32_t> small_cid;
    std::vector<uint8_t> small_why;     // 0: <= min_reads (correct.cpp:360), 1: max_pack_cells rule
    std::vector<uint32_t> small_pack;   // local pack index within the cluster
};
int plan_packs(const uint64_t *off, uint32_t n_reads, uint32_t n_clusters, const uint32_t *coff, const int32_t *mid, const uint8_t *mrev,
               const rattle_correct_params *P, int nranks, pack_plan &out);
// a read set of the result for n records and tot bases (NUL behind them); the arrays are never null pointers (exchange.hip)
void alloc_read_set(rattle_read_set &S, uint32_t n, uint64_t tot);
// longest-processing-time-first assignment of weighted items to nranks bins (ties: lower index / lower rank)
void lpt_assign(const std::vector<uint64_t> &cost, int nranks, std::vector<uint32_t> &owner);
// all-gather of one byte string per rank (sizes first, then the payload)
bool xchg_recording(const rattle_ctx *ctx);
bool xchg_replaying(const rattle_ctx *ctx);
// job_payload = false: a transport self-test (rattle_hip_comm_probe), kept out of the record / replay aid
int xchg_allgatherv(rattle_ctx *ctx, const std::vector<uint8_t> &mine, std::vector<std::vector<uint8_t>> &all, bool job_payload = true);

// one rectangle of kernel A's launch: seeds [s_base, s_base+ns) x candidates [c_base, c_base+nc) of the uploaded
// arrays, tiles [tile_base, ...), look-up table row at d_lut + lut_off
struct bvf_rect {
    uint32_t s_base, ns, c_base, nc, tile_base, lut_off, fwd_bypass, pad;
};

// copy descriptor of the gather kernel: flags bit 0 = reverse complement (qualities reversed)
struct gather_desc {
    uint64_t src, dst;
    uint32_t len, flags;
};

// arguments of the post-MSA kernel (post_msa.hip)
struct post_args {
    const uint8_t *seq, *qual;          // stage input, concatenated (qual: MODE 1 only)
    const uint64_t *off;                // per sequence
    const uint32_t *pack_first;         // per pack
    const uint32_t *col, *width;        // kernel C output: column per base, width per pack
    const uint64_t *moff;               // per pack: byte offset of its rows x width matrix (16-byte aligned)
    const uint64_t *coff;               // per pack: offset of its per-column arrays
    uint8_t *rowc, *rowq;               // matrices: bases / quality bytes; MODE 1 leaves the corrected read at each row start
    int32_t *rfirst, *rlast;            // per sequence: voting window after fix_msa_ends
    uint32_t *tfront, *tback;           // per sequence: bases trimmed by fix_msa_ends (MODE 1)
    uint32_t *olen;                     // per sequence: corrected length (MODE 1)
    uint8_t *ccons, *cflag, *csym;      // per column: winner, occupancy tests, quality symbol of the winner's mean error
    double *cerr;                       // per column: winner's mean error
    uint8_t *cons_out;                  // per pack (at coff): gap-stripped consensus (MODE 2)
    uint32_t *cons_len;
    const double *perr;                 // [256] phred_err per quality byte (utils.cpp:10-13), host computed
    const double *phred_lo;
    const unsigned long long *exc_bits;
    const int32_t *exc_val;
    int32_t phred_n0, phred_cnt;
    uint32_t n_exc;
    uint8_t order[8];                   // vote slot order
    double min_occ, gap_occ, err_ratio;
    uint32_t *rep;                      // report form of MODE 1 (else null): REP_KERNEL counters per sequence, counter f of sequence q at rep[f * rep_stride + q]
    uint32_t rep_stride;
    // report form of MODE 2, the consensus support (else ccnt is null).  Four uint32 per column, field f of column k of pack p at
    // ccnt[f * cnt_stride + coff[p] + k]: support, depth (reads), the vote's winner count and total (rows); ocnt: the same for the bases
    // of the consensus, at their index in cons_out.  Packs [0, n_composed) are POA #3 packs: in_sup / in_dep hold the support and the
    // depth of every input base (parallel to seq; the composed packs' sequences come first), msup / mdep are rows x width matrices of
    // them at moff (uint32 per cell, only for those packs)
    uint32_t *ccnt, *ocnt;
    uint64_t cnt_stride;
    uint32_t n_composed;
    const uint32_t *in_sup, *in_dep;
    uint32_t *msup, *mdep;
};

// The per-read correction report.  Kernel D's report form counts, per row, the columns of its window by the branch of step d that
// handled them (REP_MATCH ..., REP_KERNEL counters in that order); the driver puts the lengths and the trim counts in front.
enum { REP_IN = 0, REP_OUT, REP_TFRONT, REP_TBACK, REP_MATCH, REP_SUBST, REP_MISKEPT, REP_INS, REP_DEL, REP_GAPKEPT, REP_FIELDS, REP_KERNEL = 6 };
extern const char *const rep_names[REP_FIELDS];
// A rattle_correction the library hands out is the head of this box: the report lies behind the public struct, where no caller's
// layout sees it.  The library keeps a list of the boxes it made, so a rattle_correction a caller built itself is told apart (box_of
// returns null for it) and nothing behind it is read.
struct correction_box {
    rattle_correction pub;
    bool has_report;
    uint32_t *rep[REP_FIELDS];          // [pub.corrected.n] each, parallel to pub.corrected.read_id
    // the consensus support (rattle_hip_set_consensus_support): per base of pub.consensi (at pub.consensi.off) support, depth, pack_support,
    // pack_depth; per record the level (2: one pack's POA #2 vote, 3: composed through POA #3)
    bool has_support;
    uint8_t *sup_level;
    uint32_t *sup[4];
};
enum { SUP_SUPPORT = 0, SUP_DEPTH, SUP_PACK_SUPPORT, SUP_PACK_DEPTH, SUP_FIELDS };
rattle_correction *new_correction();
correction_box *box_of(const rattle_correction *c);
void alloc_report(correction_box *B, size_t n);                      // the arrays (never null pointers), has_report = true
void alloc_support(correction_box *B, size_t n, size_t bases);       // level per record, four arrays per base (zeroed), has_support = true
void print_support_totals(const rattle_correction *c);               // RATTLE_TIMING=1: the totals of the consensus support on stderr
void print_report_totals(const rattle_correction *c, const char *what);      // RATTLE_TIMING=1: the six totals on stderr

// The cluster report.  The verdict kernel's report form writes an evidence record (hit_evidence) beside every accepted pair; the greedy
// driver keeps the record of the hit that decided each absorption and emits one join per absorbed item at the end of a pass.
struct hit_evidence { int32_t bases, hc; double var; };      // 16 bytes, the layout the kernel writes
struct cluster_join {
    uint32_t pass;                      // 0: the initial pass, 1 ..: the merge passes
    double thr;                         // bit-vector threshold of the pass
    int32_t into, absorbed;             // ids in the id space of the set's member_id
    uint8_t rev, level;
    int32_t bases, hc;
    uint32_t min_len;
    double score, variance;
};
// A rattle_cluster_set the library hands out is the head of this box, as a rattle_correction is the head of a correction_box: the joins
// lie behind the public struct, and the library's list of its boxes tells a set a caller built itself apart (cluster_box_of: null).
struct cluster_box {
    rattle_cluster_set pub;
    bool has_report;
    std::vector<cluster_join> *joins;   // owned; null without a report
};
rattle_cluster_set *new_cluster_set();
cluster_box *cluster_box_of(const rattle_cluster_set *cs);

// `assign` (assign.hip): the reduction's state per read, as the kernels see it and as its owner holds it.  best / second: bit pattern of
// a score + 1 (0: none); key: target index << 1 | strand of the winner (0xFFFFFFFF: none); n: accepted comparisons; ev: the winner's
// bases, hc_bases and the variance's 64 bits.  40 bytes per read.
struct assign_dev { unsigned long long *best, *second; uint32_t *key, *n; uint4 *ev; };
struct assign_state {
    dbuf<unsigned long long> best, second;
    dbuf<uint32_t> key, n;
    dbuf<uint4> ev;
    int reserve(size_t nr);
    int clear(hipStream_t st, size_t nr);
    assign_dev dev() const { return assign_dev{best.p, second.p, key.p, n.p, ev.p}; }
};
// The candidate list (`assign_*_top`): k slots per read, slot r * k + j the read's j-th best target.  pat: bit pattern of the slot's
// score + 1 (0: unused; a read's slots are filled from 0 without a hole); key: target index << 1 | strand (0xFFFFFFFF: unused); ev: as
// assign_dev::ev; cnt: filled slots (kept by the merge in the call's state only).  28 bytes per slot, 4 per read.
struct top_dev { unsigned long long *pat; uint32_t *key; uint4 *ev; uint32_t *cnt; uint32_t k; };
struct top_state {
    dbuf<unsigned long long> pat;
    dbuf<uint32_t> key, cnt;
    dbuf<uint4> ev;
    uint32_t k = 0;
    int reserve(size_t nr, uint32_t k_);
    int clear(hipStream_t st, size_t nr);
    top_dev dev() const { return top_dev{pat.p, key.p, ev.p, cnt.p, k}; }
};

int hw_queues();      // hardware queues the HIP runtime of this process hands out (settled when the library is loaded, abi.hip)

}  // namespace rattle

struct rattle_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing = true;
    rattle::kstat stats[rattle::K_COUNT];
    rattle::read_index idx;
    // scratch for the filter / score kernels
    rattle::dbuf<uint32_t> d_seed, d_cand, d_first;
    rattle::dbuf<rattle::bvf_rect> d_rect;
    rattle::dbuf<uint32_t> d_pi2, d_pj2, d_slot2, d_seed_rect;      // pairs past the count bound, compacted on the device
    rattle::dbuf<uint8_t> d_ps2;
    rattle::dbuf<unsigned long long> d_bound_stats;
    rattle::hbuf<unsigned long long> h_bound_stats;
    rattle::dbuf<uint16_t> d_lut;
    rattle::dbuf<uint8_t> d_pass;
    rattle::dbuf<uint32_t> d_surv;          // survivor list (2 words per entry)
    rattle::dbuf<uint32_t> d_surv2;         // ... sorted by seed (double buffer of the device sort)
    rattle::dbuf<uint8_t> d_sort_tmp;
    // the "index" count pass (pair_index.hip): survivor range per candidate slot, bucket offsets, bucket entries, scan totals
    rattle::dbuf<uint32_t> d_ix_coff, d_ix_boff, d_ix_ent, d_ix_bsum;
    rattle::dbuf<uint32_t> d_counter;
    rattle::dbuf<uint32_t> d_pi, d_pj;
    rattle::dbuf<uint8_t> d_ps;
    rattle::dbuf<int32_t> d_res;            // per pair: bases, hc, n_dist, n_matches
    rattle::dbuf<double> d_var;
    rattle::dbuf<uint32_t> d_scratch;       // global scratch for oversize pairs
    rattle::hbuf<uint32_t> h_surv;
    rattle::hbuf<uint32_t> h_counter;
    // the cluster report (rattle_hip_set_cluster_report; never allocated while it is off): the evidence record of every accepted pair,
    // parallel to the accepted pairs in d_surv / h_surv
    bool cluster_report = false;
    rattle::dbuf<rattle::hit_evidence> d_hit_ev;
    rattle::hbuf<rattle::hit_evidence> h_hit_ev;
    // POA arena: kept across stages and calls (allocating ~100 GB costs seconds)
    uint8_t *poa_arena = nullptr;
    size_t poa_arena_bytes = 0;
    hipStream_t poa_st[16] = {};     // one per column class: classes run concurrently
    double stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // host wall time of the last calls' stages, summed until read (rattle_hip_stage_ms): [0] cluster, [1] correct stage 1, [2] 2a, [3] 2b+3a, [4] 3b
    int poa_shallow_graphs = 0;      // hint of the caller for the next poa_device_run: near-identical sequences (POA #2 / #3), graphs that are almost chains
    hipEvent_t poa_ev[16] = {};
    hipEvent_t poa_go = nullptr;
    rattle::hbuf<uint32_t> h_poa_col;       // pinned staging for the per-base MSA columns
    // reads staged in HBM by rattle_hip_stage_reads (keys: the host buffers they were copied from)
    const uint8_t *staged_seq_key = nullptr, *staged_qual_key = nullptr;
    uint32_t staged_n = 0;
    uint64_t staged_total = 0;
    rattle::dbuf<uint8_t> d_staged_seq, d_staged_qual;
    // post-MSA kernel constants (built on first use)
    rattle::phred_table phred;
    rattle::dbuf<double> d_phred_lo, d_perr;
    rattle::dbuf<unsigned long long> d_exc_bits;
    rattle::dbuf<int32_t> d_exc_val;
    bool phred_ready = false;
    bool correction_report = false;         // rattle_hip_set_correction_report: stage 1 of `correct` launches kernel D's report form
    bool consensus_support = false;         // rattle_hip_set_consensus_support: the consensus stages launch kernel D's mode-2 report form
    rattle::exchange xchg;
    rattle_ctx() = default;
    rattle_ctx(const rattle_ctx &) = delete;
    rattle_ctx &operator=(const rattle_ctx &) = delete;
    // streams, events and the arena; the dbuf / hbuf members release themselves
    ~rattle_ctx() {
        if (device < 0) return;                 // host-only context: nothing on a device
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (poa_arena) (void)hipFree(poa_arena);
        for (int i = 0; i < 16; ++i) { if (poa_st[i]) (void)hipStreamDestroy(poa_st[i]); if (poa_ev[i]) (void)hipEventDestroy(poa_ev[i]); }
        if (poa_go) (void)hipEventDestroy(poa_go);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace rattle {

// Event-timed launch bracket: records into ctx->stats[which].
struct ktimer {
    rattle_ctx *c;
    int which;
    uint64_t bytes;
    ktimer(rattle_ctx *c_, int w, uint64_t b) : c(c_), which(w), bytes(b) {
        if (c->timing) (void)hipEventRecord(c->ev0, c->stream);
    }
    ~ktimer() {
        c->stats[which].launches++;
        c->stats[which].bytes += bytes;
        if (c->timing) {
            (void)hipEventRecord(c->ev1, c->stream);
            (void)hipEventSynchronize(c->ev1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
            c->stats[which].ms += ms;
        }
    }
};

// kmer_extract.hip
int build_index(rattle_ctx *ctx, const uint8_t *seq, const uint64_t *off, uint32_t n, int k, int both);
// bv_filter.hip : device-side seeds/cands already uploaded in ctx->d_seed/d_cand/d_first/d_lut.
// Writes dense pass bytes (if dense) and/or appends survivors (seed_slot<<1|strand, cand_slot).
int launch_bv_filter(rattle_ctx *ctx, uint32_t n_seeds, uint32_t n_cands, int fwd_bypass, bool dense, bool list,
                     uint32_t list_cap);
// the same over a list of rectangles already uploaded to ctx->d_rect (look-up table rows in ctx->d_lut)
int launch_bv_filter_rects(rattle_ctx *ctx, uint32_t n_rects, uint32_t n_tiles, uint64_t pairs, bool dense, bool list, uint32_t list_cap);
// pair_score.hip : pairs in ctx->d_pi/d_pj/d_ps; results in ctx->d_res (4 ints per pair) + ctx->d_var.
int launch_pair_score(rattle_ctx *ctx, uint32_t n_pairs);
// the pairs `slots` (host) whose match list did not fit LDS, again, their lists in a global slab sized for max_matches
int launch_pair_score_oversize(rattle_ctx *ctx, const std::vector<uint32_t> &slots, uint32_t max_matches);
// pair_count.hip : the count pass, seed-major (survivors sorted by seed, the seed's k-mer set as an LDS bit set)
int sort_survivors_by_seed(rattle_ctx *ctx, uint32_t n, uint64_t n_seeds);
int launch_pair_count_seed(rattle_ctx *ctx, uint32_t n_pairs);
// the same pairs, |common| only (d_res[pair]); see pair_score.hip
int launch_pair_count(rattle_ctx *ctx, uint32_t n_pairs);
// pair_index.hip : the count pass over an inverted k-mer index of the evaluation's seeds (survivors grouped by candidate)
int group_survivors_by_cand(rattle_ctx *ctx, uint32_t n, uint64_t n_cands);
int launch_pair_count_index(rattle_ctx *ctx, uint32_t n_pairs, const uint32_t *h_seed, uint32_t ns, uint32_t nc, bool many);
// assign.hip : the per-read reduction over the kept pairs of the evaluation in flight (ctx->d_res / d_var / d_pi / d_pj / d_slot2)
int launch_assign_max(rattle_ctx *ctx, uint32_t n, const uint32_t *d_remap, int use_hc, double t_s, double t_v, unsigned long long *d_out,
                      uint32_t *d_big, const assign_dev &B);
int launch_assign_pick(rattle_ctx *ctx, uint32_t n, int use_hc, double t_s, double t_v, uint32_t target_base, const assign_dev &B);
int launch_assign_merge(rattle_ctx *ctx, uint32_t nr, const assign_dev &B, const assign_dev &G);
// the candidate list of the batch: slots 0 .. T.k - 1 of every read over the same n kept pairs, after launch_assign_pick and before
// launch_assign_merge (it reads B); then the batch's slots TB folded into the call's TG, TB left cleared
int launch_assign_top(rattle_ctx *ctx, uint32_t n, uint32_t nr, int use_hc, double t_s, double t_v, uint32_t target_base, const assign_dev &B,
                      const top_dev &T);
int launch_assign_top_merge(rattle_ctx *ctx, uint32_t nr, const top_dev &TB, const top_dev &TG);
// poa.hip : the words of kernel C's counter block (poa_args::counters, POA_CNT_WORDS on the device); poa_device_run hands the first
// POA_CNT_PUBLIC of them back in h_cnt.  The only place that says which slot is what.  The measurement builds reuse slots by number:
// POA_PREDSTAT 4 .. 6, POA_PROFILE 2 and 4 .. 7, POA_BARPROF 8 .. 15 (and POA_CNT_BARPROF ..), POA_HIST 16 + d and 80 + d.
enum poa_counter {
    POA_CNT_CELLS = 0,         // DP cells of the reference's work (counted once, by the pass that finishes the pack)
    POA_CNT_SEQS = 1,          // sequences aligned
    POA_CNT_NODES = 2,         // graph nodes of the finished packs
    POA_CNT_ROWS = 3,          // DP rows
    POA_CNT_SYNC = 8,          // 8 .. 10: the wait a wavefront of the team kernels gave up (POA_ERR_SYNC): who and where; saw | wants; rows | columns
    POA_CNT_STRIPS = 10,       // alignments over the full rows as strips (PK 8).  Collides with the third word of POA_CNT_SYNC: a strip count
                               // and a sync diagnosis of the same call overwrite / add to each other (known; moving it changes behaviour)
    POA_CNT_CELLS_DONE = 11,   // DP cells the device computed (every pass)
    POA_CNT_BAND_OK = 12,      // alignments with a certified band
    POA_CNT_BAND_FAIL = 13,    // ... with a failed certificate
    POA_CNT_BAND_DIAG = 14,    // 14, 15: the last alignment that lost its band: rows | length; sequence of its pack | best score in the band
    POA_CNT_PUBLIC = 16,       // words of h_cnt
    POA_CNT_BARPROF = 16,      // POA_BARPROF: wave 1's segments
    POA_CNT_PROFILE = 32,      // + 8 x class: POA_PROFILE's phase ticks (poa_args::prof)
    POA_CNT_WORDS = 160
};
// poa.hip : device-resident POA over packs (sequences, offsets, column output in HBM)
int poa_device_run(rattle_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_off, const uint64_t *h_off, uint32_t n_seqs,
                   const uint32_t *h_pack_first, uint32_t n_packs, uint32_t *d_col, uint32_t *d_width, uint32_t *h_width,
                   unsigned long long *h_cnt, std::vector<uint8_t> *skipped);
// post_msa.hip
int launch_gather(rattle_ctx *ctx, const gather_desc *d_desc, uint32_t n, const uint8_t *sseq, const uint8_t *squal, uint8_t *dseq,
                  uint8_t *dqual);
int launch_post_msa(rattle_ctx *ctx, const post_args &A, uint32_t n_packs, int mode);
// cluster_driver.cpp
int cluster_driver_many(rattle_ctx *ctx, const rattle_cluster_params *P, const uint32_t *ids, const uint64_t *sub_off,
                        const uint32_t *which, uint32_t n_which, rattle_cluster_set **outs);
// ... all n_subsets of them, shared out over the ranks of the context and their sets exchanged: outs[i] for every subset, or none on error
int cluster_subsets_ranked(rattle_ctx *ctx, const rattle_cluster_params *P, const uint32_t *ids, const uint64_t *sub_off, uint32_t n_subsets,
                           rattle_cluster_set **outs);
int cluster_driver(rattle_ctx *ctx, const rattle_cluster_params *P, const uint32_t *subset, uint32_t n_subset,
                   rattle_cluster_set **out);
int debug_evaluate(rattle_ctx *ctx, const rattle_cluster_params *P, int count_mode, const rattle_debug_rect *R, uint32_t n_rects,
                   rattle_debug_eval **out);
// records [out_base, out_base + n_reads) of A: the loaded reads read_ids placed on the loaded reads target_ids
// C (or nullptr): the candidate lists of the same reads, slots [out_base * C->k, (out_base + n_reads) * C->k), and their counts
int assign_driver(rattle_ctx *ctx, const rattle_assign_params *P, const uint32_t *target_ids, uint32_t n_targets, const uint32_t *read_ids,
                  uint32_t n_reads, rattle_assignment *A, uint32_t out_base, rattle_candidates *C = nullptr);
// pair_cigar.hip : kernel F, the CIGAR of every pair kernel E aligned, chunk by chunk of kernel E while its sequences are on the device
struct cigar_pair {                     // one pair of a launch: where its rectangle's sequences, code records, strip and ops region lie
    uint64_t q, t;                      // byte offsets of the rectangle's first row (reverse strand: its last base as given) and first column
    uint64_t codes, strip, ops;         // offsets in 16-byte records, in 4-byte words, in 4-byte words
    uint32_t rows, cols, rev, pad;
};
struct cigar_in {                       // one pair of kernel E's chunk, from its record
    uint64_t q, t;
    uint32_t rows, cols, read;          // q_end - q_start, t_end - t_start, the read the ops belong to
    uint8_t status, rev;
};
struct cigar_run {                      // one call of rattle_hip_align_cigars: the result so far and the buffers, kept from chunk to chunk
    uint64_t code_cap = 0;              // cap on a sub-chunk's code bytes
    std::vector<uint32_t> count;        // [n_reads] ops of every read
    std::vector<uint32_t> ops;          // the ops of all reads, in read order
    dbuf<cigar_pair> d_pairs;
    dbuf<uint4> d_codes;
    dbuf<int32_t> d_strip;
    dbuf<uint32_t> d_ops, d_count, d_out;
    dbuf<uint64_t> d_off;
    hbuf<cigar_pair> h_pairs;
    hbuf<uint32_t> h_count, h_out;
    hbuf<uint64_t> h_off;
    // rattle_hip_align_pileup alone (kernel G, pair_pileup.hip); the align_cigars calls leave all of it as it stands here
    bool want_pileup = false;           // align_pairs_run makes the two tables below and hands h_pileup on filled
    bool keep_ops = true;               // false: the compact ops stay on the device: `ops` stays empty, `count` is filled for the pairs that
                                        // went to kernel F and stays 0 for a read-mode pair without a column (cigar_no_column is not run)
    uint32_t *h_pileup = nullptr;       // calloc'ed, the caller's to free: 8 planes of target_offsets[n_targets] counts, position p = byte p
    uint32_t *d_pileup = nullptr;       // 8 planes of pileup_n counts, position 0 = the first uploaded target byte (d_t)
    uint64_t pileup_n = 0;
};
uint64_t cigar_code_cap();              // 4 GiB, or what RATTLE_CIGAR_CODE_BYTES says
// pair_pileup.hip : kernel G over the m pairs of the sub-chunk that pair_cigar_chunk has just gathered (R.d_pairs, R.d_off, R.d_out), into R.d_pileup
int pair_pileup_launch(rattle_ctx *ctx, const cigar_run &R, uint32_t m, const uint8_t *d_q, uint64_t alg);
// scoring == nullptr: the linear form (GAP_LINEAR of pair_wave.h, id 7); else the affine form with that scoring (GAP_AFFINE, id 9)
int pair_cigar_chunk(rattle_ctx *ctx, const uint8_t *d_q, const uint8_t *d_t, const cigar_in *in, uint32_t n, uint32_t pair_chunk, cigar_run &R,
                     const rattle_align_scoring *scoring = nullptr, int mode = RATTLE_ALIGN_LOCAL);
// pair_align.hip : kernel E, the local alignment of every submitted read on its target; fills every array of A (arguments checked by the caller).
// With `cigars`, every chunk goes on to kernel F before its sequences leave the device (cigars->count sized n_reads by the caller).
// scoring == nullptr: kernels E and F (linear, ids 6 and 7); else their three-state forms with that scoring (ids 8 and 9).
// mode: RATTLE_ALIGN_LOCAL, or RATTLE_ALIGN_READ -- the whole read, the <*, true> instantiations of both kernels, the same ids.
struct align_pair {                     // one submitted pair: where its sequences lie in the uploaded buffers, and its strip (in records; unused when
    uint64_t q, t, strip;               // the read has one block)
    uint32_t lq, lt, rev, pad;
};
int align_pairs_run(rattle_ctx *ctx, const uint8_t *tseq, const uint64_t *toff, uint32_t n_targets, const uint8_t *rseq, const uint64_t *roff,
                    uint32_t n_reads, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, rattle_alignment *A,
                    cigar_run *cigars = nullptr, const rattle_align_scoring *scoring = nullptr, int mode = RATTLE_ALIGN_LOCAL);
// abundance.hip : the EM over the compatible targets tgt[r * k + j] (-1: slot j of read r takes no part; a read whose slot 0 is -1 takes
// none), n, nt >= 1, targets checked by the caller.  Fills R->iterations, converged, units, compatible_reads and posterior (allocated by
// the caller) and `deltas`, one entry per iteration run.
int abundance_run(rattle_ctx *ctx, const int32_t *h_tgt, uint32_t n, uint32_t k, uint32_t nt, unsigned long long tol_units, uint32_t max_iters,
                  uint32_t iter_block, rattle_abundance *R, std::vector<uint64_t> &deltas);
constexpr uint32_t AL_REC_WORDS = 10;   // a pair's record on the device: status, score, q_start, q_end, t_start, t_end, matches, mismatches, q_gap, t_gap

// correct_driver.hip
int debug_post_msa(rattle_ctx *ctx, const rattle_correct_params *P, int mode, const rattle_debug_msa *in, rattle_debug_post **out);
int debug_consensus_support(rattle_ctx *ctx, const rattle_correct_params *P, const rattle_debug_support_msa *in, rattle_debug_support **out);

}  // namespace rattle
