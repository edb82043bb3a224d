// extern "C" surface of librattle_hip.so (include/rattle_hip.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <dirent.h>
#include <unistd.h>

#include <memory>
#include <unordered_set>

#include "common.h"

namespace rattle {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

int launch_pair_score_oversize(rattle_ctx *ctx, const std::vector<uint32_t> &slots, uint32_t max_matches);
int poa_msa_run(rattle_ctx *ctx, const uint8_t *seq, const uint64_t *off, uint32_t n_seqs, const uint32_t *pack_first,
                uint32_t n_packs, rattle_msa_set **out);

int correct_driver(rattle_ctx *ctx, const uint8_t *seq, const uint8_t *qual, const uint64_t *off, uint32_t n_reads,
                   uint32_t n_clusters, const uint32_t *coff, const int32_t *mid, const uint8_t *mrev,
                   const rattle_correct_params *P, rattle_correction **out);

// Hardware queues the HIP runtime of this process hands out (kernel C runs one stream per POA column class and wants a queue
// for each: classes sharing a queue run one after the other, poa.hip).  The runtime reads GPU_MAX_HW_QUEUES once, when it
// starts -- the first HIP call of the process -- so the value is settled when this library is LOADED, not when kernel C runs:
// if the variable is set by then it is taken at its word; if it is not and the runtime has not started yet (no /dev/kfd
// descriptor in the process), the library sets it to 12 itself; otherwise the runtime is already running with its default of 4.
// RATTLE_NO_ENV_SETUP=1 keeps the library's hands off the environment (a multi-threaded host that cannot have setenv() called under
// it at dlopen time, or one that wants the runtime's default for its other HIP users): kernel C then deals its classes onto four streams.
static int g_hw_queues = 4;
__attribute__((constructor)) static void settle_hw_queues() {
    if (const char *v = getenv("GPU_MAX_HW_QUEUES")) { g_hw_queues = std::max(1, atoi(v)); return; }
    if (getenv("RATTLE_NO_ENV_SETUP")) return;
    bool runtime_up = false;
    if (DIR *d = opendir("/proc/self/fd")) {                 // every descriptor of the process, whatever its number
        char link[300], target[256];
        while (struct dirent *e = readdir(d)) {
            if (e->d_name[0] == '.') continue;
            snprintf(link, sizeof link, "/proc/self/fd/%s", e->d_name);
            const ssize_t n = readlink(link, target, sizeof target - 1);
            if (n > 0) { target[n] = 0; if (strcmp(target, "/dev/kfd") == 0) { runtime_up = true; break; } }
        }
        closedir(d);
    }
    if (!runtime_up) { setenv("GPU_MAX_HW_QUEUES", "12", 0); g_hw_queues = 12; }
}
int hw_queues() { return g_hw_queues; }

void dev_free(void *p) { if (p) (void)hipFree(p); }

// ---- result objects of `correct`: the public struct at the head of a box that also holds the correction report (common.h)
const char *const rep_names[REP_FIELDS] = {"in_len", "out_len", "trim_front", "trim_back", "match", "substituted", "mismatch_kept", "inserted", "deleted", "gap_kept"};
namespace {
std::mutex g_box_mu;
std::unordered_set<const rattle_correction *> &boxes() { static std::unordered_set<const rattle_correction *> s; return s; }
}  // namespace

rattle_correction *new_correction() {
    correction_box *B = (correction_box *)calloc(1, sizeof(correction_box));
    std::lock_guard<std::mutex> g(g_box_mu);
    boxes().insert(&B->pub);
    return &B->pub;
}

correction_box *box_of(const rattle_correction *c) {
    std::lock_guard<std::mutex> g(g_box_mu);
    return c && boxes().count(c) ? (correction_box *)c : nullptr;
}

// ---- result objects of `cluster`: the public struct at the head of a box that also holds the joins of the cluster report (common.h)
namespace {
std::unordered_set<const rattle_cluster_set *> &cluster_boxes() { static std::unordered_set<const rattle_cluster_set *> s; return s; }
}  // namespace

rattle_cluster_set *new_cluster_set() {
    cluster_box *B = (cluster_box *)calloc(1, sizeof(cluster_box));
    std::lock_guard<std::mutex> g(g_box_mu);
    cluster_boxes().insert(&B->pub);
    return &B->pub;
}

cluster_box *cluster_box_of(const rattle_cluster_set *cs) {
    std::lock_guard<std::mutex> g(g_box_mu);
    return cs && cluster_boxes().count(cs) ? (cluster_box *)cs : nullptr;
}

void alloc_report(correction_box *B, size_t n) {
    for (int f = 0; f < REP_FIELDS; ++f) { free(B->rep[f]); B->rep[f] = (uint32_t *)calloc(std::max<size_t>(1, n), 4); }
    B->has_report = true;
}

void alloc_support(correction_box *B, size_t n, size_t bases) {
    free(B->sup_level); B->sup_level = (uint8_t *)calloc(std::max<size_t>(1, n), 1);
    for (int f = 0; f < SUP_FIELDS; ++f) { free(B->sup[f]); B->sup[f] = (uint32_t *)calloc(std::max<size_t>(1, bases), 4); }
    B->has_support = true;
}

void print_support_totals(const rattle_correction *c) {
    static const bool enabled = getenv("RATTLE_TIMING") != nullptr;
    const correction_box *B = enabled ? box_of(c) : nullptr;
    if (!B || !B->has_support) return;
    const rattle_read_set &S = c->consensi;
    uint64_t sup = 0, dep = 0, weak = 0, composed = 0;
    for (uint64_t b = 0; b < S.off[S.n]; ++b) { sup += B->sup[SUP_SUPPORT][b]; dep += B->sup[SUP_DEPTH][b]; weak += 2ull * B->sup[SUP_SUPPORT][b] <= B->sup[SUP_DEPTH][b]; }
    for (uint32_t i = 0; i < S.n; ++i) composed += B->sup_level[i] == 3;
    fprintf(stderr, "[rattle] consensus support: %u consensi (%llu composed through POA #3), %llu bases, support %llu of depth %llu, %llu weak bases\n", S.n,
            (unsigned long long)composed, (unsigned long long)S.off[S.n], (unsigned long long)sup, (unsigned long long)dep, (unsigned long long)weak);
}

void print_report_totals(const rattle_correction *c, const char *what) {
    static const bool enabled = getenv("RATTLE_TIMING") != nullptr;
    const correction_box *B = enabled ? box_of(c) : nullptr;
    if (!B || !B->has_report) return;
    std::string line = std::string("[rattle] ") + what + ":";
    for (int f = REP_MATCH; f < REP_FIELDS; ++f) {
        uint64_t tot = 0;
        for (uint32_t i = 0; i < c->corrected.n; ++i) tot += B->rep[f][i];
        line += std::string(" ") + rep_names[f] + " " + std::to_string(tot);
    }
    fprintf(stderr, "%s (%u reads)\n", line.c_str(), c->corrected.n);
}

}  // namespace rattle

using namespace rattle;

// compute entry points need the context's device; a host-only context (rattle_hip_ctx_create_host) has none
static int use_device(rattle_ctx *c) {
    if (c->device < 0) { set_error("this context has no device (rattle_hip_ctx_create_host): only the exchange entry points work"); return RATTLE_ERR_STATE; }
    RT_HIP(hipSetDevice(c->device));
    return 0;
}

// The cluster report does not travel through the exchange of a sharded job yet: refused on every rank alike, before any collective
static int report_needs_one_rank(rattle_ctx *c) {
    if (c->cluster_report && c->xchg.nranks > 1) {
        set_error("the cluster report (rattle_hip_set_cluster_report) is not available on a context that is one rank of several: "
                  "switch it off on every rank, or cluster on one device");
        return RATTLE_ERR_STATE;
    }
    return 0;
}

// joins of a set whose ids were positions in `map` -> the ids map holds
static void translate_joins(rattle_cluster_set *cs, const uint32_t *map) {
    cluster_box *B = cluster_box_of(cs);
    if (!B || !B->has_report) return;
    for (cluster_join &j : *B->joins) { j.into = (int32_t)map[j.into]; j.absorbed = (int32_t)map[j.absorbed]; }
}

extern "C" {

const char *rattle_hip_last_error(void) { return g_err.c_str(); }
int rattle_hip_abi_version(void) { return 4; }

int rattle_hip_ctx_create(int device, rattle_ctx **out) {
    if (!out) { set_error("out is null"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error(std::string("no HIP device available (librattle_hip has no CPU fallback): ") + hipGetErrorString(e));
        return RATTLE_ERR_HIP;
    }
    if (device < 0 || device >= n) { set_error("device index out of range"); return RATTLE_ERR_ARG; }
    RT_HIP(hipSetDevice(device));
    rattle_ctx *c = new rattle_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess) {
        set_error("stream/event creation failed");
        delete c;
        return RATTLE_ERR_HIP;
    }
    if (getenv("RATTLE_NO_KERNEL_TIMING")) c->timing = false;
    *out = c;
    return 0;
}

int rattle_hip_ctx_create_host(rattle_ctx **out) {
    if (!out) { set_error("out is null"); return RATTLE_ERR_ARG; }
    rattle_ctx *c = new rattle_ctx();
    c->device = -1;
    c->timing = false;
    *out = c;
    return 0;
}

void rattle_hip_ctx_destroy(rattle_ctx *c) {
    if (!c) return;
    (void)rattle_hip_comm_destroy(c);
    delete c;            // ~rattle_ctx: streams, events, arena; the buffers release themselves
}

int rattle_hip_load_reads(rattle_ctx *c, const uint8_t *seq, const uint64_t *off, uint32_t n, int k, int both) {
    if (!c || !off || (n && !seq)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    return build_index(c, seq, off, n, k, both);
}

int rattle_hip_get_read_index(rattle_ctx *c, uint32_t r, int strand, uint32_t *hash_out, int32_t *pos_out, uint64_t *bv_out,
                              uint32_t *pc_out) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    read_index &X = c->idx;
    if (r >= X.n) { set_error("read out of range"); return RATTLE_ERR_ARG; }
    if (strand < 0 || strand > 1 || (strand == 1 && !X.both)) { set_error("strand not indexed"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    uint64_t ko = X.h_koff[r], nk = X.h_koff[r + 1] - ko;
    if (nk && hash_out) RT_HIP(hipMemcpy(hash_out, X.kh[strand].p + ko, nk * 4, hipMemcpyDeviceToHost));
    if (nk && pos_out) RT_HIP(hipMemcpy(pos_out, X.kp[strand].p + ko, nk * 4, hipMemcpyDeviceToHost));
    if (bv_out) RT_HIP(hipMemcpy(bv_out, X.bv[strand].p + (uint64_t)r * 64, 512, hipMemcpyDeviceToHost));
    if (pc_out) RT_HIP(hipMemcpy(pc_out, X.pc[strand].p + r, 4, hipMemcpyDeviceToHost));
    return 0;
}

int rattle_hip_bv_filter(rattle_ctx *c, const uint32_t *seed_ids, uint32_t n_seeds, const uint32_t *cand_ids, uint32_t n_cands,
                         const uint32_t *first_cand, const uint16_t *lut, int fwd_bypass, uint8_t *out_pass) {
    if (!c || !seed_ids || !cand_ids || !first_cand || !lut || !out_pass) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (c->idx.n == 0) { set_error("no reads loaded"); return RATTLE_ERR_STATE; }
    for (uint32_t i = 0; i < n_seeds; ++i) if (seed_ids[i] >= c->idx.n) { set_error("seed id out of range"); return RATTLE_ERR_ARG; }
    for (uint32_t i = 0; i < n_cands; ++i) if (cand_ids[i] >= c->idx.n) { set_error("cand id out of range"); return RATTLE_ERR_ARG; }
    if (n_seeds == 0 || n_cands == 0) return 0;
    RT_TRY(use_device(c));
    hipStream_t st = c->stream;
    RT_TRY(c->d_seed.reserve(n_seeds)); RT_TRY(c->d_first.reserve(n_seeds)); RT_TRY(c->d_cand.reserve(n_cands));
    RT_TRY(c->d_lut.reserve(4097)); RT_TRY(c->d_pass.reserve((size_t)n_seeds * n_cands)); RT_TRY(c->d_counter.reserve(4));
    RT_HIP(hipMemcpyAsync(c->d_seed.p, seed_ids, n_seeds * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(c->d_first.p, first_cand, n_seeds * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(c->d_cand.p, cand_ids, (size_t)n_cands * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(c->d_lut.p, lut, 4097 * 2, hipMemcpyHostToDevice, st));
    RT_TRY(launch_bv_filter(c, n_seeds, n_cands, fwd_bypass, true, false, 0));
    RT_HIP(hipMemcpyAsync(out_pass, c->d_pass.p, (size_t)n_seeds * n_cands, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return 0;
}

int rattle_hip_pair_score(rattle_ctx *c, const uint32_t *i_ids, const uint32_t *j_ids, const uint8_t *strand, uint32_t n,
                          int32_t *bases, int32_t *hc_bases, int32_t *n_dist, double *variance, int32_t *n_matches) {
    if (!c || !i_ids || !j_ids || !strand) { set_error("null argument"); return RATTLE_ERR_ARG; }
    read_index &X = c->idx;
    if (X.n == 0) { set_error("no reads loaded"); return RATTLE_ERR_STATE; }
    for (uint32_t p = 0; p < n; ++p) {
        if (i_ids[p] >= X.n || j_ids[p] >= X.n) { set_error("read id out of range"); return RATTLE_ERR_ARG; }
        if (strand[p] > 1 || (strand[p] == 1 && !X.both)) { set_error("strand not indexed"); return RATTLE_ERR_ARG; }
    }
    if (n == 0) return 0;
    RT_TRY(use_device(c));
    hipStream_t st = c->stream;
    RT_TRY(c->d_pi.reserve(n)); RT_TRY(c->d_pj.reserve(n)); RT_TRY(c->d_ps.reserve(n));
    RT_TRY(c->d_res.reserve((size_t)n * 4)); RT_TRY(c->d_var.reserve(n));
    RT_HIP(hipMemcpyAsync(c->d_pi.p, i_ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(c->d_pj.p, j_ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(c->d_ps.p, strand, n, hipMemcpyHostToDevice, st));
    RT_TRY(launch_pair_score(c, n));
    std::vector<int32_t> res((size_t)n * 4);
    std::vector<double> var(n);
    RT_HIP(hipMemcpyAsync(res.data(), c->d_res.p, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(var.data(), c->d_var.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> big;
    uint32_t big_m = 0;
    for (uint32_t p = 0; p < n; ++p)
        if (res[4 * (size_t)p] == INT32_MIN) { big.push_back(p); big_m = std::max(big_m, (uint32_t)res[4 * (size_t)p + 3]); }
    if (!big.empty()) {
        RT_TRY(launch_pair_score_oversize(c, big, big_m));
        RT_HIP(hipMemcpy(res.data(), c->d_res.p, (size_t)n * 16, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(var.data(), c->d_var.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    uint64_t bytes = 0;
    for (uint32_t p = 0; p < n; ++p) {
        if (bases) bases[p] = res[4 * (size_t)p];
        if (hc_bases) hc_bases[p] = res[4 * (size_t)p + 1];
        if (n_dist) n_dist[p] = res[4 * (size_t)p + 2];
        if (n_matches) n_matches[p] = res[4 * (size_t)p + 3];
        if (variance) variance[p] = var[p];
        bytes += 8ull * ((X.h_koff[i_ids[p] + 1] - X.h_koff[i_ids[p]]) + (X.h_koff[j_ids[p] + 1] - X.h_koff[j_ids[p]]));
    }
    c->stats[K_SCORE].bytes += bytes;
    return 0;
}

int rattle_hip_cluster_reads(rattle_ctx *c, const rattle_cluster_params *P, rattle_cluster_set **out) {
    if (!c || !P || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    RT_TRY(report_needs_one_rank(c));
    RT_TRY(use_device(c));
    if (c->idx.k == 0) { set_error("no reads loaded"); return RATTLE_ERR_STATE; }      // (never loaded, or the index made room for a big `correct`)
    if (!P->is_rna && !c->idx.both) { set_error("cDNA mode needs the reads loaded with both_strands=1"); return RATTLE_ERR_STATE; }
    // cluster.cpp:42: `if (is_rna) return {-1,false}` comes before the reverse test, so a both-strand index would over-cluster
    if (P->is_rna && c->idx.both) { set_error("--rna mode needs the reads loaded with both_strands=0"); return RATTLE_ERR_STATE; }
    return cluster_driver(c, P, nullptr, 0, out);
}

int rattle_hip_cluster_subset(rattle_ctx *c, const rattle_cluster_params *P, const uint32_t *subset, uint32_t n_subset,
                              rattle_cluster_set **out) {
    if (!c || !P || !out || (n_subset && !subset)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    RT_TRY(report_needs_one_rank(c));
    for (uint32_t i = 0; i < n_subset; ++i) if (subset[i] >= c->idx.n) { set_error("subset id out of range"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    if (!P->is_rna && !c->idx.both) { set_error("cDNA mode needs the reads loaded with both_strands=1"); return RATTLE_ERR_STATE; }
    // cluster.cpp:42: `if (is_rna) return {-1,false}` comes before the reverse test, so a both-strand index would over-cluster
    if (P->is_rna && c->idx.both) { set_error("--rna mode needs the reads loaded with both_strands=0"); return RATTLE_ERR_STATE; }
    static const uint32_t none = 0;
    return cluster_driver(c, P, n_subset ? subset : &none, n_subset, out);
}

// Many independent subsets at once (the --iso second level: one subset per gene cluster).  Small
// problems are launch- and synchronisation-bound, so the subsets' greedy rounds advance in lockstep and every
// round is ONE evaluation on the device (cluster_driver.hip: cluster_driver_many).
int rattle_hip_cluster_subsets(rattle_ctx *c, const rattle_cluster_params *P, const uint32_t *ids, const uint64_t *sub_off,
                               uint32_t n_subsets, rattle_cluster_set **outs, int n_workers) {
    if (!c || !P || !outs || !sub_off || (n_subsets && sub_off[n_subsets] && !ids)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    for (uint32_t i = 0; i < n_subsets; ++i) outs[i] = nullptr;
    RT_TRY(report_needs_one_rank(c));
    for (uint64_t i = 0; i < sub_off[n_subsets]; ++i) if (ids[i] >= c->idx.n) { set_error("subset id out of range"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    if (!P->is_rna && !c->idx.both) { set_error("cDNA mode needs the reads loaded with both_strands=1"); return RATTLE_ERR_STATE; }
    // cluster.cpp:42: `if (is_rna) return {-1,false}` comes before the reverse test, so a both-strand index would over-cluster
    if (P->is_rna && c->idx.both) { set_error("--rna mode needs the reads loaded with both_strands=0"); return RATTLE_ERR_STATE; }
    RT_HIP(hipStreamSynchronize(c->stream));
    (void)n_workers;                                              // round 1 ran one host thread per worker; the subsets now advance in lockstep
    return cluster_subsets_ranked(c, P, ids, sub_off, n_subsets, outs);
}

int rattle_hip_stage_reads(rattle_ctx *c, const uint8_t *seq, const uint8_t *qual, const uint64_t *off, uint32_t n) {
    if (!c || !off || (n && !seq)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    const uint64_t total = off[n] - off[0];
    c->staged_seq_key = nullptr; c->staged_qual_key = nullptr;
    RT_TRY(c->d_staged_seq.reserve(total + 64));
    RT_HIP(hipMemcpy(c->d_staged_seq.p, seq + off[0], total, hipMemcpyHostToDevice));
    if (qual) {
        RT_TRY(c->d_staged_qual.reserve(total + 64));
        RT_HIP(hipMemcpy(c->d_staged_qual.p, qual + off[0], total, hipMemcpyHostToDevice));
        c->staged_qual_key = qual;
    }
    c->staged_seq_key = seq; c->staged_n = n; c->staged_total = total;
    return 0;
}

int rattle_hip_unstage_reads(rattle_ctx *c) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    c->staged_seq_key = nullptr; c->staged_qual_key = nullptr; c->staged_n = 0; c->staged_total = 0;
    c->d_staged_seq.release(); c->d_staged_qual.release();
    return 0;
}

// main.cpp:254-262: stable sort by length, longest first (counting sort; lengths are small integers), the reads
// gathered into processing order (on the device when they are staged there) and indexed with k-mer size k
static int sort_and_index(rattle_ctx *c, const uint8_t *seq, const uint64_t *off, uint32_t n, int k, int both, std::vector<uint32_t> &order) {
    order.resize(n);
    {
        phase_timer T("cluster: sort + gather");
        uint64_t max_len = 0;
        for (uint32_t i = 0; i < n; ++i) max_len = std::max<uint64_t>(max_len, off[i + 1] - off[i]);
        if (max_len <= (1u << 24)) {
            std::vector<uint32_t> start(max_len + 2, 0);
            for (uint32_t i = 0; i < n; ++i) ++start[max_len - (off[i + 1] - off[i]) + 1];      // bucket 0 = longest
            for (uint64_t b = 0; b <= max_len; ++b) start[b + 1] += start[b];
            for (uint32_t i = 0; i < n; ++i) order[start[max_len - (off[i + 1] - off[i])]++] = i;
        } else {
            for (uint32_t i = 0; i < n; ++i) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [off](uint32_t a, uint32_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
        }
    }
    std::vector<uint64_t> soff(n + 1);
    {
        uint64_t p = 0;
        for (uint32_t i = 0; i < n; ++i) { soff[i] = p; p += off[order[i] + 1] - off[order[i]]; }
        soff[n] = p;
    }
    if (n && c->staged_seq_key == seq && c->staged_n == n && c->staged_total == off[n] - off[0] && off[0] == 0) {
        // the reads are resident (rattle_hip_stage_reads): gather them into processing order on the device
        phase_timer T("cluster: device gather + build_index");
        std::vector<gather_desc> desc(n);
        for (uint32_t i = 0; i < n; ++i) desc[i] = gather_desc{off[order[i]], soff[i], (uint32_t)(soff[i + 1] - soff[i]), 0u};
        dbuf<gather_desc> d_desc;
        dbuf<uint8_t> d_cat;
        RT_TRY(d_desc.reserve(n)); RT_TRY(d_cat.reserve(soff[n] + 64));
        RT_HIP(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)n * sizeof(gather_desc), hipMemcpyHostToDevice, c->stream));
        RT_TRY(launch_gather(c, d_desc.p, n, c->d_staged_seq.p, nullptr, d_cat.p, nullptr));
        int rc = build_index(c, d_cat.p, soff.data(), n, k, both);
        RT_HIP(hipStreamSynchronize(c->stream));
        return rc;
    }
    std::unique_ptr<uint8_t[]> cat(new uint8_t[off[n] - off[0] + 1]);
    {
        phase_timer T("cluster: host gather");
        const size_t chunk = 2048;
        parallel_for((n + chunk - 1) / chunk, 0, [&](size_t ch) {
            for (size_t i = ch * chunk; i < std::min<size_t>(n, (ch + 1) * chunk); ++i)
                memcpy(cat.get() + soff[i], seq + off[order[i]], soff[i + 1] - soff[i]);
        });
    }
    phase_timer T("cluster: build_index");
    return build_index(c, cat.get(), soff.data(), n, k, both);
}

int rattle_hip_cluster_unsorted(rattle_ctx *c, const uint8_t *seq, const uint64_t *off, uint32_t n, int k,
                                const rattle_cluster_params *P, rattle_cluster_set **out) {
    if (!c || !off || !P || !out || (n && !seq)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    RT_TRY(report_needs_one_rank(c));
    RT_TRY(use_device(c));
    phase_timer T_all("cluster_unsorted: total");
    std::vector<uint32_t> order;
    RT_TRY(sort_and_index(c, seq, off, n, k, P->is_rna ? 0 : 1, order));
    { phase_timer T("cluster: greedy driver"); RT_TRY(cluster_driver(c, P, nullptr, 0, out)); }
    rattle_cluster_set *cs = *out;
    const uint32_t nm = cs->offsets[cs->n_clusters];
    for (uint32_t i = 0; i < cs->n_clusters; ++i) cs->main_id[i] = (int32_t)order[cs->main_id[i]];
    for (uint32_t i = 0; i < nm; ++i) cs->member_id[i] = (int32_t)order[cs->member_id[i]];
    translate_joins(cs, order.data());
    return 0;
}

// `rattle cluster --iso`, main.cpp:254-323, for reads in FILE order: gene level with (k, gene params), then every
// gene cluster's members -- re-sorted by length desc, ties larger id first (:285-291; the order cluster_reads
// already leaves them in) -- clustered again with (iso_k, iso params); transcript clusters appended in gene
// order, each carrying its gene's index.
int rattle_hip_cluster_iso_unsorted(rattle_ctx *c, const uint8_t *seq, const uint64_t *off, uint32_t n, int k, int iso_k,
                                    const rattle_cluster_params *P, const rattle_cluster_params *iso_P, rattle_cluster_set **out,
                                    uint32_t *n_gene_clusters) {
    if (!c || !off || !P || !iso_P || !out || (n && !seq)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    RT_TRY(report_needs_one_rank(c));
    RT_TRY(use_device(c));
    phase_timer T_all("cluster_iso_unsorted: total");
    std::vector<uint32_t> order;
    RT_TRY(sort_and_index(c, seq, off, n, k, P->is_rna ? 0 : 1, order));
    rattle_cluster_set *gene = nullptr;
    { phase_timer T("cluster: gene level"); RT_TRY(cluster_driver(c, P, nullptr, 0, &gene)); }
    struct freer { rattle_cluster_set *p; ~freer() { rattle_hip_cluster_set_free(p); } } gene_free{gene};
    if (n_gene_clusters) *n_gene_clusters = gene->n_clusters;
    // second index with the iso k-mer size over the same (already sorted, device-resident) reads
    {
        phase_timer T("cluster: iso index");
        std::vector<uint64_t> soff = c->idx.h_off;
        RT_TRY(build_index(c, c->idx.seq.p, soff.data(), n, iso_k, iso_P->is_rna ? 0 : 1));
    }
    const uint32_t G = gene->n_clusters;
    std::vector<uint32_t> ids(gene->offsets[G] ? gene->offsets[G] : 1);
    std::vector<uint64_t> sub_off(G + 1, 0);
    for (uint32_t g = 0; g <= G; ++g) sub_off[g] = gene->offsets[g];
    for (uint32_t i = 0; i < gene->offsets[G]; ++i) ids[i] = (uint32_t)gene->member_id[i];
    std::vector<rattle_cluster_set *> subs(G ? G : 1, nullptr);
    { phase_timer T("cluster: iso level"); RT_TRY(rattle_hip_cluster_subsets(c, iso_P, ids.data(), sub_off.data(), G, subs.data(), 0)); }
    size_t nc = 0, nm = 0;
    for (uint32_t g = 0; g < G; ++g) { nc += subs[g]->n_clusters; nm += subs[g]->offsets[subs[g]->n_clusters]; }
    rattle_cluster_set *R = new_cluster_set();
    // the cluster report: the gene level's joins, then every gene's, all in the caller's order
    std::vector<cluster_join> *joins = nullptr;
    if (const cluster_box *GB = cluster_box_of(gene); GB && GB->has_report) {
        joins = new std::vector<cluster_join>(*GB->joins);
        for (cluster_join &j : *joins) { j.into = (int32_t)order[j.into]; j.absorbed = (int32_t)order[j.absorbed]; }
        cluster_box *RB = cluster_box_of(R);
        RB->joins = joins; RB->has_report = true;
    }
    R->n_clusters = (uint32_t)nc;
    R->main_id = (int32_t *)malloc(std::max<size_t>(1, nc) * 4); R->main_rev = (uint8_t *)malloc(std::max<size_t>(1, nc));
    R->gene_id = (int32_t *)malloc(std::max<size_t>(1, nc) * 4);
    R->offsets = (uint32_t *)malloc((nc + 1) * 4);
    R->member_id = (int32_t *)malloc(std::max<size_t>(1, nm) * 4); R->member_rev = (uint8_t *)malloc(std::max<size_t>(1, nm));
    uint32_t ci = 0, mi = 0;
    for (int i = 0; i < 8; ++i) R->counters[i] = gene->counters[i];
    for (uint32_t g = 0; g < G; ++g) {
        const rattle_cluster_set *S = subs[g];
        const uint32_t *gids = ids.data() + sub_off[g];
        for (uint32_t k2 = 0; k2 < S->n_clusters; ++k2) {
            R->main_id[ci] = (int32_t)order[gids[S->main_id[k2]]]; R->main_rev[ci] = S->main_rev[k2]; R->gene_id[ci] = (int32_t)g;
            R->offsets[ci] = mi;
            for (uint32_t t = S->offsets[k2]; t < S->offsets[k2 + 1]; ++t) { R->member_id[mi] = (int32_t)order[gids[S->member_id[t]]]; R->member_rev[mi] = S->member_rev[t]; ++mi; }
            ++ci;
        }
        for (int i = 0; i < 8; ++i) R->counters[i] += S->counters[i];
        if (const cluster_box *SB = joins ? cluster_box_of(S) : nullptr; SB && SB->has_report)
            for (cluster_join j : *SB->joins) {
                j.level = 1; j.into = (int32_t)order[gids[j.into]]; j.absorbed = (int32_t)order[gids[j.absorbed]];
                joins->push_back(j);
            }
        rattle_hip_cluster_set_free(subs[g]);
    }
    R->offsets[nc] = mi;
    *out = R;
    return 0;
}

void rattle_hip_cluster_set_free(rattle_cluster_set *cs) {
    if (!cs) return;
    if (cluster_box *B = cluster_box_of(cs)) {
        delete B->joins;
        std::lock_guard<std::mutex> g(g_box_mu);
        cluster_boxes().erase(cs);
    }
    free(cs->main_id); free(cs->main_rev); free(cs->offsets); free(cs->member_id); free(cs->member_rev); free(cs->gene_id);
    free(cs);
}

int rattle_hip_set_cluster_report(rattle_ctx *c, int on) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    c->cluster_report = on != 0;
    if (!c->cluster_report) { c->d_hit_ev.release(); c->h_hit_ev.release(); }
    return 0;
}

int rattle_hip_cluster_report(const rattle_cluster_set *cs, rattle_cluster_report **out) {
    if (out) *out = nullptr;
    if (!cs || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    const cluster_box *B = cluster_box_of(cs);
    if (!B || !B->has_report) {
        set_error("this cluster set carries no report: rattle_hip_set_cluster_report(ctx, 1) comes before the clustering call, and the set must be one this library returned");
        return RATTLE_ERR_STATE;
    }
    const std::vector<cluster_join> &J = *B->joins;
    const size_t n = J.size(), m = std::max<size_t>(1, n);
    rattle_cluster_report *R = (rattle_cluster_report *)calloc(1, sizeof(rattle_cluster_report));
    R->n = n;
    R->level = (uint8_t *)malloc(m); R->pass = (uint32_t *)malloc(4 * m); R->bv_threshold = (double *)malloc(8 * m);
    R->into = (int32_t *)malloc(4 * m); R->absorbed = (int32_t *)malloc(4 * m); R->rev = (uint8_t *)malloc(m);
    R->bases = (int32_t *)malloc(4 * m); R->hc_bases = (int32_t *)malloc(4 * m); R->min_len = (uint32_t *)malloc(4 * m);
    R->score = (double *)malloc(8 * m); R->variance = (double *)malloc(8 * m);
    for (size_t i = 0; i < n; ++i) {
        const cluster_join &j = J[i];
        R->level[i] = j.level; R->pass[i] = j.pass; R->bv_threshold[i] = j.thr; R->into[i] = j.into; R->absorbed[i] = j.absorbed;
        R->rev[i] = j.rev; R->bases[i] = j.bases; R->hc_bases[i] = j.hc; R->min_len[i] = j.min_len; R->score[i] = j.score;
        R->variance[i] = j.variance;
    }
    *out = R;
    return 0;
}

void rattle_hip_cluster_report_free(rattle_cluster_report *r) {
    if (!r) return;
    free(r->level); free(r->pass); free(r->bv_threshold); free(r->into); free(r->absorbed); free(r->rev); free(r->bases);
    free(r->hc_bases); free(r->min_len); free(r->score); free(r->variance);
    free(r);
}

// ---- assign ---------------------------------------------------------------------------------------------------------------
// n records, every read unassigned
static rattle_assignment *new_assignment(uint32_t n) {
    const size_t m = std::max<size_t>(1, n);
    rattle_assignment *A = (rattle_assignment *)calloc(1, sizeof(rattle_assignment));
    A->n = n;
    A->target = (int32_t *)malloc(4 * m); A->rev = (uint8_t *)calloc(m, 1);
    A->bases = (int32_t *)calloc(m, 4); A->hc_bases = (int32_t *)calloc(m, 4); A->min_len = (uint32_t *)calloc(m, 4);
    A->score = (double *)malloc(8 * m); A->variance = (double *)calloc(m, 8); A->second_score = (double *)malloc(8 * m);
    A->n_accepted = (uint32_t *)calloc(m, 4);
    for (size_t i = 0; i < m; ++i) { A->target[i] = -1; A->score[i] = -1.0; A->second_score[i] = -1.0; }
    return A;
}

// n reads of k slots, every slot unused
static rattle_candidates *new_candidates(uint32_t n, uint32_t k) {
    const size_t m = std::max<size_t>(1, (size_t)n * k);
    rattle_candidates *C = (rattle_candidates *)calloc(1, sizeof(rattle_candidates));
    C->n = n; C->k = k;
    C->count = (uint32_t *)calloc(std::max<size_t>(1, n), 4);
    C->target = (int32_t *)malloc(4 * m); C->rev = (uint8_t *)calloc(m, 1);
    C->bases = (int32_t *)calloc(m, 4); C->hc_bases = (int32_t *)calloc(m, 4); C->min_len = (uint32_t *)calloc(m, 4);
    C->score = (double *)malloc(8 * m); C->variance = (double *)calloc(m, 8);
    for (size_t i = 0; i < m; ++i) { C->target[i] = -1; C->score[i] = -1.0; }
    return C;
}

// the candidate list a call asks for (the _top entry points): none for the plain ones
struct top_request { bool on; uint32_t k; rattle_candidates **cands; };

// what the entry points require of their parameters and of the context, in the order the header promises: arguments (the _top
// calls' own last), then the refusal of a sharded job (before anything is exchanged), then the device
static int assign_enter(rattle_ctx *c, const rattle_assign_params *P, const top_request &T) {
    if (P->count_pass < 0 || P->count_pass > 3) { set_error("count_pass must be 0 (auto), 1 (seed-major), 2 (search) or 3 (index)"); return RATTLE_ERR_ARG; }
    if (T.on && (T.k < 1 || T.k > 8)) { set_error("k, the candidates per read, must be in [1,8]"); return RATTLE_ERR_ARG; }
    if (T.on && !T.cands) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (c->xchg.nranks > 1) {
        set_error("assign is not available on a context that is one rank of several: sharded jobs are not built, assign on one device");
        return RATTLE_ERR_STATE;
    }
    return use_device(c);
}

static int assign_loaded(rattle_ctx *c, const rattle_assign_params *P, const uint32_t *tids, uint32_t nt, const uint32_t *rids, uint32_t nr,
                         rattle_assignment **out, const top_request &T) {
    if (out) *out = nullptr;
    if (T.cands) *T.cands = nullptr;
    if (!c || !P || !out || (nt && !tids) || (nr && !rids)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (nt >= (1u << 31)) { set_error("too many targets"); return RATTLE_ERR_ARG; }
    RT_TRY(assign_enter(c, P, T));
    if (nt && nr) {
        if (c->idx.k == 0) { set_error("no reads loaded"); return RATTLE_ERR_STATE; }
        if (!P->is_rna && !c->idx.both) { set_error("cDNA mode needs the reads loaded with both_strands=1"); return RATTLE_ERR_STATE; }
        if (P->is_rna && c->idx.both) { set_error("--rna mode needs the reads loaded with both_strands=0"); return RATTLE_ERR_STATE; }
        for (uint32_t i = 0; i < nt; ++i) if (tids[i] >= c->idx.n) { set_error("target id out of range"); return RATTLE_ERR_ARG; }
        for (uint32_t i = 0; i < nr; ++i) if (rids[i] >= c->idx.n) { set_error("read id out of range"); return RATTLE_ERR_ARG; }
    }
    rattle_assignment *A = new_assignment(nr);
    rattle_candidates *C = T.on ? new_candidates(nr, T.k) : nullptr;
    const int rc = assign_driver(c, P, tids, nt, rids, nr, A, 0, C);
    if (rc != 0) { rattle_hip_assignment_free(A); rattle_hip_candidates_free(C); return rc; }
    *out = A;
    if (T.on) *T.cands = C;
    return 0;
}

int rattle_hip_assign_loaded(rattle_ctx *c, const rattle_assign_params *P, const uint32_t *tids, uint32_t nt, const uint32_t *rids,
                             uint32_t nr, rattle_assignment **out) {
    return assign_loaded(c, P, tids, nt, rids, nr, out, top_request{false, 0, nullptr});
}

int rattle_hip_assign_loaded_top(rattle_ctx *c, const rattle_assign_params *P, const uint32_t *tids, uint32_t nt, const uint32_t *rids,
                                 uint32_t nr, uint32_t k, rattle_assignment **out, rattle_candidates **cands) {
    return assign_loaded(c, P, tids, nt, rids, nr, out, top_request{true, k, cands});
}

static int assign_reads(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                        uint32_t nr, int k, const rattle_assign_params *P, rattle_assignment **out, const top_request &T) {
    if (out) *out = nullptr;
    if (T.cands) *T.cands = nullptr;
    if (!c || !P || !out || !toff || !roff || (nt && !tseq) || (nr && !rseq)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (k < 1 || k > 16) { set_error("kmer size must be in [1,16] (main.cpp:223)"); return RATTLE_ERR_ARG; }
    if (nt >= (1u << 31)) { set_error("too many targets"); return RATTLE_ERR_ARG; }
    RT_TRY(assign_enter(c, P, T));
    phase_timer T_all("assign_reads: total");
    rattle_assignment *A = new_assignment(nr);
    rattle_candidates *C = T.on ? new_candidates(nr, T.k) : nullptr;
    struct freer { rattle_assignment *p; rattle_candidates *q; ~freer() { rattle_hip_assignment_free(p); rattle_hip_candidates_free(q); } } guard{A, C};
    const uint64_t tbytes = nt ? toff[nt] - toff[0] : 0;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(P->read_chunk ? P->read_chunk : 1u << 20, 0xFFFFFFF0ull - nt);
    std::vector<uint32_t> tids(nt), rids;
    for (uint32_t i = 0; i < nt; ++i) tids[i] = i;
    std::vector<uint64_t> off;
    std::unique_ptr<uint8_t[]> cat;
    size_t cat_cap = 0;
    for (uint64_t r0 = 0; nt && r0 < nr; r0 += chunk) {
        // the targets, then the chunk's reads, as ONE read set: ids [0, nt) and [nt, nt + m)
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, nr - r0);
        const uint64_t rbytes = roff[r0 + m] - roff[r0];
        if (tbytes + rbytes + 1 > cat_cap) { cat_cap = tbytes + rbytes + 1; cat.reset(new uint8_t[cat_cap]); if (tbytes) memcpy(cat.get(), tseq + toff[0], tbytes); }
        if (rbytes) memcpy(cat.get() + tbytes, rseq + roff[r0], rbytes);
        off.resize((size_t)nt + m + 1);
        for (uint32_t i = 0; i <= nt; ++i) off[i] = toff[i] - toff[0];
        for (uint32_t i = 0; i <= m; ++i) off[(size_t)nt + i] = tbytes + (roff[r0 + i] - roff[r0]);
        RT_TRY(build_index(c, cat.get(), off.data(), nt + m, k, P->is_rna ? 0 : 1));
        rids.resize(m);
        for (uint32_t i = 0; i < m; ++i) rids[i] = nt + i;
        RT_TRY(assign_driver(c, P, tids.data(), nt, rids.data(), m, A, (uint32_t)r0, C));
    }
    guard.p = nullptr; guard.q = nullptr;
    *out = A;
    if (T.on) *T.cands = C;
    return 0;
}

int rattle_hip_assign_reads(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                            uint32_t nr, int k, const rattle_assign_params *P, rattle_assignment **out) {
    return assign_reads(c, tseq, toff, nt, rseq, roff, nr, k, P, out, top_request{false, 0, nullptr});
}

int rattle_hip_assign_reads_top(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                                uint32_t nr, int kmer_size, const rattle_assign_params *P, uint32_t k, rattle_assignment **out,
                                rattle_candidates **cands) {
    return assign_reads(c, tseq, toff, nt, rseq, roff, nr, kmer_size, P, out, top_request{true, k, cands});
}

void rattle_hip_candidates_free(rattle_candidates *c) {
    if (!c) return;
    free(c->count); free(c->target); free(c->rev); free(c->bases); free(c->hc_bases); free(c->min_len); free(c->score); free(c->variance);
    free(c);
}

// ---- abundance (abundance.hip) ----------------------------------------------------------------------------------------------
// the checks in the order the header promises, the compatibility mask on the host (the rule's own double expression; this file is built
// with -ffp-contract=off), the EM on the device, the per-target doubles from its integers
int rattle_hip_abundance(rattle_ctx *c, const rattle_candidates *cands, uint32_t nt, const rattle_abundance_params *params, rattle_abundance **out) {
    if (out) *out = nullptr;
    if (!c || !cands || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    const uint32_t n = cands->n, k = cands->k;
    if (n && (!cands->count || !cands->target || !cands->score)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (k < 1 || k > 8) { set_error("abundance: k, the slots per read, must be in [1,8]"); return RATTLE_ERR_ARG; }
    for (uint32_t r = 0; r < n; ++r)
        if (cands->count[r] > k) { set_error("abundance: count of read " + std::to_string(r) + " exceeds k"); return RATTLE_ERR_ARG; }
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t j = 0; j < cands->count[r]; ++j) {
            const int32_t t = cands->target[(size_t)r * k + j];
            if (t < 0 || (uint32_t)t >= nt) {
                set_error("abundance: slot " + std::to_string(j) + " of read " + std::to_string(r) + " names target " + std::to_string(t) + " of " + std::to_string(nt));
                return RATTLE_ERR_ARG;
            }
        }
    const rattle_abundance_params dflt = {0.95, 1e-3, 1000, 0};
    const rattle_abundance_params P = params ? *params : dflt;
    if (!(P.ratio > 0.0 && P.ratio <= 1.0)) { set_error("abundance: ratio must be in (0, 1]"); return RATTLE_ERR_ARG; }
    if (!(P.tol >= 0.0 && P.tol < 1048576.0)) { set_error("abundance: tol must be in [0, 2^20) reads"); return RATTLE_ERR_ARG; }
    if (P.max_iters == 0) { set_error("abundance: max_iters must be at least 1"); return RATTLE_ERR_ARG; }
    if (c->xchg.nranks > 1) {
        set_error("abundance is not available on a context that is one rank of several: sharded jobs are not built, estimate on one device");
        return RATTLE_ERR_STATE;
    }
    RT_TRY(use_device(c));
    phase_timer T_all("abundance: total");
    rattle_abundance *R = (rattle_abundance *)calloc(1, sizeof(rattle_abundance));
    const size_t mt = std::max<size_t>(1, nt), ms = std::max<size_t>(1, (size_t)n * k);
    R->n_targets = nt; R->n_reads = n; R->k = k; R->converged = 1;
    R->units = (uint64_t *)calloc(mt, 8); R->est_reads = (double *)calloc(mt, 8); R->cpm = (double *)calloc(mt, 8);
    R->compatible_reads = (uint32_t *)calloc(mt, 4); R->posterior = (double *)calloc(ms, 8);
    std::vector<uint64_t> deltas;
    if (n && nt) {
        std::vector<int32_t> tgt((size_t)n * k, -1);
        for (uint32_t r = 0; r < n; ++r) {
            const size_t s = (size_t)r * k;
            if (cands->count[r] == 0) continue;
            ++R->n_placed;
            const double least = P.ratio * cands->score[s];
            tgt[s] = cands->target[s];
            for (uint32_t j = 1; j < cands->count[r]; ++j) if (cands->score[s + j] >= least) tgt[s + j] = cands->target[s + j];
        }
        const int rc = abundance_run(c, tgt.data(), n, k, nt, (unsigned long long)(P.tol * 4294967296.0), P.max_iters, P.iter_block, R, deltas);
        if (rc != 0) { rattle_hip_abundance_free(R); return rc; }
    }
    R->delta = (uint64_t *)calloc(std::max<size_t>(1, deltas.size()), 8);
    for (size_t i = 0; i < deltas.size(); ++i) R->delta[i] = deltas[i];
    const double mass = (double)(R->n_placed << 32);
    for (uint32_t t = 0; t < nt; ++t) {
        R->est_reads[t] = (double)R->units[t] / 4294967296.0;
        R->cpm[t] = R->n_placed ? (double)R->units[t] / mass * 1e6 : 0.0;
    }
    *out = R;
    return 0;
}

void rattle_hip_abundance_free(rattle_abundance *a) {
    if (!a) return;
    free(a->units); free(a->est_reads); free(a->cpm); free(a->compatible_reads); free(a->delta); free(a->posterior);
    free(a);
}

void rattle_hip_assignment_free(rattle_assignment *a) {
    if (!a) return;
    free(a->target); free(a->rev); free(a->bases); free(a->hc_bases); free(a->min_len); free(a->score); free(a->variance);
    free(a->second_score); free(a->n_accepted);
    free(a);
}

// ---- align_pairs (kernel E), align_cigars (kernels E and F), and their _scored forms (the three-state kernels) ------------
// what an entry point asks of align_entry
struct align_request {
    std::string who;                  // the entry point's name in the messages
    bool scored;                      // a scoring is required: S is checked behind every other argument, still before the device is looked
                                      // at, and the three-state kernels run
    const rattle_align_scoring *S;
    int mode;
};
// the request of a *_mode entry point: scoring NULL is the linear form, and RATTLE_ALIGN_LOCAL is the call it stands for, name and all
static align_request mode_request(const char *call, const rattle_align_scoring *S, int mode) {
    return {std::string(call) + (mode != RATTLE_ALIGN_LOCAL ? "_mode" : S ? "_scored" : ""), S != nullptr, S, mode};
}

// the body of the six entry points, from the null-argument check on; `run` (the align_cigars calls) takes the ops of kernel F
static int align_entry(const align_request &Q, rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                       uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, rattle_alignment **out, cigar_run *run) {
    if (out) *out = nullptr;
    if (!c || !P || !out || !toff || !roff || (nr && (!target || !rev)) || (!tseq && toff[nt] != toff[0]) || (!rseq && roff[nr] != roff[0])) {
        set_error("null argument");
        return RATTLE_ERR_ARG;
    }
    const auto &[who, scored, S, mode] = Q;
    const std::string w = who + ": ";
    // the arguments, on the host: indices, strands, lengths, and the letters of every sequence that is submitted (a target once)
    auto clean = [](const uint8_t *s, uint64_t n) { for (uint64_t i = 0; i < n; ++i) if (!s[i] || !strchr("ACGTU", s[i])) return false; return true; };
    std::vector<uint8_t> seen(nt, 0);
    for (uint32_t r = 0; r < nr; ++r) {
        const int32_t t = target[r];
        if (t < 0) continue;
        if ((uint32_t)t >= nt) { set_error(w + "read " + std::to_string(r) + " names target " + std::to_string(t) + " of " + std::to_string(nt)); return RATTLE_ERR_ARG; }
        if (rev[r] > 1) { set_error(w + "rev of read " + std::to_string(r) + " is neither 0 nor 1"); return RATTLE_ERR_ARG; }
        if (roff[r + 1] - roff[r] >= (1ull << 31) || toff[t + 1] - toff[t] >= (1ull << 31)) { set_error(w + "a sequence of 2^31 bases or more"); return RATTLE_ERR_ARG; }
        if (!clean(rseq + roff[r], roff[r + 1] - roff[r])) { set_error(w + "read " + std::to_string(r) + " has a base other than A, C, G, T, U"); return RATTLE_ERR_ARG; }
        if (!seen[t]) {
            if (!clean(tseq + toff[t], toff[t + 1] - toff[t])) { set_error(w + "target " + std::to_string(t) + " has a base other than A, C, G, T, U"); return RATTLE_ERR_ARG; }
            seen[t] = 1;
        }
    }
    if (c->xchg.nranks > 1) {
        set_error(who + " is not available on a context that is one rank of several: sharded jobs are not built, align on one device");
        return RATTLE_ERR_STATE;
    }
    if (scored) {
        if (!S) { set_error(w + "null scoring"); return RATTLE_ERR_ARG; }
        if (S->match < 1 || S->match > 64 || S->mismatch < 1 || S->mismatch > 64 || S->gap_open < 1 || S->gap_open > 64 || S->gap_extend < 1 ||
            S->gap_extend > S->gap_open) {
            set_error(w + "scoring " + std::to_string(S->match) + "," + std::to_string(S->mismatch) + "," + std::to_string(S->gap_open) + "," +
                      std::to_string(S->gap_extend) + ": match, mismatch, gap_open, gap_extend must be in [1, 64] and gap_extend <= gap_open");
            return RATTLE_ERR_ARG;
        }
        for (uint32_t r = 0; r < nr; ++r) {
            if (target[r] < 0) continue;
            const uint64_t lq = roff[r + 1] - roff[r], lt = toff[target[r] + 1] - toff[target[r]];
            if (S->match * std::min(lq, lt) > 0x7FFFFFFFull) {
                set_error(w + "read " + std::to_string(r) + ": match * min(Lq, Lt) exceeds 2^31 - 1, the score might not fit the record");
                return RATTLE_ERR_ARG;
            }
        }
    }
    // the mode (the *_mode entry points), behind every check of the four calls: the left border of the read mode, -(open + (Lq - 1) extend),
    // has to stay well above PW_NEG = -2^30, the kernels' minus infinity
    if (mode != RATTLE_ALIGN_LOCAL && mode != RATTLE_ALIGN_READ) { set_error(w + "mode " + std::to_string(mode) + " is neither RATTLE_ALIGN_LOCAL nor RATTLE_ALIGN_READ"); return RATTLE_ERR_ARG; }
    if (mode == RATTLE_ALIGN_READ) {
        const uint64_t o = scored ? S->gap_open : 8, e = scored ? S->gap_extend : 8;
        for (uint32_t r = 0; r < nr; ++r) {
            if (target[r] < 0) continue;
            const uint64_t lq = roff[r + 1] - roff[r];
            if (lq && o + e * (lq - 1) >= (1ull << 29)) {
                set_error(w + "read " + std::to_string(r) + ": gap_open + gap_extend * (Lq - 1) reaches 2^29, a read that long cannot be aligned end to end");
                return RATTLE_ERR_ARG;
            }
        }
    }
    RT_TRY(use_device(c));
    const size_t m = std::max<size_t>(1, nr);
    rattle_alignment *A = (rattle_alignment *)calloc(1, sizeof(rattle_alignment));
    A->n = nr;
    A->status = (uint8_t *)calloc(m, 1); A->score = (int32_t *)calloc(m, 4);
    for (uint32_t **f : {&A->q_start, &A->q_end, &A->t_start, &A->t_end, &A->matches, &A->mismatches, &A->q_gap, &A->t_gap}) *f = (uint32_t *)calloc(m, 4);
    if (run) { run->count.assign(nr, 0); run->ops.clear(); run->code_cap = cigar_code_cap(); }
    const int rc = align_pairs_run(c, tseq, toff, nt, rseq, roff, nr, target, rev, P, A, run, scored ? S : nullptr, mode);
    if (rc != 0) { rattle_hip_alignment_free(A); return rc; }
    *out = A;
    return 0;
}

int rattle_hip_align_pairs(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                           uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, rattle_alignment **out) {
    return align_entry({"align_pairs", false, nullptr, RATTLE_ALIGN_LOCAL}, c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, nullptr);
}

int rattle_hip_align_pairs_scored(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                                  uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, const rattle_align_scoring *S,
                                  rattle_alignment **out) {
    return align_entry({"align_pairs_scored", true, S, RATTLE_ALIGN_LOCAL}, c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, nullptr);
}

// the ops and counts of a finished run as the caller's arrays
static rattle_cigars *cigars_from(const cigar_run &run, uint32_t nr) {
    rattle_cigars *G = (rattle_cigars *)calloc(1, sizeof(rattle_cigars));
    G->n = nr;
    G->offset = (uint64_t *)calloc((size_t)nr + 1, 8);
    G->ops = (uint32_t *)calloc(std::max<size_t>(1, run.ops.size()), 4);
    for (uint32_t r = 0; r < nr; ++r) G->offset[r + 1] = G->offset[r] + run.count[r];
    if (!run.ops.empty()) memcpy(G->ops, run.ops.data(), run.ops.size() * 4);
    return G;
}

// the body of the three align_cigars calls: its own null argument, align_entry, and the ops as the caller's arrays
static int cigars_entry(const align_request &Q, rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                        uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, rattle_alignment **out,
                        rattle_cigars **cigars) {
    if (out) *out = nullptr;
    if (cigars) *cigars = nullptr;
    if (!cigars) { set_error("null argument"); return RATTLE_ERR_ARG; }
    cigar_run run;
    RT_TRY(align_entry(Q, c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, &run));
    *cigars = cigars_from(run, nr);
    return 0;
}

int rattle_hip_align_cigars(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                            uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, rattle_alignment **out,
                            rattle_cigars **cigars) {
    return cigars_entry({"align_cigars", false, nullptr, RATTLE_ALIGN_LOCAL}, c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, cigars);
}

int rattle_hip_align_cigars_scored(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                                   uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, const rattle_align_scoring *S,
                                   rattle_alignment **out, rattle_cigars **cigars) {
    return cigars_entry({"align_cigars_scored", true, S, RATTLE_ALIGN_LOCAL}, c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, cigars);
}

// the four calls above with a mode
int rattle_hip_align_pairs_mode(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                                uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, const rattle_align_scoring *S,
                                int mode, rattle_alignment **out) {
    return align_entry(mode_request("align_pairs", S, mode), c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, nullptr);
}

int rattle_hip_align_cigars_mode(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                                 uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, const rattle_align_scoring *S,
                                 int mode, rattle_alignment **out, rattle_cigars **cigars) {
    return cigars_entry(mode_request("align_cigars", S, mode), c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, cigars);
}

// align_cigars_mode, and kernel G's table of the same call; without `cigars` the ops stay on the device
int rattle_hip_align_pileup(rattle_ctx *c, const uint8_t *tseq, const uint64_t *toff, uint32_t nt, const uint8_t *rseq, const uint64_t *roff,
                            uint32_t nr, const int32_t *target, const uint8_t *rev, const rattle_align_params *P, const rattle_align_scoring *S,
                            int mode, rattle_alignment **out, rattle_cigars **cigars, rattle_pileup **pileup) {
    if (out) *out = nullptr;
    if (cigars) *cigars = nullptr;
    if (pileup) *pileup = nullptr;
    if (!pileup) { set_error("null argument"); return RATTLE_ERR_ARG; }
    cigar_run run;
    run.want_pileup = true; run.keep_ops = cigars != nullptr;
    const int rc = align_entry({"align_pileup", S != nullptr, S, mode}, c, tseq, toff, nt, rseq, roff, nr, target, rev, P, out, &run);
    if (rc != 0) { free(run.h_pileup); return rc; }
    if (cigars) *cigars = cigars_from(run, nr);
    rattle_pileup *U = (rattle_pileup *)calloc(1, sizeof(rattle_pileup));
    const uint64_t N = toff[nt];
    U->n = N;
    uint32_t **planes[8] = {&U->a, &U->c, &U->g, &U->t, &U->del, &U->ins, &U->starts, &U->ends};
    for (uint32_t k = 0; k < 8; ++k) *planes[k] = run.h_pileup + k * N;      // one allocation: rattle_hip_pileup_free frees it through `a`
    *pileup = U;
    return 0;
}

void rattle_hip_pileup_free(rattle_pileup *u) {
    if (!u) return;
    free(u->a);
    free(u);
}

void rattle_hip_cigars_free(rattle_cigars *g) {
    if (!g) return;
    free(g->offset); free(g->ops);
    free(g);
}

void rattle_hip_alignment_free(rattle_alignment *a) {
    if (!a) return;
    free(a->status); free(a->score); free(a->q_start); free(a->q_end); free(a->t_start); free(a->t_end); free(a->matches); free(a->mismatches);
    free(a->q_gap); free(a->t_gap);
    free(a);
}

int rattle_hip_poa_msa(rattle_ctx *c, const uint8_t *seq, const uint64_t *off, uint32_t n_seqs, const uint32_t *pack_first,
                       uint32_t n_packs, rattle_msa_set **out) {
    if (!c || !off || !pack_first || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    // byte 0 pads the rows' columns beyond a sequence and '-' is the gap of the rows that come back: neither can be a letter (checked on the
    // host, before the device is looked at)
    for (uint32_t q = 0; q < n_seqs; ++q) {
        if (off[q + 1] < off[q]) { set_error("offsets must not decrease"); return RATTLE_ERR_ARG; }
        const uint64_t len = off[q + 1] - off[q];
        if (!len) continue;
        if (!seq) { set_error("null argument"); return RATTLE_ERR_ARG; }
        const bool nul = memchr(seq + off[q], 0, len) != nullptr;
        if (nul || memchr(seq + off[q], '-', len)) {
            set_error("poa_msa: sequence " + std::to_string(q) + " holds " + (nul ? "a zero byte" : "'-'") + ": every byte but 0 and '-' is a letter");
            return RATTLE_ERR_ARG;
        }
    }
    RT_TRY(use_device(c));
    return poa_msa_run(c, seq, off, n_seqs, pack_first, n_packs, out);
}

void rattle_hip_msa_set_free(rattle_msa_set *ms) {
    if (!ms) return;
    free(ms->width); free(ms->row_offset); free(ms->rows);
    free(ms);
}

int rattle_hip_correct_reads(rattle_ctx *c, const uint8_t *seq, const uint8_t *qual, const uint64_t *off, uint32_t n_reads,
                             uint32_t n_clusters, const uint32_t *coff, const int32_t *mid, const uint8_t *mrev,
                             const rattle_correct_params *P, rattle_correction **out) {
    if (!c || !off || !P || !out || (n_clusters && (!coff || !mid || !mrev)) || (n_reads && (!seq || !qual))) {
        set_error("null argument");
        return RATTLE_ERR_ARG;
    }
    *out = nullptr;
    RT_TRY(use_device(c));
    // The consensus support does not travel through the exchange of a sharded job yet: refused on every rank alike, before any collective
    if (c->consensus_support && c->xchg.nranks > 1) {
        set_error("the consensus support (rattle_hip_set_consensus_support) is not available on a context that is one rank of several: "
                  "switch it off on every rank, or correct on one device");
        return RATTLE_ERR_STATE;
    }
    {
        // A context that clustered its reads still holds their k-mer index (12-20 bytes per base) and kernel B's work lists; `correct`
        // uses none of it and sizes its arena by what is free.  Beyond 24 GB the index goes first (3e6 mixed reads: 72 GB of it beside the
        // arena ran stage 2 out of memory); the reads must then be loaded again before the next cluster call, which is what every
        // caller of the big jobs does anyway (RATTLE_ERR_STATE "no reads loaded" otherwise).
        read_index &X = c->idx;
        const uint64_t held = 4ull * (X.uh.cap + X.kh[0].cap + X.kh[1].cap + X.kp[0].cap + X.kp[1].cap) + 8ull * (X.bv[0].cap + X.bv[1].cap);
        const char *keep_mb = getenv("RATTLE_INDEX_KEEP_MB");            // (tests lower the bound to see the index go)
        if (held > (keep_mb ? (uint64_t)strtoull(keep_mb, nullptr, 10) << 20 : 24ull << 30)) {
            X.uh.release(); X.kh[0].release(); X.kh[1].release(); X.kp[0].release(); X.kp[1].release(); X.bv[0].release(); X.bv[1].release();
            X.pc[0].release(); X.pc[1].release(); X.seq.release(); X.off.release(); X.koff.release(); X.len.release();
            X.n = 0; X.k = 0; X.total_bases = X.total_kmers = 0;
            c->d_surv.release(); c->d_surv2.release(); c->d_sort_tmp.release(); c->d_pi.release(); c->d_pj.release(); c->d_ps.release();
            c->d_pi2.release(); c->d_pj2.release(); c->d_slot2.release(); c->d_ps2.release(); c->d_res.release(); c->d_var.release();
            c->d_scratch.release(); c->d_pass.release();
        }
    }
    int rc = correct_driver(c, seq, qual, off, n_reads, n_clusters, coff, mid, mrev, P, out);
    if (rc != 0 && *out) { rattle_hip_correction_free(*out); *out = nullptr; }
    return rc;
}

int rattle_hip_reserve_arena(rattle_ctx *c, uint64_t bytes) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    size_t free_b = 0, total_b = 0;
    RT_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t take = std::min<uint64_t>(bytes, (uint64_t)((free_b + c->poa_arena_bytes) * 0.8));
    if (take <= c->poa_arena_bytes) return 0;
    if (c->poa_arena) (void)hipFree(c->poa_arena);
    c->poa_arena = nullptr; c->poa_arena_bytes = 0;
    RT_HIP(hipMalloc((void **)&c->poa_arena, take));
    c->poa_arena_bytes = take;
    return 0;
}

static void free_set(rattle_read_set &s) {
    free(s.read_id); free(s.cluster_id); free(s.n_reads); free(s.off); free(s.seq); free(s.qual);
}

void rattle_hip_correction_free(rattle_correction *r) {
    if (!r) return;
    if (correction_box *B = box_of(r)) {
        for (int f = 0; f < REP_FIELDS; ++f) free(B->rep[f]);
        for (int f = 0; f < SUP_FIELDS; ++f) free(B->sup[f]);
        free(B->sup_level);
        std::lock_guard<std::mutex> g(g_box_mu);
        boxes().erase(r);
    }
    free_set(r->corrected); free_set(r->uncorrected); free_set(r->consensi);
    free(r->skipped.cluster_id); free(r->skipped.pack); free(r->skipped.stage); free(r->skipped.read_off); free(r->skipped.read_id);
    free(r->corrected_pack); free(r->uncorrected_pack);
    free(r);
}

int rattle_hip_set_correction_report(rattle_ctx *c, int on) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    c->correction_report = on != 0;
    return 0;
}

int rattle_hip_correction_report(const rattle_correction *c, rattle_correction_report **out) {
    if (out) *out = nullptr;
    if (!c || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    const correction_box *B = box_of(c);
    if (!B || !B->has_report) {
        set_error("this correction carries no report: rattle_hip_set_correction_report(ctx, 1) comes before rattle_hip_correct_reads, on every rank of a sharded job");
        return RATTLE_ERR_STATE;
    }
    rattle_correction_report *R = (rattle_correction_report *)calloc(1, sizeof(rattle_correction_report));
    const size_t n = c->corrected.n;
    R->n = (uint32_t)n;
    uint32_t **dst[REP_FIELDS] = {&R->in_len, &R->out_len, &R->trim_front, &R->trim_back, &R->match, &R->substituted, &R->mismatch_kept,
                                  &R->inserted, &R->deleted, &R->gap_kept};
    for (int f = 0; f < REP_FIELDS; ++f) {
        *dst[f] = (uint32_t *)malloc(std::max<size_t>(1, n) * 4);
        if (n) memcpy(*dst[f], B->rep[f], n * 4);
    }
    *out = R;
    return 0;
}

void rattle_hip_correction_report_free(rattle_correction_report *r) {
    if (!r) return;
    free(r->in_len); free(r->out_len); free(r->trim_front); free(r->trim_back); free(r->match); free(r->substituted);
    free(r->mismatch_kept); free(r->inserted); free(r->deleted); free(r->gap_kept);
    free(r);
}

int rattle_hip_set_consensus_support(rattle_ctx *c, int on) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    c->consensus_support = on != 0;
    return 0;
}

int rattle_hip_consensus_support(const rattle_correction *c, rattle_consensus_support **out) {
    if (out) *out = nullptr;
    if (!c || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    const correction_box *B = box_of(c);
    if (!B || !B->has_support) {
        set_error("this correction carries no consensus support: rattle_hip_set_consensus_support(ctx, 1) comes before rattle_hip_correct_reads, on one device, "
                  "and the correction must be one this library returned");
        return RATTLE_ERR_STATE;
    }
    rattle_consensus_support *R = (rattle_consensus_support *)calloc(1, sizeof(rattle_consensus_support));
    const rattle_read_set &S = c->consensi;
    const size_t n = S.n, bases = S.off[n];
    R->n = (uint32_t)n;
    R->level = (uint8_t *)malloc(std::max<size_t>(1, n));
    R->off = (uint64_t *)malloc((n + 1) * 8);
    if (n) memcpy(R->level, B->sup_level, n);
    memcpy(R->off, S.off, (n + 1) * 8);
    uint32_t **dst[SUP_FIELDS] = {&R->support, &R->depth, &R->pack_support, &R->pack_depth};
    for (int f = 0; f < SUP_FIELDS; ++f) {
        *dst[f] = (uint32_t *)malloc(std::max<size_t>(1, bases) * 4);
        if (bases) memcpy(*dst[f], B->sup[f], bases * 4);
    }
    *out = R;
    return 0;
}

void rattle_hip_consensus_support_free(rattle_consensus_support *s) {
    if (!s) return;
    free(s->level); free(s->off); free(s->support); free(s->depth); free(s->pack_support); free(s->pack_depth);
    free(s);
}

// Test hook (no device needed): the value of `-10*log10(p)+33` before the narrowing to char, once through the
// threshold table kernel D uses and once through the host libm (utils.cpp:6-8).  They must agree for every p.
int rattle_hip_debug_phred_symbol(double p, int *table_value, int *libm_value) {
    static std::mutex mu;
    static phred_table T;
    static bool ready = false;
    {
        std::lock_guard<std::mutex> g(mu);
        if (!ready) { build_phred_table(T); ready = true; }
    }
    if (table_value) *table_value = phred_lookup_host(T, p);
    if (libm_value) *libm_value = (int)(-10 * log10(p) + 33);
    return (int)T.exc_bits.size();
}

int rattle_hip_debug_evaluate(rattle_ctx *c, const rattle_cluster_params *P, int count_pass, const rattle_debug_rect *R,
                              uint32_t n_rects, rattle_debug_eval **out) {
    if (!c || !P || !out || (n_rects && !R)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    if (count_pass < 0 || count_pass > 3) { set_error("count_pass must be 0 (auto), 1 (seed-major), 2 (search) or 3 (index)"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    if (c->idx.k == 0) { set_error("no reads loaded"); return RATTLE_ERR_STATE; }
    if (!P->is_rna && !c->idx.both) { set_error("cDNA mode needs the reads loaded with both_strands=1"); return RATTLE_ERR_STATE; }
    if (P->is_rna && c->idx.both) { set_error("--rna mode needs the reads loaded with both_strands=0"); return RATTLE_ERR_STATE; }
    for (uint32_t r = 0; r < n_rects; ++r) {
        if ((R[r].n_seeds && !R[r].seed_ids) || (!R[r].triangular && R[r].n_cands && !R[r].cand_ids)) { set_error("null argument"); return RATTLE_ERR_ARG; }
        for (uint32_t i = 0; i < R[r].n_seeds; ++i) if (R[r].seed_ids[i] >= c->idx.n) { set_error("seed id out of range"); return RATTLE_ERR_ARG; }
        if (!R[r].triangular)
            for (uint32_t i = 0; i < R[r].n_cands; ++i) if (R[r].cand_ids[i] >= c->idx.n) { set_error("cand id out of range"); return RATTLE_ERR_ARG; }
    }
    return debug_evaluate(c, P, count_pass, R, n_rects, out);
}

static void free_pairs(rattle_debug_pairs &d) { free(d.rect); free(d.seed); free(d.cand); free(d.strand); free(d.count); }

void rattle_hip_debug_evaluate_free(rattle_debug_eval *e) {
    if (!e) return;
    free_pairs(e->survivors); free_pairs(e->kept); free_pairs(e->hits);
    free(e->hit_bases); free(e->hit_hc_bases); free(e->hit_variance);
    free(e->counters);
    free(e);
}

// what the kernel D test hooks require of an MSA before anything of it reaches the device
static int check_debug_msa(const rattle_debug_msa *in, int mode) {
    if (!in->pack_first || !in->off || (in->n_packs && !in->width)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (mode != 1 && mode != 2) { set_error("mode must be 1 (after POA #1: correction) or 2 (after POA #2 / #3: consensus)"); return RATTLE_ERR_ARG; }
    const uint32_t np = in->n_packs;
    if (in->pack_first[0] != 0 || in->off[0] != 0) { set_error("pack_first and off must start at 0"); return RATTLE_ERR_ARG; }
    for (uint32_t p = 0; p < np; ++p) if (in->pack_first[p + 1] < in->pack_first[p]) { set_error("pack_first decreases"); return RATTLE_ERR_ARG; }
    const uint32_t n = in->pack_first[np];
    for (uint32_t q = 0; q < n; ++q) if (in->off[q + 1] < in->off[q]) { set_error("off decreases"); return RATTLE_ERR_ARG; }
    if (in->off[n] && (!in->seq || !in->col)) { set_error("null argument"); return RATTLE_ERR_ARG; }
    if (mode == 1 && in->off[n] && !in->qual) { set_error("mode 1 needs the qualities"); return RATTLE_ERR_ARG; }
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t W = in->width[p];
        if (W == 0) continue;                                    // a skipped pack: its columns are never read
        if ((uint64_t)(in->pack_first[p + 1] - in->pack_first[p]) * W > (1ull << 32)) { set_error("pack too large for the test hook"); return RATTLE_ERR_ARG; }
        for (uint32_t q = in->pack_first[p]; q < in->pack_first[p + 1]; ++q)
            for (uint64_t b = in->off[q]; b < in->off[q + 1]; ++b) {
                if (!strchr("ACGTU", in->seq[b]) || !in->seq[b]) { set_error("row " + std::to_string(q) + ": a base other than A, C, G, T, U"); return RATTLE_ERR_ARG; }
                if (in->col[b] >= W) { set_error("row " + std::to_string(q) + ": column " + std::to_string(in->col[b]) + " is not below the pack's width " + std::to_string(W)); return RATTLE_ERR_ARG; }
                if (b > in->off[q] && in->col[b] <= in->col[b - 1]) { set_error("row " + std::to_string(q) + ": columns are not strictly increasing"); return RATTLE_ERR_ARG; }
            }
    }
    return 0;
}

int rattle_hip_debug_post_msa(rattle_ctx *c, const rattle_correct_params *P, int mode, const rattle_debug_msa *in, rattle_debug_post **out) {
    if (!c || !P || !in || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    RT_TRY(check_debug_msa(in, mode));
    RT_TRY(use_device(c));
    int rc = debug_post_msa(c, P, mode, in, out);
    if (rc != 0 && *out) { rattle_hip_debug_post_msa_free(*out); *out = nullptr; }
    return rc;
}

void rattle_hip_debug_post_msa_free(rattle_debug_post *d) {
    if (!d) return;
    free(d->moff); free(d->coff); free(d->rfirst); free(d->rlast); free(d->tfront); free(d->tback); free(d->olen); free(d->out_off);
    free(d->out_seq); free(d->out_qual); free(d->cons); free(d->flag); free(d->sym); free(d->err); free(d->cons_len); free(d->consensus);
    free(d->match); free(d->substituted); free(d->mismatch_kept); free(d->inserted); free(d->deleted); free(d->gap_kept);
    free(d);
}

int rattle_hip_debug_consensus_support(rattle_ctx *c, const rattle_correct_params *P, const rattle_debug_support_msa *in, rattle_debug_support **out) {
    if (!c || !P || !in || !out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    *out = nullptr;
    const rattle_debug_msa M = {in->n_packs, in->pack_first, in->width, in->off, in->seq, nullptr, in->col};
    RT_TRY(check_debug_msa(&M, 2));
    if ((in->sup == nullptr) != (in->dep == nullptr)) { set_error("sup and dep come together (both NULL: rows that are reads)"); return RATTLE_ERR_ARG; }
    RT_TRY(use_device(c));
    int rc = debug_consensus_support(c, P, in, out);
    if (rc != 0 && *out) { rattle_hip_debug_consensus_support_free(*out); *out = nullptr; }
    return rc;
}

void rattle_hip_debug_consensus_support_free(rattle_debug_support *d) {
    if (!d) return;
    free(d->coff); free(d->cons_len); free(d->consensus); free(d->support); free(d->depth); free(d->pack_support); free(d->pack_depth);
    free(d);
}

int rattle_hip_kernel_stats(rattle_ctx *c, int kernel, double *ms, uint64_t *launches, uint64_t *bytes) {
    if (!c || kernel < 0 || kernel >= K_COUNT) { set_error("bad kernel id"); return RATTLE_ERR_ARG; }
    if (ms) *ms = c->stats[kernel].ms;
    if (launches) *launches = c->stats[kernel].launches;
    if (bytes) *bytes = c->stats[kernel].bytes;
    return 0;
}

int rattle_hip_kernel_stats_reset(rattle_ctx *c) {
    if (!c) { set_error("null ctx"); return RATTLE_ERR_ARG; }
    for (int i = 0; i < K_COUNT; ++i) c->stats[i] = kstat();
    return 0;
}

int rattle_hip_stage_ms(rattle_ctx *c, double *ms_out, int reset) {
    if (!c || !ms_out) { set_error("null argument"); return RATTLE_ERR_ARG; }
    for (int i = 0; i < 8; ++i) { ms_out[i] = c->stage_ms[i]; if (reset) c->stage_ms[i] = 0; }
    return 0;
}

}  // extern "C"
