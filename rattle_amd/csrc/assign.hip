// `assign`: reads placed on a given set of targets by their best cluster_together score.  The evaluation is the greedy clustering's
// (cluster_driver.hip: kernels A and B, the count bound, the verdict's double expression); its second ending, here, replaces the hit
// list by a reduction per read over every accepted (target, strand) comparison of the evaluation, so that a fixed-size record per read
// is all the host ever sees, however many isoforms accept a read.
//
// Shape ("assign"): three passes of plain atomics over the n2 kept pairs of one target batch into a batch-local state,
//   1. best   = atomicMax over the accepted pairs of (bit pattern of the score) + 1   (scores are doubles >= +0: the pattern orders them;
//               0 = nothing accepted), n = atomicAdd of 1; pairs whose match list did not fit LDS are listed for the oversize
//               relaunch as the verdict kernel lists them, and pass 1 runs again over that list once their res / var are filled in;
//   2. key    = atomicMin of (target index << 1 | strand) over the accepted pairs whose score equals best: lowest target, forward first;
//   3. second = atomicMax of the score pattern over the accepted pairs of OTHER targets than key's; the one pair that owns key writes
//               its evidence (bases, hc_bases, the variance's 64 bits) with one 16-byte vector store,
// then one thread per read folds the batch's state into the call's state and clears it.  Every step is a max, a min or a count, so the
// result does not depend on the order in which the device scores the pairs; batches are folded in target order with a strict `>`, so an
// equal score of a later batch never displaces a lower target index.
//
// The candidate list (`assign_*_top`, DESIGN.md "assign: the candidate list"): the k best targets of every read in a second state of k
// slots per read (pattern, key, evidence), filled behind pass 3 and rank by rank -- slot 0 is the record above; for j = 1 .. k - 1
//   (a) atomicMax of the pattern into slot j over the accepted pairs whose TARGET sits in none of the slots < j (so the other strand of
//       a target is no second candidate), the owner of slot j - 1's key writing that slot's evidence on the way,
//   (b) atomicMin of the key over those pairs that reach slot j's pattern,
// and one thread per read merges the batch's sorted slots into the call's, the call's entry ahead on an equal pattern.  The rule of
// this file holds there too: every step is a max, a min, a count, or a per-read operation on data that is already order-free, so two
// runs give the same bits; no step lists pairs, waits for another wavefront or synchronises with the host, every loop is bounded by k.
#include "common.h"

namespace rattle {

namespace {

// the verdict's test (cluster_driver.hip: verdict_body) on kept pair q; pat = the score's bit pattern + 1
__device__ __forceinline__ bool accepted(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t q,
                                         const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj, const uint32_t *__restrict__ len,
                                         int use_hc, double t_s, double t_v, unsigned long long &pat) {
    const int32_t *r = res + 4 * (size_t)q;
    const uint32_t li = len[pi[q]], lj = len[pj[q]];
    const double mn = (double)(li < lj ? li : lj);
    const double score = use_hc ? (double)r[1] / mn : (double)r[0] / mn;
    pat = (unsigned long long)__double_as_longlong(score) + 1ull;
    return score >= t_s && var[q] < t_v;
}

// pass 1 over pairs [0, n) (remap: over the pairs remap[0 .. n), the oversize list after its relaunch).  out[1] / out[2] / big: the
// pairs still to be scored by the oversize pass, their count and largest match count (the verdict kernel's protocol).
__global__ __launch_bounds__(256) void assign_max_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                         const uint32_t *__restrict__ remap, const uint32_t *__restrict__ pi,
                                                         const uint32_t *__restrict__ pj, const uint32_t *__restrict__ slot2,
                                                         const uint32_t *__restrict__ len, int use_hc, double t_s, double t_v,
                                                         unsigned long long *__restrict__ out, uint32_t *__restrict__ big, assign_dev B) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool over = false;
    uint32_t q = 0, m_over = 0;
    if (t < n) {
        q = remap ? remap[t] : t;
        const int32_t *r = res + 4 * (size_t)q;
        if (r[0] == INT32_MIN) { over = true; m_over = (uint32_t)r[3]; }
        else {
            unsigned long long pat;
            if (accepted(res, var, q, pi, pj, len, use_hc, t_s, t_v, pat)) {
                const uint32_t c = slot2[2 * (size_t)q + 1];
                atomicMax(&B.best[c], pat);
                atomicAdd(&B.n[c], 1u);
            }
        }
    }
    const unsigned long long mo = __ballot(over);
    if (mo) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&out[1], (unsigned long long)__popcll(mo));
        base = __shfl(base, 0, 64);
        if (over) { big[base + (uint64_t)__popcll(mo & ((1ull << lane) - 1ull))] = q; atomicMax(&out[2], (unsigned long long)m_over); }
    }
}

// pass 2: the lowest (target << 1 | strand) among the pairs that reach the best score
__global__ __launch_bounds__(256) void assign_key_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                         const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj,
                                                         const uint32_t *__restrict__ slot2, const uint32_t *__restrict__ len, int use_hc,
                                                         double t_s, double t_v, uint32_t base, assign_dev B) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    unsigned long long pat;
    if (!accepted(res, var, q, pi, pj, len, use_hc, t_s, t_v, pat)) return;
    const uint32_t a = slot2[2 * (size_t)q], c = slot2[2 * (size_t)q + 1];
    if (pat == B.best[c]) atomicMin(&B.key[c], ((base + (a >> 1)) << 1) | (a & 1u));
}

// pass 3: the runner-up over the other targets; the winning pair's evidence
__global__ __launch_bounds__(256) void assign_second_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                            const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj,
                                                            const uint32_t *__restrict__ slot2, const uint32_t *__restrict__ len, int use_hc,
                                                            double t_s, double t_v, uint32_t base, assign_dev B) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    unsigned long long pat;
    if (!accepted(res, var, q, pi, pj, len, use_hc, t_s, t_v, pat)) return;
    const uint32_t a = slot2[2 * (size_t)q], c = slot2[2 * (size_t)q + 1];
    const uint32_t key = ((base + (a >> 1)) << 1) | (a & 1u), win = B.key[c];
    if (key == win) {
        const int32_t *r = res + 4 * (size_t)q;
        const unsigned long long vb = (unsigned long long)__double_as_longlong(var[q]);
        B.ev[c] = make_uint4((uint32_t)r[0], (uint32_t)r[1], (uint32_t)vb, (uint32_t)(vb >> 32));
    } else if ((key >> 1) != (win >> 1)) atomicMax(&B.second[c], pat);
}

// the batch's state B folded into the call's state G, one thread per read; B is left cleared for the next batch.  Batches come in
// target order: on an equal score G (a lower target index) stays.
__global__ __launch_bounds__(256) void assign_merge_kernel(uint32_t nr, assign_dev B, assign_dev G) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const unsigned long long bb = B.best[r];
    if (bb == 0) return;
    const unsigned long long gb = G.best[r], gs = G.second[r], bs = B.second[r];
    G.n[r] += B.n[r];
    if (bb > gb) {
        G.second[r] = gb > bs ? gb : bs;              // (gs <= gb)
        G.best[r] = bb; G.key[r] = B.key[r]; G.ev[r] = B.ev[r];
    } else G.second[r] = gs > bb ? gs : bb;           // (bs <= bb)
    B.best[r] = 0; B.second[r] = 0; B.n[r] = 0; B.key[r] = 0xFFFFFFFFu;
}

// ---- the candidate list: k slots per read beside the record above ------------------------------------------------------------------
// slot 0 of the batch is the batch's record: best, key and evidence as passes 1 to 3 left them (an unused slot: 0, 0xFFFFFFFF, zeros)
__global__ __launch_bounds__(256) void top_seed_kernel(uint32_t nr, assign_dev B, top_dev T) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const size_t s = (size_t)r * T.k;
    T.pat[s] = B.best[r]; T.key[s] = B.key[r]; T.ev[s] = B.ev[r];
}

// is accepted pair (key, read c) a comparison of slot j: a target that sits in none of the slots < j.  A read with no more than j
// accepted comparisons in this batch (B.n) has no slot j; neither has one whose slot j - 1 stayed empty.
__device__ __forceinline__ bool top_open(const assign_dev &B, const top_dev &T, uint32_t c, uint32_t key, uint32_t j) {
    if (B.n[c] <= j) return false;
    const size_t s = (size_t)c * T.k;
    if (T.pat[s + j - 1] == 0) return false;
    for (uint32_t i = 0; i < j; ++i) if ((T.key[s + i] >> 1) == (key >> 1)) return false;
    return true;
}

// rank j, step (a): the pair that owns slot j - 1's key writes that slot's evidence; then (j < k) atomicMax of the score pattern into
// slot j over the accepted pairs of the targets in none of the slots < j.  j runs 1 .. k: the launch with j == k only writes evidence.
__global__ __launch_bounds__(256) void top_max_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                      const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj,
                                                      const uint32_t *__restrict__ slot2, const uint32_t *__restrict__ len, int use_hc,
                                                      double t_s, double t_v, uint32_t base, uint32_t j, assign_dev B, top_dev T) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    unsigned long long pat;
    if (!accepted(res, var, q, pi, pj, len, use_hc, t_s, t_v, pat)) return;
    const uint32_t a = slot2[2 * (size_t)q], c = slot2[2 * (size_t)q + 1];
    const uint32_t key = ((base + (a >> 1)) << 1) | (a & 1u);
    const size_t s = (size_t)c * T.k;
    if (j > 1 && T.key[s + j - 1] == key) {               // (slot 0's evidence came with the seed)
        const int32_t *r = res + 4 * (size_t)q;
        const unsigned long long vb = (unsigned long long)__double_as_longlong(var[q]);
        T.ev[s + j - 1] = make_uint4((uint32_t)r[0], (uint32_t)r[1], (uint32_t)vb, (uint32_t)(vb >> 32));
        return;
    }
    if (j < T.k && top_open(B, T, c, key, j)) atomicMax(&T.pat[s + j], pat);
}

// rank j, step (b): the lowest (target << 1 | strand) among those pairs that reach slot j's pattern
__global__ __launch_bounds__(256) void top_key_kernel(const int32_t *__restrict__ res, const double *__restrict__ var, uint32_t n,
                                                      const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj,
                                                      const uint32_t *__restrict__ slot2, const uint32_t *__restrict__ len, int use_hc,
                                                      double t_s, double t_v, uint32_t base, uint32_t j, assign_dev B, top_dev T) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    unsigned long long pat;
    if (!accepted(res, var, q, pi, pj, len, use_hc, t_s, t_v, pat)) return;
    const uint32_t a = slot2[2 * (size_t)q], c = slot2[2 * (size_t)q + 1];
    const uint32_t key = ((base + (a >> 1)) << 1) | (a & 1u);
    const size_t s = (size_t)c * T.k;
    if (pat == T.pat[s + j] && top_open(B, T, c, key, j)) atomicMin(&T.key[s + j], key);
}

// the batch's sorted slots B merged into the call's G, one thread per read; B is left cleared.  Both lists are sorted and hold
// different targets, the batch's the higher indices: on an equal pattern G's entry stays ahead.  First the number of entries each
// side gives to the first k of the merged list, then the slots are written from the last to the first, so that no entry of G is
// overwritten before it is read (its new slot is never lower than its old one) and no list is held in registers.
__global__ __launch_bounds__(256) void top_merge_kernel(uint32_t nr, top_dev B, top_dev G) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const uint32_t k = G.k;
    const size_t s = (size_t)r * k;
    if (B.pat[s] == 0) return;                            // nothing accepted in this batch: its slots are as they were cleared
    uint32_t g = 0, b = 0;
    while (g + b < k) {
        const unsigned long long gp = g < k ? G.pat[s + g] : 0, bp = b < k ? B.pat[s + b] : 0;
        if (gp == 0 && bp == 0) break;
        if (gp >= bp) ++g; else ++b;
    }
    G.cnt[r] = g + b;
    for (uint32_t o = g + b; b > 0; --o) {                // (o - 1 >= g - 1: once b == 0 the rest of G is in place)
        if (g > 0 && G.pat[s + g - 1] < B.pat[s + b - 1]) {
            --g;
            G.pat[s + o - 1] = G.pat[s + g]; G.key[s + o - 1] = G.key[s + g]; G.ev[s + o - 1] = G.ev[s + g];
        } else {
            --b;
            G.pat[s + o - 1] = B.pat[s + b]; G.key[s + o - 1] = B.key[s + b]; G.ev[s + o - 1] = B.ev[s + b];
        }
    }
    for (uint32_t i = 0; i < k && B.pat[s + i] != 0; ++i) {
        B.pat[s + i] = 0; B.key[s + i] = 0xFFFFFFFFu; B.ev[s + i] = make_uint4(0, 0, 0, 0);
    }
}

int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string(what) + " launch: " + hipGetErrorString(e)); return RATTLE_ERR_HIP; }
    return 0;
}

}  // namespace

int assign_state::reserve(size_t nr) {
    RT_TRY(best.reserve(nr)); RT_TRY(second.reserve(nr)); RT_TRY(key.reserve(nr)); RT_TRY(n.reserve(nr)); RT_TRY(ev.reserve(nr));
    return 0;
}

int assign_state::clear(hipStream_t st, size_t nr) {
    RT_HIP(hipMemsetAsync(best.p, 0, nr * 8, st)); RT_HIP(hipMemsetAsync(second.p, 0, nr * 8, st));
    RT_HIP(hipMemsetAsync(key.p, 0xFF, nr * 4, st)); RT_HIP(hipMemsetAsync(n.p, 0, nr * 4, st));
    RT_HIP(hipMemsetAsync(ev.p, 0, nr * sizeof(uint4), st));
    return 0;
}

// the pairs are the kept pairs of the evaluation in flight (evaluator::run_local, after its full_pass): ctx->d_res / d_var / d_pi / d_pj / d_slot2
int launch_assign_max(rattle_ctx *ctx, uint32_t n, const uint32_t *d_remap, int use_hc, double t_s, double t_v, unsigned long long *d_out,
                      uint32_t *d_big, const assign_dev &B) {
    if (n == 0) return 0;
    ktimer T(ctx, K_ASSIGN, 0);
    hipLaunchKernelGGL(assign_max_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, d_remap, ctx->d_pi.p,
                       ctx->d_pj.p, ctx->d_slot2.p, ctx->idx.len.p, use_hc, t_s, t_v, d_out, d_big, B);
    return launched("assign (best score)");
}

int launch_assign_pick(rattle_ctx *ctx, uint32_t n, int use_hc, double t_s, double t_v, uint32_t target_base, const assign_dev &B) {
    if (n == 0) return 0;
    ktimer T(ctx, K_ASSIGN, 0);
    hipLaunchKernelGGL(assign_key_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, ctx->d_pi.p, ctx->d_pj.p,
                       ctx->d_slot2.p, ctx->idx.len.p, use_hc, t_s, t_v, target_base, B);
    RT_TRY(launched("assign (winner)"));
    hipLaunchKernelGGL(assign_second_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, ctx->d_pi.p, ctx->d_pj.p,
                       ctx->d_slot2.p, ctx->idx.len.p, use_hc, t_s, t_v, target_base, B);
    return launched("assign (runner-up)");
}

int launch_assign_merge(rattle_ctx *ctx, uint32_t nr, const assign_dev &B, const assign_dev &G) {
    if (nr == 0) return 0;
    ktimer T(ctx, K_ASSIGN, 0);
    hipLaunchKernelGGL(assign_merge_kernel, dim3((nr + 255) / 256), dim3(256), 0, ctx->stream, nr, B, G);
    return launched("assign (merge)");
}

int top_state::reserve(size_t nr, uint32_t k_) {
    k = k_;
    RT_TRY(pat.reserve(nr * k)); RT_TRY(key.reserve(nr * k)); RT_TRY(ev.reserve(nr * k)); RT_TRY(cnt.reserve(nr));
    return 0;
}

int top_state::clear(hipStream_t st, size_t nr) {
    RT_HIP(hipMemsetAsync(pat.p, 0, nr * k * 8, st)); RT_HIP(hipMemsetAsync(key.p, 0xFF, nr * k * 4, st));
    RT_HIP(hipMemsetAsync(ev.p, 0, nr * k * sizeof(uint4), st)); RT_HIP(hipMemsetAsync(cnt.p, 0, nr * 4, st));
    return 0;
}

// the batch's candidate list: the seed, then ranks 1 .. k - 1 in two launches each and one more for the last slot's evidence (2k
// launches, one if k == 1); no synchronisation in between, the stream orders them
int launch_assign_top(rattle_ctx *ctx, uint32_t n, uint32_t nr, int use_hc, double t_s, double t_v, uint32_t target_base, const assign_dev &B,
                      const top_dev &T) {
    if (n == 0 || nr == 0) return 0;
    const dim3 grid((n + 255) / 256), block(256);
    {
        ktimer K(ctx, K_ASSIGN, 0);
        hipLaunchKernelGGL(top_seed_kernel, dim3((nr + 255) / 256), block, 0, ctx->stream, nr, B, T);
        RT_TRY(launched("assign (candidates, slot 0)"));
    }
    for (uint32_t j = 1; j <= T.k && T.k > 1; ++j) {
        {
            ktimer K(ctx, K_ASSIGN, 0);
            hipLaunchKernelGGL(top_max_kernel, grid, block, 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, ctx->d_pi.p, ctx->d_pj.p, ctx->d_slot2.p,
                               ctx->idx.len.p, use_hc, t_s, t_v, target_base, j, B, T);
            RT_TRY(launched("assign (candidates, score)"));
        }
        if (j == T.k) break;
        ktimer K(ctx, K_ASSIGN, 0);
        hipLaunchKernelGGL(top_key_kernel, grid, block, 0, ctx->stream, ctx->d_res.p, ctx->d_var.p, n, ctx->d_pi.p, ctx->d_pj.p, ctx->d_slot2.p,
                           ctx->idx.len.p, use_hc, t_s, t_v, target_base, j, B, T);
        RT_TRY(launched("assign (candidates, target)"));
    }
    return 0;
}

int launch_assign_top_merge(rattle_ctx *ctx, uint32_t nr, const top_dev &TB, const top_dev &TG) {
    if (nr == 0) return 0;
    ktimer K(ctx, K_ASSIGN, 0);
    hipLaunchKernelGGL(top_merge_kernel, dim3((nr + 255) / 256), dim3(256), 0, ctx->stream, nr, TB, TG);
    return launched("assign (candidates, merge)");
}

}  // namespace rattle
