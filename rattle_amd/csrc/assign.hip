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

}  // namespace rattle
