// `abundance`: per-target read estimates by an expectation-maximisation over every read's compatible candidates (include/rattle_hip.h,
// "abundance"; DESIGN.md "abundance").  The rule is integer fixed point -- an abundance is a uint64 in units of 2^-32 read, a read hands
// out exactly 2^32 units per iteration -- so the M-step is a sum of integers and the rule of assign.hip holds here too: no step depends
// on the order in which the device adds, two runs give the same bits, and a plain-Python model (tests/abundance_ref.py) gives them too.
//
// Shape: the compatible targets of every read are uploaded once, -1 in every other slot, and laid out slot-major in the order the
// iterations walk the reads; then per iteration
//   step    one thread per read: A_cur of its up to 8 targets, D = their sum, share_j = floor(A_j / D * 2^32) for the slots j >= 1, the
//           rest of 2^32 to slot 0, every share added into A_next;
//   finish  one thread per target: atomicMax of |A_next - A_cur| into delta[i], and A_cur = 0: iteration i + 1 adds into it.
// There is no host round trip per iteration: every step and finish launch of iteration i reads delta[i - 1] first and returns at once if
// it is within the tolerance, so the converged state stays where it is (finish hands the small delta on to delta[i]), and the buffer
// that holds it follows from the iteration count alone.  The host enqueues iter_block iterations, reads their deltas, and stops
// enqueueing at the first small one; the result does not depend on iter_block.
//
// The skew: a handful of targets hold most reads, and a thread per read would pile its wavefront's 64 atomics on one address.  The reads
// are therefore walked in the order of their slot-0 target (a counting sort on the device: histogram, scan, scatter; the order inside a
// target is whatever the scatter's atomics give, integer sums do not care), and per slot the step kernel sums the shares of neighbouring
// lanes with the same target (a segmented scan over __shfl_up) so that the last lane of a run issues ONE atomicAdd for it; a wavefront
// that lies inside one run of slot 0 sums its later slots target by target across all its lanes (em_add_matched).
// RATTLE_EM_PLAIN=1 takes the reads as they come and issues one atomic per entry: the same bits, for the A/B measurement.
// No floating-point atomic, no wait on another wavefront; every loop is bounded by k, the wavefront size, max_iters or the input's size.
#include "common.h"

namespace rattle {

namespace {

constexpr unsigned long long EM_ONE = 1ull << 32;
constexpr uint32_t EM_K = 8;                    // slots per read at the most

int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string(what) + " launch: " + hipGetErrorString(e)); return RATTLE_ERR_HIP; }
    return 0;
}

// the sort key of read r: its slot-0 target; a read that takes no part goes behind every target
__device__ __forceinline__ uint32_t em_key(const int32_t *__restrict__ in, uint32_t r, uint32_t k, uint32_t nt) {
    const int32_t t = in[(size_t)r * k];
    return t < 0 ? nt : (uint32_t)t;
}

__global__ __launch_bounds__(256) void em_hist_kernel(const int32_t *__restrict__ in, uint32_t n, uint32_t k, uint32_t nt, uint32_t *__restrict__ hist) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) atomicAdd(&hist[em_key(in, r, k, nt)], 1u);
}

// exclusive scan of hist[0, m) in place, one workgroup, 1024 entries per round
__global__ __launch_bounds__(1024) void em_scan_kernel(uint32_t *__restrict__ hist, uint32_t m) {
    __shared__ uint32_t s[1024];
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < m; i0 += 1024) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < m ? hist[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint32_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < m) hist[i] = base + s[threadIdx.x] - v;
        base += s[1023];
        __syncthreads();
    }
}

// read r to its position p: src[p] = r, slot j at tgt[j * n + p].  cursor: the scan above (sorted), or null: p = r
__global__ __launch_bounds__(256) void em_place_kernel(const int32_t *__restrict__ in, uint32_t n, uint32_t k, uint32_t nt, uint32_t *__restrict__ cursor,
                                                       int32_t *__restrict__ tgt, uint32_t *__restrict__ src) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t p = cursor ? atomicAdd(&cursor[em_key(in, r, k, nt)], 1u) : r;
    src[p] = r;
    for (uint32_t j = 0; j < k; ++j) tgt[(size_t)j * n + p] = in[(size_t)r * k + j];
}

// the start: ONE / c to every compatible slot j >= 1, the rest of ONE to slot 0; compatible_reads counts a read once per target
__global__ __launch_bounds__(256) void em_init_kernel(const int32_t *__restrict__ tgt, uint32_t n, uint32_t k, unsigned long long *__restrict__ A,
                                                      uint32_t *__restrict__ compat) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int32_t t[EM_K];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < EM_K; ++j) { t[j] = j < k ? tgt[(size_t)j * n + p] : -1; c += t[j] >= 0; }
    if (t[0] < 0) return;
    const unsigned long long s = EM_ONE / c;
#pragma unroll
    for (uint32_t j = 0; j < EM_K; ++j) {
        if (t[j] < 0) continue;
        atomicAdd(&A[t[j]], j == 0 ? EM_ONE - s * (c - 1) : s);
        bool first = true;
#pragma unroll
        for (uint32_t i = 0; i < j; ++i) first = first && t[i] != t[j];
        if (first) atomicAdd(&compat[t[j]], 1u);
    }
}

// the E-step of position p at the state A: its targets and what each gets of the read's ONE (0 for a slot that is not compatible)
__device__ __forceinline__ void em_shares(const int32_t *__restrict__ tgt, uint32_t n, uint32_t k, uint32_t p, const unsigned long long *__restrict__ A,
                                          int32_t (&t)[EM_K], unsigned long long (&sh)[EM_K]) {
    unsigned long long a[EM_K], D = 0;
#pragma unroll
    for (uint32_t j = 0; j < EM_K; ++j) {
        t[j] = (j < k && p < n) ? tgt[(size_t)j * n + p] : -1;
        a[j] = t[j] >= 0 ? A[t[j]] : 0;
        D += a[j];
    }
    const double dD = (double)D;
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t j = 1; j < EM_K; ++j) {
        sh[j] = t[j] >= 0 ? (unsigned long long)((double)a[j] / dD * 4294967296.0) : 0;
        sum += sh[j];
    }
    sh[0] = (t[0] >= 0 && sum < EM_ONE) ? EM_ONE - sum : 0;
}

// v of every lane added into A[t] (t < 0: nothing), one atomic per run of neighbouring lanes with the same t.  Called by all 64 lanes.
__device__ __forceinline__ void em_add_merged(unsigned long long *__restrict__ A, int32_t t, unsigned long long v, int lane) {
    const int32_t before = __shfl_up(t, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || before != t);      // bit 0 is always set
    if (heads != ~0ull) {
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(v, d, 64);
            if (lane - d >= start) v += up;
        }
    }
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (tail && t >= 0) atomicAdd(&A[t], v);
}

// the same for a wavefront whose reads all have the same best target: their later slots name the few members of one family in any order,
// equal targets are seldom neighbours, and the wavefront's adds would still queue on those few addresses.  EM_ROUNDS times the first
// lane still to add names its target, the lanes with that target are summed across the wavefront and that lane issues one atomicAdd
// for them; what is left after the rounds adds for itself.  Called by all 64 lanes; every loop is bounded.
constexpr int EM_ROUNDS = 8;
__device__ __forceinline__ void em_add_matched(unsigned long long *__restrict__ A, int32_t t, unsigned long long v, int lane) {
    unsigned long long todo = __ballot(t >= 0);
    for (int round = 0; round < EM_ROUNDS && todo; ++round) {               // (todo is the same in every lane)
        const int first = __ffsll((long long)todo) - 1;
        const int32_t tt = __shfl(t, first, 64);
        unsigned long long s = t == tt ? v : 0;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == first) atomicAdd(&A[tt], s);
        todo &= ~__ballot(t == tt);
    }
    if ((todo >> lane) & 1ull) atomicAdd(&A[t], v);
}

// one E/M round trip, A_cur -> A_next (cleared by the finish before).  prev: the delta of the iteration before (all ones in front of
// the first); within tol, the state is final and nothing is done
template <bool MERGE>
__global__ __launch_bounds__(256) void em_step_kernel(const int32_t *__restrict__ tgt, uint32_t n, uint32_t k, const unsigned long long *__restrict__ prev,
                                                      unsigned long long tol, const unsigned long long *__restrict__ A_cur,
                                                      unsigned long long *__restrict__ A_next) {
    if (*prev <= tol) return;
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t t[EM_K];
    unsigned long long sh[EM_K];
    em_shares(tgt, n, k, p, A_cur, t, sh);
    const int lane = threadIdx.x & 63;
    const bool one_best = MERGE && __ballot(t[0] != __shfl(t[0], 0, 64)) == 0;      // the whole wavefront inside one run of slot 0
#pragma unroll
    for (uint32_t j = 0; j < EM_K; ++j) {
        if (j >= k) break;                                                     // (uniform)
        if (MERGE && j > 0 && one_best) em_add_matched(A_next, t[j], sh[j], lane);
        else if (MERGE) em_add_merged(A_next, t[j], sh[j], lane);
        else if (t[j] >= 0) atomicAdd(&A_next[t[j]], sh[j]);
    }
}

// delta[i] = max |A_next - A_cur|, and A_cur cleared for the next iteration's sums.  A stopped run hands its delta on
__global__ __launch_bounds__(256) void em_finish_kernel(uint32_t nt, const unsigned long long *__restrict__ prev, unsigned long long tol,
                                                        unsigned long long *__restrict__ delta, unsigned long long *__restrict__ A_cur,
                                                        const unsigned long long *__restrict__ A_next) {
    const unsigned long long dp = *prev;
    if (dp <= tol) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *delta = dp;
        return;
    }
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long d = 0;
    if (t < nt) {
        const unsigned long long a = A_cur[t], b = A_next[t];
        d = a > b ? a - b : b - a;
        A_cur[t] = 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(d, o, 64);
        d = other > d ? other : d;
    }
    if ((threadIdx.x & 63) == 0 && d) atomicMax(delta, d);
}

// the posterior: one more E-step at the final state, written in the caller's read order
__global__ __launch_bounds__(256) void em_posterior_kernel(const int32_t *__restrict__ tgt, const uint32_t *__restrict__ src, uint32_t n, uint32_t k,
                                                           const unsigned long long *__restrict__ A, double *__restrict__ post) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int32_t t[EM_K];
    unsigned long long sh[EM_K];
    em_shares(tgt, n, k, p, A, t, sh);
    const size_t o = (size_t)src[p] * k;
#pragma unroll
    for (uint32_t j = 0; j < EM_K; ++j) if (j < k) post[o + j] = (double)sh[j] / 4294967296.0;
}

}  // namespace

int abundance_run(rattle_ctx *ctx, const int32_t *h_tgt, uint32_t n, uint32_t k, uint32_t nt, unsigned long long tol_units, uint32_t max_iters,
                  uint32_t iter_block, rattle_abundance *R, std::vector<uint64_t> &deltas) {
    const bool plain = getenv("RATTLE_EM_PLAIN") && atoi(getenv("RATTLE_EM_PLAIN")) != 0;
    const size_t slots = (size_t)n * k;
    const uint32_t block = std::min(std::min(iter_block ? iter_block : 32u, max_iters), 1u << 16);
    hipStream_t st = ctx->stream;
    dbuf<int32_t> d_in, d_tgt;
    dbuf<uint32_t> d_src, d_hist, d_compat;
    dbuf<unsigned long long> d_A[2], d_delta;
    dbuf<double> d_post;
    hbuf<unsigned long long> h_delta;
    RT_TRY(d_in.reserve(slots)); RT_TRY(d_tgt.reserve(slots)); RT_TRY(d_src.reserve(n)); RT_TRY(d_hist.reserve((size_t)nt + 1));
    RT_TRY(d_compat.reserve(nt)); RT_TRY(d_A[0].reserve(nt)); RT_TRY(d_A[1].reserve(nt)); RT_TRY(d_delta.reserve((size_t)block + 1));
    RT_TRY(d_post.reserve(slots)); RT_TRY(h_delta.reserve(block));
    RT_HIP(hipMemcpyAsync(d_in.p, h_tgt, slots * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemsetAsync(d_compat.p, 0, (size_t)nt * 4, st));
    RT_HIP(hipMemsetAsync(d_A[0].p, 0, (size_t)nt * 8, st)); RT_HIP(hipMemsetAsync(d_A[1].p, 0, (size_t)nt * 8, st));
    RT_HIP(hipMemsetAsync(d_delta.p, 0xFF, 8, st));                          // in front of the first iteration: nothing has converged
    const dim3 g_reads((n + 255) / 256), g_targets((nt + 255) / 256), wg(256);
    {
        ktimer T(ctx, K_ABUNDANCE, slots * 8);
        if (!plain) {
            RT_HIP(hipMemsetAsync(d_hist.p, 0, ((size_t)nt + 1) * 4, st));
            hipLaunchKernelGGL(em_hist_kernel, g_reads, wg, 0, st, d_in.p, n, k, nt, d_hist.p);
            RT_TRY(launched("abundance (histogram)"));
            hipLaunchKernelGGL(em_scan_kernel, dim3(1), dim3(1024), 0, st, d_hist.p, nt + 1);
            RT_TRY(launched("abundance (scan)"));
            ctx->stats[K_ABUNDANCE].launches += 2;
        }
        hipLaunchKernelGGL(em_place_kernel, g_reads, wg, 0, st, d_in.p, n, k, nt, plain ? nullptr : d_hist.p, d_tgt.p, d_src.p);
        RT_TRY(launched("abundance (order)"));
        hipLaunchKernelGGL(em_init_kernel, g_reads, wg, 0, st, d_tgt.p, n, k, d_A[0].p, d_compat.p);
        RT_TRY(launched("abundance (start)"));
        ctx->stats[K_ABUNDANCE].launches += 1;
    }
    // the iterations, `block` of them per visit of the host
    deltas.clear();
    bool converged = false;
    uint32_t done = 0;
    while (done < max_iters && !converged) {
        const uint32_t B = std::min(block, max_iters - done);
        if (done) RT_HIP(hipMemcpyAsync(d_delta.p, d_delta.p + block, 8, hipMemcpyDeviceToDevice, st));      // (every block before the last is full)
        RT_HIP(hipMemsetAsync(d_delta.p + 1, 0, (size_t)B * 8, st));
        {
            ktimer T(ctx, K_ABUNDANCE, (uint64_t)B * (slots * 12 + (uint64_t)nt * 24));
            for (uint32_t b = 0; b < B; ++b) {
                unsigned long long *cur = d_A[(done + b) & 1].p, *next = d_A[(done + b + 1) & 1].p;
                if (plain) hipLaunchKernelGGL(em_step_kernel<false>, g_reads, wg, 0, st, d_tgt.p, n, k, d_delta.p + b, tol_units, cur, next);
                else hipLaunchKernelGGL(em_step_kernel<true>, g_reads, wg, 0, st, d_tgt.p, n, k, d_delta.p + b, tol_units, cur, next);
                RT_TRY(launched("abundance (step)"));
                hipLaunchKernelGGL(em_finish_kernel, g_targets, wg, 0, st, nt, d_delta.p + b, tol_units, d_delta.p + b + 1, cur, next);
                RT_TRY(launched("abundance (finish)"));
            }
            ctx->stats[K_ABUNDANCE].launches += 2 * (uint64_t)B - 1;
        }
        RT_HIP(hipMemcpyAsync(h_delta.p, d_delta.p + 1, (size_t)B * 8, hipMemcpyDeviceToHost, st));
        RT_HIP(hipStreamSynchronize(st));
        for (uint32_t b = 0; b < B && !converged; ++b) {
            deltas.push_back(h_delta.p[b]);
            converged = h_delta.p[b] <= tol_units;
        }
        done += B;
    }
    R->iterations = (uint32_t)deltas.size();
    R->converged = converged ? 1 : 0;
    const unsigned long long *A = d_A[deltas.size() & 1].p;                  // iteration i reads buffer i & 1 and leaves its result in the other
    {
        ktimer T(ctx, K_ABUNDANCE, slots * 12);
        hipLaunchKernelGGL(em_posterior_kernel, g_reads, wg, 0, st, d_tgt.p, d_src.p, n, k, A, d_post.p);
        RT_TRY(launched("abundance (posterior)"));
    }
    RT_HIP(hipMemcpyAsync(R->units, A, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(R->compatible_reads, d_compat.p, (size_t)nt * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipMemcpyAsync(R->posterior, d_post.p, slots * 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace rattle
