// Kernel B, count pass, "index": an exact inverted index on the k-mers of the SEEDS of one evaluation.
//
// |common| (kmer.cpp:45-67: the full cross product on repeated hashes) = sum over the candidate's k-mers b of the number of
// times hash(b) occurs in the seed.  The two other forms (pair_count.hip, pair_score.hip) stream a candidate's hash list once
// per surviving PAIR; where the bit-vector filter saturates (reads of several kb) that is once per seed of the batch.  Here the
// seeds' forward hash lists are turned into a CSR table bucket -> seed slots (a seed that holds a hash m times appears m times
// in its bucket), and a candidate's list is streamed ONCE per strand: one bucket lookup per k-mer and one LDS increment per
// seed that really holds that hash.  The sum of increments is the cross product; there is no repeat list and so no overflow rule.
//
// Semantics of the count:
//   k <= 10: the bucket is the hash itself (4^k <= 2^20 buckets): exactly |common|.
//   k >  10: the bucket is the 20-bit fold pair_count.hip uses, (h ^ h >> 20) & 0xFFFFF: the sum over the candidate's k-mers b
//            of the multiplicity of fold(hash(b)) among the seed's folded hashes -- an UPPER bound of |common|, which is all the
//            caller's exact rejection needs (cluster_driver.hip: pairs that pass it go through the reference's full comparison).
// Counts saturate at INT32_MAX like the seed-major form's.
//
// Steps, all on the context's stream, in buffers the context keeps and grows by high-water mark:
//   group   the survivor list is grouped by candidate slot (counting sort keyed on the second word; the rest of the evaluation
//           reads whatever order d_surv has, as after the seed-major sort)
//   build   histogram of the buckets over the seed slots, exclusive scan, scatter
//   count   one wavefront per (candidate, strand) with at least one survivor: the lanes take the candidate's k-mers, read the
//           bucket range and add 1 to a per-wavefront counter array in LDS indexed by seed slot (PIX_SEEDS counters; a
//           rectangle with more seeds is handled in seed chunks, one pass over the candidate's list per chunk)
//   deliver the wavefront walks the candidate's survivors and writes the counter of each one's seed to d_res
// A bucket holds the seeds of EVERY rectangle of the evaluation; a candidate only counts the entries inside the seed range of
// its own rectangle (the chunk test), so a seed is never counted for a candidate of another rectangle.
//
// Device memory: 4 B x (buckets + 2) + 4 B per indexed seed k-mer, the survivor double buffer the seed-major sort also uses,
// and 4 B per candidate slot.  The indexed k-mers of one build are capped (PIX_MAX_ENTRIES, 2^27 = 512 MB;
// RATTLE_INDEX_ENTRIES overrides it): an evaluation whose seeds hold more is done in several ranges of seed slots, one build +
// count each; every survivor's seed lies in exactly one range.
#include <algorithm>
#include <cstring>

#include "common.h"

namespace rattle {

#define PIX_SEEDS 1024u                  // LDS counters per wavefront
#define PIX_SCAN 1024u                   // elements per workgroup of the scan
#define PIX_MAX_ENTRIES (1ull << 27)

struct pix_args {
    const uint2 *surv;           // [n] (seed_slot << 1 | strand, cand_slot), grouped by candidate slot
    const uint32_t *coff;        // [nc + 1] survivor range of every candidate slot
    const uint32_t *seed_rect;   // rectangle of a seed slot, or nullptr (one rectangle)
    const bvf_rect *rects;
    const uint32_t *cand_ids;
    const uint32_t *kh[2];       // per strand: hash lists
    const uint64_t *koff;
    const uint32_t *boff;        // [buckets + 1] entry range of every bucket
    const uint32_t *ent;         // seed slots, bucket after bucket
    uint64_t n_items;            // candidate slots x strands
    uint32_t strands, bmask, folded;
    uint32_t r0, r1;             // seed slots this index holds
    int32_t *res;                // [n] count per survivor
};

__device__ __forceinline__ uint32_t pix_bucket(uint32_t h, uint32_t folded, uint32_t bmask) {
    return (folded ? h ^ (h >> 20) : h) & bmask;
}

// ---- build: histogram (SCATTER = false) and scatter (true) of the seeds' k-mers over the buckets; one seed slot per workgroup turn
template <bool SCATTER>
__global__ __launch_bounds__(256) void pix_bucket_kernel(const uint32_t *__restrict__ seed_ids, const uint64_t *__restrict__ koff,
                                                         const uint32_t *__restrict__ uh, uint32_t s0, uint32_t s1, uint32_t folded,
                                                         uint32_t bmask, uint32_t *__restrict__ cursor, uint32_t *__restrict__ ent) {
    for (uint64_t slot = (uint64_t)s0 + blockIdx.x; slot < s1; slot += gridDim.x) {
        const uint32_t ri = seed_ids[slot];
        const uint64_t o0 = koff[ri];
        const uint32_t n = (uint32_t)(koff[ri + 1] - o0);
        const uint32_t *__restrict__ h = uh + o0;
        for (uint32_t t = threadIdx.x; t < n; t += 256) {
            const uint32_t f = pix_bucket(h[t], folded, bmask);
            if (SCATTER) ent[atomicAdd(&cursor[f], 1u)] = (uint32_t)slot;
            else atomicAdd(&cursor[f], 1u);
        }
    }
}

// ---- exclusive scan of a[0 .. n) in place: per workgroup, then the workgroup totals, then the offsets added back
__global__ __launch_bounds__(PIX_SCAN) void pix_scan_block_kernel(uint32_t *__restrict__ a, uint32_t n, uint32_t *__restrict__ bsum) {
    __shared__ uint32_t wtot[PIX_SCAN / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * PIX_SCAN + tid;
    const uint32_t v = i < n ? a[i] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += o; }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; ++w) base += wtot[w];
    if (i < n) a[i] = base + incl - v;
    if (tid == PIX_SCAN - 1) bsum[blockIdx.x] = base + incl;
}

__global__ __launch_bounds__(PIX_SCAN) void pix_scan_top_kernel(uint32_t *__restrict__ bsum, uint32_t nb) {
    __shared__ uint32_t wtot[PIX_SCAN / 64];
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += PIX_SCAN) {
        const uint32_t i = b0 + tid;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += o; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t base = carry;
        for (uint32_t w = 0; w < wave; ++w) base += wtot[w];
        if (i < nb) bsum[i] = base + incl - v;
        __syncthreads();
        if (tid == PIX_SCAN - 1) carry = base + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PIX_SCAN) void pix_scan_add_kernel(uint32_t *__restrict__ a, uint32_t n, const uint32_t *__restrict__ bsum) {
    const uint64_t i = (uint64_t)blockIdx.x * PIX_SCAN + threadIdx.x;
    if (i < n) a[i] += bsum[blockIdx.x];
}

static int pix_scan(rattle_ctx *ctx, uint32_t *a, uint32_t n) {
    if (n == 0) return 0;
    const uint32_t nb = (uint32_t)(((uint64_t)n + PIX_SCAN - 1) / PIX_SCAN);
    RT_TRY(ctx->d_ix_bsum.reserve(nb));
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(pix_scan_block_kernel, dim3(nb), dim3(PIX_SCAN), 0, st, a, n, ctx->d_ix_bsum.p);
    if (nb > 1) {
        hipLaunchKernelGGL(pix_scan_top_kernel, dim3(1), dim3(PIX_SCAN), 0, st, ctx->d_ix_bsum.p, nb);
        hipLaunchKernelGGL(pix_scan_add_kernel, dim3(nb), dim3(PIX_SCAN), 0, st, a, n, (const uint32_t *)ctx->d_ix_bsum.p);
    }
    RT_HIP(hipGetLastError());
    return 0;
}

// ---- group: the survivors by candidate slot
__global__ __launch_bounds__(256) void pix_cand_hist_kernel(const uint2 *__restrict__ surv, uint32_t n, uint32_t *__restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&count[surv[i].y], 1u);
}

__global__ __launch_bounds__(256) void pix_cand_scatter_kernel(const uint2 *__restrict__ surv, uint32_t n, uint32_t *__restrict__ cursor,
                                                               uint2 *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 e = surv[i];
    out[atomicAdd(&cursor[e.y], 1u)] = e;
}

// group the survivor list (ctx->d_surv, n entries of two words) by candidate slot; afterwards the survivors of slot c are
// entries [coff[c], coff[c + 1]) with coff = ctx->d_ix_coff
int group_survivors_by_cand(rattle_ctx *ctx, uint32_t n, uint64_t n_cands) {
    if (n_cands >= 0xFFFFFFF0ull) { set_error("survivor grouping: too many candidates"); return RATTLE_ERR_ARG; }
    const uint32_t nc = (uint32_t)n_cands;
    RT_TRY(ctx->d_surv2.reserve((size_t)n * 2));
    RT_TRY(ctx->d_ix_coff.reserve((size_t)nc + 2));
    // coff[0] stays 0; the cursors are coff + 1: the scan leaves the start of slot c in coff[c + 1] and the scatter moves it to
    // the end of slot c, which is the start of slot c + 1
    uint32_t *coff = ctx->d_ix_coff.p;
    hipStream_t st = ctx->stream;
    ktimer T(ctx, K_SCORE, 0);                   // the grouping is part of this form's cost
    RT_HIP(hipMemsetAsync(coff, 0, ((size_t)nc + 2) * 4, st));
    const uint32_t blocks = (n + 255u) / 256u;
    if (n) hipLaunchKernelGGL(pix_cand_hist_kernel, dim3(blocks), dim3(256), 0, st, (const uint2 *)ctx->d_surv.p, n, coff + 1);
    RT_TRY(pix_scan(ctx, coff + 1, nc));
    if (n) hipLaunchKernelGGL(pix_cand_scatter_kernel, dim3(blocks), dim3(256), 0, st, (const uint2 *)ctx->d_surv.p, n, coff + 1, (uint2 *)ctx->d_surv2.p);
    RT_HIP(hipGetLastError());
    ctx->d_surv.swap(ctx->d_surv2);
    return 0;
}

// ---- count + deliver: one wavefront (= one workgroup) per (candidate slot, strand)
__global__ __launch_bounds__(64) void pair_count_index_kernel(pix_args A) {
    __shared__ uint32_t cnt[PIX_SEEDS];
    const uint32_t lane = threadIdx.x;
    for (uint64_t item = blockIdx.x; item < A.n_items; item += gridDim.x) {
        const uint32_t c = (uint32_t)(A.strands == 2 ? item >> 1 : item), strand = A.strands == 2 ? (uint32_t)item & 1u : 0u;
        const uint32_t p0 = A.coff[c], p1 = A.coff[c + 1];
        if (p0 == p1) continue;                                  // no survivor: the list is not read
        // all survivors of a candidate slot have their seeds in the slot's own rectangle
        const uint32_t rect = A.seed_rect ? A.seed_rect[A.surv[p0].x >> 1] : 0u;
        const uint32_t sb = A.rects[rect].s_base, se = sb + A.rects[rect].ns;
        const uint32_t lo = max(sb, A.r0), hi = min(se, A.r1);
        const uint32_t rj = A.cand_ids[c];
        const uint64_t o0 = A.koff[rj];
        const uint32_t nB = (uint32_t)(A.koff[rj + 1] - o0);
        const uint32_t *__restrict__ bh = A.kh[strand] + o0;
        const uint32_t *__restrict__ boff = A.boff;
        const uint32_t *__restrict__ ent = A.ent;
        for (uint32_t cb = lo; cb < hi; cb += PIX_SEEDS) {       // (wave-uniform: the barriers below are met by all lanes)
            const uint32_t cn = min(PIX_SEEDS, hi - cb);
            bool mine = false;
            for (uint32_t p = p0 + lane; p < p1; p += 64) {
                const uint32_t a = A.surv[p].x;
                mine |= (a & 1u) == strand && (a >> 1) - cb < cn;
            }
            if (!__any(mine)) continue;
            for (uint32_t i = lane; i < cn; i += 64) cnt[i] = 0;
            __syncthreads();
            auto walk = [&](uint32_t e, uint32_t e1) {
                for (; e < e1; ++e) {
                    const uint32_t d = ent[e] - cb;
                    if (d < cn) atomicAdd(&cnt[d], 1u);
                }
            };
            uint32_t t = lane;
            for (; t + 192 < nB; t += 256) {                     // four lists' bucket ranges in flight per lane
                const uint32_t f0 = pix_bucket(bh[t], A.folded, A.bmask), f1 = pix_bucket(bh[t + 64], A.folded, A.bmask);
                const uint32_t f2 = pix_bucket(bh[t + 128], A.folded, A.bmask), f3 = pix_bucket(bh[t + 192], A.folded, A.bmask);
                const uint32_t a0 = boff[f0], b0 = boff[f0 + 1], a1 = boff[f1], b1 = boff[f1 + 1];
                const uint32_t a2 = boff[f2], b2 = boff[f2 + 1], a3 = boff[f3], b3 = boff[f3 + 1];
                walk(a0, b0); walk(a1, b1); walk(a2, b2); walk(a3, b3);
            }
            for (; t < nB; t += 64) {
                const uint32_t f = pix_bucket(bh[t], A.folded, A.bmask);
                walk(boff[f], boff[f + 1]);
            }
            __syncthreads();
            for (uint32_t p = p0 + lane; p < p1; p += 64) {
                const uint32_t a = A.surv[p].x, d = (a >> 1) - cb;
                if ((a & 1u) == strand && d < cn) A.res[p] = (int32_t)min(cnt[d], 0x7FFFFFFFu);
            }
            __syncthreads();                                     // the counters are cleared for the next chunk
        }
    }
}

// survivors in ctx->d_surv grouped by candidate (group_survivors_by_cand), seeds / candidates / rectangles in ctx->d_seed /
// d_cand / d_rect (and d_seed_rect when many): the count of each survivor into ctx->d_res[survivor].  h_seed: the host's copy
// of the seed slots' read ids.
int launch_pair_count_index(rattle_ctx *ctx, uint32_t n_pairs, const uint32_t *h_seed, uint32_t ns, uint32_t nc, bool many) {
    if (n_pairs == 0) return 0;
    read_index &X = ctx->idx;
    static const uint64_t max_entries = [] {
        const char *e = getenv("RATTLE_INDEX_ENTRIES");
        const long long v = e ? atoll(e) : 0;
        return v > 0 ? (uint64_t)std::min<long long>(v, 0x7FFFFFFFll) : (uint64_t)PIX_MAX_ENTRIES;
    }();
    const int bits = 2 * X.k < 20 ? 2 * X.k : 20;
    const uint32_t nb = 1u << bits;
    hipStream_t st = ctx->stream;
    pix_args A;
    A.surv = (const uint2 *)ctx->d_surv.p; A.coff = ctx->d_ix_coff.p;
    A.seed_rect = many ? ctx->d_seed_rect.p : nullptr; A.rects = ctx->d_rect.p; A.cand_ids = ctx->d_cand.p;
    A.kh[0] = X.kh[0].p; A.kh[1] = X.kh[1].p; A.koff = X.koff.p;
    A.strands = X.both ? 2u : 1u; A.n_items = (uint64_t)nc * A.strands;
    A.bmask = nb - 1u; A.folded = 2 * X.k > 20 ? 1u : 0u;
    A.res = ctx->d_res.p;
    RT_TRY(ctx->d_ix_boff.reserve((size_t)nb + 2));
    ktimer T(ctx, K_SCORE, 0);
    uint32_t r0 = 0;
    while (r0 < ns) {
        // the next range of seed slots: as many as the entry cap holds (at least one)
        uint64_t tot = 0;
        uint32_t r1 = r0;
        while (r1 < ns) {
            const uint64_t m = X.h_koff[(size_t)h_seed[r1] + 1] - X.h_koff[h_seed[r1]];
            if (r1 > r0 && tot + m > max_entries) break;
            tot += m; ++r1;
        }
        if (tot >= 0xFFFFFFF0ull) { set_error("pair_count_index: a seed holds too many k-mers"); return RATTLE_ERR_ARG; }
        RT_TRY(ctx->d_ix_ent.reserve((size_t)tot));
        uint32_t *boff = ctx->d_ix_boff.p;
        RT_HIP(hipMemsetAsync(boff, 0, ((size_t)nb + 2) * 4, st));
        const uint32_t blocks = std::min<uint32_t>(r1 - r0, 65536u);
        hipLaunchKernelGGL((pix_bucket_kernel<false>), dim3(blocks), dim3(256), 0, st, (const uint32_t *)ctx->d_seed.p, (const uint64_t *)X.koff.p,
                           (const uint32_t *)X.uh.p, r0, r1, A.folded, A.bmask, boff + 1, ctx->d_ix_ent.p);
        RT_TRY(pix_scan(ctx, boff + 1, nb));
        hipLaunchKernelGGL((pix_bucket_kernel<true>), dim3(blocks), dim3(256), 0, st, (const uint32_t *)ctx->d_seed.p, (const uint64_t *)X.koff.p,
                           (const uint32_t *)X.uh.p, r0, r1, A.folded, A.bmask, boff + 1, ctx->d_ix_ent.p);
        A.boff = boff; A.ent = ctx->d_ix_ent.p; A.r0 = r0; A.r1 = r1;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(A.n_items, 1u << 20);
        hipLaunchKernelGGL(pair_count_index_kernel, dim3(grid), dim3(64), 0, st, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error(std::string("pair_count_index launch: ") + hipGetErrorString(e)); return RATTLE_ERR_HIP; }
        r0 = r1;
    }
    return 0;
}

}  // namespace rattle
