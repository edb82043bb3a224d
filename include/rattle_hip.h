/*
 * rattle_hip.h -- C ABI of librattle_hip.so, the MI355X (gfx950) implementation of
 * RATTLE's `cluster` + `correct` hot path.
 *
 * RATTLE has no FFI / plugin interface: the seams are the C++ functions
 *   cluster_reads(...)   /root/reference/cluster.hpp:44   (called at main.cpp:258,300,669)
 *   correct_reads(...)   /root/reference/correct.hpp:44   (called at main.cpp:405,670)
 * This header is the C boundary a maintainer binds underneath those two functions
 * (INTEGRATION.md shows the binding).  Plain pointers and sizes only; no C++ or torch
 * types.  All functions return 0 on success and a negative code on error, with text
 * available from rattle_hip_last_error().  Nothing throws across the boundary.
 * Input buffers are caller-owned; result objects are library-owned and released with
 * the matching *_free function.  One host thread drives one context.
 *
 * Every entry point REQUIRES a HIP device: there is no CPU fallback.
 */
#ifndef RATTLE_HIP_H
#define RATTLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RATTLE_OK 0
#define RATTLE_ERR_HIP (-1)       /* a HIP runtime call failed (no device, OOM, launch error) */
#define RATTLE_ERR_ARG (-2)       /* invalid argument (bad base in a read, k out of range, ...) */
#define RATTLE_ERR_STATE (-3)     /* call order violated (e.g. no reads loaded) */

typedef struct rattle_ctx rattle_ctx;

const char *rattle_hip_last_error(void);
int rattle_hip_abi_version(void);

/* Context = one HIP device + its streams and device-resident read index. */
int rattle_hip_ctx_create(int device, rattle_ctx **out);
/* A context WITHOUT a device, for a coordinating process and for CPU tests of the sharding: only
 * rattle_hip_set_exchange and rattle_hip_correction_gather work on it; every compute entry point returns
 * RATTLE_ERR_STATE (there is still no CPU path for the kernels). */
int rattle_hip_ctx_create_host(rattle_ctx **out);
void rattle_hip_ctx_destroy(rattle_ctx *ctx);

/* ------------------------------------------------------------------------------------
 * a3  extract_kmers_from_read   /root/reference/kmer.cpp:6-42, kmer.hpp:25-40
 * Uploads n reads (ASCII A/C/G/T/U, concatenated; offsets has n+1 entries) and builds on
 * the device, per read: the 4096-bit 6-mer bit-vector(s) (kmer.hpp:14-16), and the
 * (hash,pos)-sorted k-mer list(s) with L-k entries.  both_strands = !is_rna.
 * Replaces any previously loaded read set.  Reads must be given in PROCESSING order
 * (cluster_reads consumes them length-descending, main.cpp:254).
 */
int rattle_hip_load_reads(rattle_ctx *ctx, const uint8_t *seq_concat, const uint64_t *offsets, uint32_t n_reads,
                          int kmer_size, int both_strands);

/* Read back one read's index (tests): hash/pos need max(L-k,0) entries, bv 64 words. */
int rattle_hip_get_read_index(rattle_ctx *ctx, uint32_t read, int strand, uint32_t *hash_out, int32_t *pos_out,
                              uint64_t *bv_out, uint32_t *bv_popcount);

/* ------------------------------------------------------------------------------------
 * a4  bit-vector filter of cluster_together   /root/reference/cluster.cpp:13-19,43
 * For every (seed s, candidate c) with c >= first_cand[s]:
 *   common_f = popcount(bv_f[seed] & bv_f[cand]); common_r = popcount(bv_f[seed] & bv_r[cand])
 *   mmax = max(popcount(bv_f[seed]), popcount(bv_f[cand]))
 *   bit0 = fwd_bypass || common_f >= min_common_lut[mmax]
 *   bit1 = both_strands && common_r >= min_common_lut[mmax]
 * min_common_lut[m] (4097 entries) is the smallest c with double(c)/double(m) >= thr
 * evaluated by the caller in the reference's own double arithmetic (0xFFFF = never).
 * out_pass is n_seeds*n_cands bytes, row-major by seed.
 */
int rattle_hip_bv_filter(rattle_ctx *ctx, const uint32_t *seed_ids, uint32_t n_seeds, const uint32_t *cand_ids,
                         uint32_t n_cands, const uint32_t *first_cand, const uint16_t *min_common_lut, int fwd_bypass,
                         uint8_t *out_pass);

/* ------------------------------------------------------------------------------------
 * a5+a6+a7  get_common_kmers + calc_similarity + var
 *           /root/reference/kmer.cpp:45-67, similarity.cpp:4-97, utils.cpp:36-55
 * For each pair p: read i_ids[p] (forward list) against read j_ids[p] (forward list if
 * strand[p]==0, reverse-complement list otherwise).  Outputs per pair: bases, hc_bases,
 * n_dist = distances.size(), variance = var(distances) (IEEE double, same operation order
 * as the reference; NaN for n_dist==1), n_matches = common.size().
 */
int rattle_hip_pair_score(rattle_ctx *ctx, const uint32_t *i_ids, const uint32_t *j_ids, const uint8_t *strand,
                          uint32_t n_pairs, int32_t *bases, int32_t *hc_bases, int32_t *n_dist, double *variance,
                          int32_t *n_matches);

/* ------------------------------------------------------------------------------------
 * a8-a11  cluster_reads   /root/reference/cluster.cpp:93-259 (signature cluster.hpp:44)
 * Runs on the reads loaded by rattle_hip_load_reads (kmer_size / strands taken from there).
 * min_reads_cluster, use_hc and verbose of the reference signature are accepted and
 * ignored exactly as the reference ignores / never sets them (cluster.cpp:242-243).
 */
typedef struct {
    double t_s, t_v;
    double bv_threshold, min_bv_threshold, bv_falloff;
    int min_reads_cluster;
    int use_hc;
    double repr_percentile;
    int is_rna;
} rattle_cluster_params;

typedef struct {
    uint32_t n_clusters;
    int32_t *main_id;       /* [n_clusters]   cluster_t::main_seq.seq_id (index into the loaded reads) */
    uint8_t *main_rev;      /* [n_clusters]   cluster_t::main_seq.rev */
    uint32_t *offsets;      /* [n_clusters+1] member range of each cluster */
    int32_t *member_id;     /* [n_members]    cseq_t::seq_id, in the order cluster_t::seqs holds them */
    uint8_t *member_rev;    /* [n_members]    cseq_t::rev */
    /* work counters.  Exact and identical on every rank of a sharded job: [0] bit-vector pair tests, [1] full
       comparisons (pairs past the filter: their common k-mers are counted).  [2] k-mer matches summed over the count pass:
       exact when the pass counts per pair, an UPPER BOUND when the seed-major count kernel folds the hash (k > 10) or a
       seed's repeat list overflows -- it depends on which form the driver picked and is for reporting only.  The "index"
       form (RATTLE_PAIR_COUNT=index): k <= 10: exactly |common|; k > 10: the sum over the candidate's k-mers b of the
       multiplicity of fold(hash(b)), fold(h) = (h ^ h >> 20) & 0xFFFFF, among the seed's folded hashes -- an upper bound
       of |common| with no overflow rule (it keeps no repeat list).  Local to the
       calling rank: [3] seed rounds, [4] kernel launches, [5] pairs whose match count could still reach t_s and went
       through the patience search (the others are rejected exactly on the count). */
    uint64_t counters[8];
    int32_t *gene_id;       /* [n_clusters] cseq_t::gene_id of the --iso flow (index of the gene cluster), else NULL */
} rattle_cluster_set;

/* Keep a copy of the reads (and, if not NULL, their qualities) in HBM.  Later calls of
 * rattle_hip_cluster_unsorted / rattle_hip_correct_reads that are handed the SAME host buffers
 * (pointer, read count, total bases) use the resident copy instead of uploading the bases again;
 * the host buffers must stay unchanged until rattle_hip_unstage_reads.  This is how a caller that
 * runs `cluster` and `correct` on one read set (main.cpp reads the same fastq twice) pays the PCIe
 * transfer once. */
int rattle_hip_stage_reads(rattle_ctx *ctx, const uint8_t *seq_concat, const uint8_t *qual_concat, const uint64_t *offsets,
                           uint32_t n_reads);
int rattle_hip_unstage_reads(rattle_ctx *ctx);

int rattle_hip_cluster_reads(rattle_ctx *ctx, const rattle_cluster_params *params, rattle_cluster_set **out);
/* Same, restricted to a subset of the loaded reads given in processing order (the --iso
 * second level, main.cpp:281-318).  Ids in the result are positions in `subset`. */
int rattle_hip_cluster_subset(rattle_ctx *ctx, const rattle_cluster_params *params, const uint32_t *subset,
                              uint32_t n_subset, rattle_cluster_set **out);
/* Several subsets in one call (all gene clusters of the --iso level): subset i is
 * subset_ids[subset_offsets[i] .. subset_offsets[i+1]); outs[i] receives its clusters.  The subsets
 * are independent: their greedy rounds advance in lockstep and every round is one evaluation on the
 * device (n_workers is kept for ABI compatibility and ignored).  Results are identical to n_subsets
 * calls of rattle_hip_cluster_subset. */
int rattle_hip_cluster_subsets(rattle_ctx *ctx, const rattle_cluster_params *params, const uint32_t *subset_ids,
                               const uint64_t *subset_offsets, uint32_t n_subsets, rattle_cluster_set **outs, int n_workers);
/* The `rattle cluster` flow around cluster_reads for reads in FILE order (main.cpp:254-277):
 * stable length-descending sort (sort_read_set, fasta.cpp:458-464), index, gene-level
 * cluster_reads, then ids translated back to positions in the caller's order. */
int rattle_hip_cluster_unsorted(rattle_ctx *ctx, const uint8_t *seq_concat, const uint64_t *offsets, uint32_t n_reads,
                                int kmer_size, const rattle_cluster_params *params, rattle_cluster_set **out);
/* `rattle cluster --iso` (main.cpp:254-323) for reads in FILE order: gene level with (kmer_size, params), every
 * gene cluster sub-clustered with (iso_kmer_size, iso_params); result = the transcript clusters in gene order
 * with gene_id set, ids = positions in the caller's order.  n_gene_clusters (optional) receives the first level's count. */
int rattle_hip_cluster_iso_unsorted(rattle_ctx *ctx, const uint8_t *seq_concat, const uint64_t *offsets, uint32_t n_reads,
                                    int kmer_size, int iso_kmer_size, const rattle_cluster_params *params,
                                    const rattle_cluster_params *iso_params, rattle_cluster_set **out, uint32_t *n_gene_clusters);
void rattle_hip_cluster_set_free(rattle_cluster_set *cs);

/* The cluster report: why every read is where it is.  Every absorption the greedy clustering performs is one JOIN: in the initial
 * pass (pass 0) a read joins a founder, in merge pass 1, 2, ... a cluster, through its representative main.id, joins another
 * cluster's representative.  A clustering of n reads into c clusters has exactly n - c joins.  A join names the comparison that
 * decided it -- the first accepting founder, forward before reverse, exactly as the driver resolved it -- with what the full
 * comparison computed for that pair (cluster.cpp:20-34 / :44-58): bases, hc_bases and the variance, min_len = the shorter read's
 * length and score = the double the verdict compared with t_s (use_hc ? hc_bases / min_len : bases / min_len); score >= t_s and
 * variance < t_v hold for every join.  Joins are ordered by pass, then by the absorbed item's position in the pass; neither the
 * order nor the content depends on the seed batch.
 * Off by default; rattle_hip_set_cluster_report(ctx, 1) makes the following clustering calls on this context launch the report form of
 * the verdict kernel, which writes the three numbers of every accepted pair beside the pair.  No cluster set changes with the switch.
 * The joins travel inside the result object, behind the public struct; rattle_hip_cluster_report copies them out (release with
 * rattle_hip_cluster_report_free).  into / absorbed are ids in the id space of that set's member_id: loaded reads (cluster_reads),
 * positions in the subset (cluster_subset, cluster_subsets: every outs[i] carries its own joins), the caller's order
 * (cluster_unsorted).  cluster_iso_unsorted: the level-0 joins of the gene clustering (n - n_genes of them), then the level-1 joins of
 * every gene in gene order (n - n_clusters in all), ids in the caller's order.
 * RATTLE_ERR_STATE if the set was made with the switch off or is not an object of this library.  Sharded jobs carry no report yet: with
 * the switch on, on a context that is one rank of several (rattle_hip_set_exchange / rattle_hip_comm_init, nranks > 1), every
 * clustering entry point returns RATTLE_ERR_STATE before it exchanges anything (on every rank alike, so none is left waiting). */
typedef struct {
    uint64_t n;                 /* joins */
    uint8_t  *level;            /* 0: gene level / plain clustering, 1: --iso second level */
    uint32_t *pass; double *bv_threshold;
    int32_t  *into, *absorbed;
    uint8_t  *rev;
    int32_t  *bases, *hc_bases; uint32_t *min_len;
    double   *score, *variance;
} rattle_cluster_report;
int rattle_hip_set_cluster_report(rattle_ctx *ctx, int on);
int rattle_hip_cluster_report(const rattle_cluster_set *cs, rattle_cluster_report **out);
void rattle_hip_cluster_report_free(rattle_cluster_report *r);

/* ------------------------------------------------------------------------------------
 * assign: reads placed on a GIVEN set of targets (a transcriptome and a second sample, a replicate, the reads --min-reads left out)
 * by the comparison that decides cluster membership, cluster_together (/root/reference/cluster.cpp:13-61); the reference has no
 * counterpart.  For read r the ACCEPTED comparisons are the (target t, strand) for which cluster_together(T[t], R[r]) accepts on that
 * strand -- the target takes the seed's role whatever the two lengths are: the 6-mer bit-vector test at bv_threshold (with the forward
 * bypass of bv_threshold == 0), then score >= t_s && variance < t_v with score = (use_hc ? hc_bases : bases) / min(len) in the
 * reference's double arithmetic (a NaN variance rejects); strand 1 exists only when !is_rna.  There are no falloff or merge passes.
 *   best          the accepted comparison with the largest score (compared as doubles); ties: lowest target index, then forward
 *   n_accepted    the number of accepted (target, strand) comparisons
 *   second_score  the largest score among the accepted comparisons of OTHER targets than best's (two identical targets: == score;
 *                 the other strand of the same target does not count); -1.0 if there is none
 * target, rev, bases, hc_bases, min_len, score, variance describe the winning comparison (the fields of a line of cluster_report.tsv);
 * a read nothing accepts -- one shorter than kmer_size among them -- has target -1, score -1.0, second_score -1.0 and zeros elsewhere.
 * The result does not depend on target_batch, read_chunk, count_pass or the order in which the device scores the pairs: the accepted
 * comparisons are reduced per read ON THE DEVICE (csrc/assign.hip) and one 40-byte record per read is all that returns to the host.
 */
typedef struct {
    double t_s, t_v;
    double bv_threshold;
    int use_hc;
    int is_rna;
    uint32_t target_batch;  /* targets per evaluation against all reads; 0 = the default (512) */
    uint32_t read_chunk;    /* rattle_hip_assign_reads: reads indexed at a time; 0 = the default (2^20) */
    int count_pass;         /* 0 = automatic; 1 seed-major, 2 per-pair search, 3 seed-batch index, as in rattle_hip_debug_evaluate */
} rattle_assign_params;

typedef struct {
    uint32_t n;             /* reads; every array has n entries, in the order the reads were given */
    int32_t  *target;       /* index into the targets as given, or -1 */
    uint8_t  *rev;
    int32_t  *bases, *hc_bases;
    uint32_t *min_len;
    double   *score, *variance, *second_score;
    uint32_t *n_accepted;
} rattle_assignment;

/* The core: targets and reads are ids into the set rattle_hip_load_reads loaded (strands as for cluster_reads: both_strands = !is_rna).
 * The targets go in batches of target_batch seeds against all the reads.  n_targets == 0 or n_reads == 0: every read unassigned.
 * RATTLE_ERR_STATE, before anything is exchanged, on a context that is one rank of several: sharded jobs are not built. */
int rattle_hip_assign_loaded(rattle_ctx *ctx, const rattle_assign_params *params, const uint32_t *target_ids, uint32_t n_targets,
                             const uint32_t *read_ids, uint32_t n_reads, rattle_assignment **out);
/* Targets and reads from two buffers, in any order (no length sort is needed).  The reads go through in chunks of read_chunk, each
 * indexed together with the targets (replacing the loaded read set), so the device memory is bounded by the chunk, not by the sample;
 * the records come back in the caller's read order. */
int rattle_hip_assign_reads(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                            const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads, int kmer_size,
                            const rattle_assign_params *params, rattle_assignment **out);
void rattle_hip_assignment_free(rattle_assignment *a);

/* The candidate list (ABI 4): not only the best target of a read but its k best, k in 1..8, each with the fields of a line of
 * assignments.tsv, so that the runner-up of an isoform family can be named, aligned (align_pairs takes slot j's target and rev as they
 * are) and compared with the winner.  For read r:
 *   one candidate per target   of the accepted comparisons of r -- exactly those rattle_hip_assign_* reduces -- every target t that
 *                              accepts r on at least one strand gives ONE candidate, its comparison with the larger score; an equal
 *                              score goes to forward; the other strand of the same target is not a second candidate
 *   order                      score descending, compared as doubles; ties go to the lower target index
 *   length                     count[r] = min(k, number of accepting targets); the list is the first count[r] candidates
 *   slot r * k + j             target, rev, bases, hc_bases, min_len, score, variance of the j-th candidate; an unused slot
 *                              (j >= count[r]) has target -1, score -1.0 and zeros elsewhere
 * By construction slot 0 is the record of rattle_assignment and slot 1's score is its second_score.  Like that record the list does not
 * depend on target_batch, read_chunk, count_pass or the order in which the device scores the pairs: it is selected ON THE DEVICE
 * beside the record (csrc/assign.hip), 4 + 28 k bytes per read return to the host, and no pair is ever listed for it. */
typedef struct {
    uint32_t n, k;          /* reads, slots per read */
    uint32_t *count;        /* [n] filled slots of every read */
    int32_t  *target;       /* [n * k] from here on: slot r * k + j */
    uint8_t  *rev;
    int32_t  *bases, *hc_bases;
    uint32_t *min_len;
    double   *score, *variance;
} rattle_candidates;

/* rattle_hip_assign_loaded / rattle_hip_assign_reads with the candidate list: *out is field for field what the call without _top
 * returns for the same arguments, produced by the same code.  The errors are those of that call, in the same order; then
 * RATTLE_ERR_ARG for k == 0, k > 8 or cands == NULL -- all argument errors come before the refusal of a context that is one rank of
 * several (RATTLE_ERR_STATE) and before the device is looked at.  On an error both *out and *cands are NULL. */
int rattle_hip_assign_loaded_top(rattle_ctx *ctx, const rattle_assign_params *params, const uint32_t *target_ids, uint32_t n_targets,
                                 const uint32_t *read_ids, uint32_t n_reads, uint32_t k, rattle_assignment **out,
                                 rattle_candidates **cands);
int rattle_hip_assign_reads_top(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                                const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads, int kmer_size,
                                const rattle_assign_params *params, uint32_t k, rattle_assignment **out, rattle_candidates **cands);
void rattle_hip_candidates_free(rattle_candidates *c);

/* abundance (ABI 4): how much of every target is in the sample -- an expectation-maximisation over each read's compatible candidates, run
 * on the device (csrc/abundance.hip) in INTEGER FIXED POINT, so that the result is the same bits on every run and a scalar model
 * reproduces them (tests/abundance_ref.py).  The input is a candidate list as the _top calls return it; a hand-built one is as good.
 *   compatible     slot j < count[r] of read r is compatible iff score[r, j] >= ratio * score[r, 0] (one double multiply, one compare);
 *                  slot 0 always is.  The weights are uniform over the compatible slots.  A read with count[r] == 0 takes no part;
 *                  n_placed is the number of reads that do.  compatible_reads[t]: the reads with t in a compatible slot.
 *   units          A[t] is a uint64 in units of 2^-32 read, ONE = 2^32.  Start: a read with c compatible slots gives s = ONE / c to each
 *                  compatible slot j >= 1 and ONE - s (c - 1) to slot 0.
 *   one iteration  per read D = the sum of A[target] over its compatible slots; slot j >= 1 gets (uint64) floor((double)A_j / (double)D *
 *                  2^32) -- correctly rounded conversions, one IEEE division, no contraction --, slot 0 gets ONE minus those shares
 *                  (saturating at 0); A'[t] = the sum of the shares t receives, so sum(A') == n_placed * ONE after every iteration.
 *   stop           delta[i] = max_t |A'[t] - A[t]| after iteration i = 0, 1, ..; the result is the state after the first iteration with
 *                  delta[i] <= (uint64)(tol * 2^32), else the state after max_iters iterations with converged = 0.
 *   posterior      one more E-step at the final state: posterior[r * k + j] = (double)share / 2^32, 0.0 in every other slot.
 *   per target     units = A[t], est_reads = (double)A[t] / 2^32, cpm = (double)A[t] / (double)(n_placed * ONE) * 1e6 (0 if n_placed == 0).
 * iter_block: iterations enqueued between two looks of the host at delta (0: 32); the result does not depend on it.  RATTLE_EM_PLAIN=1 in
 * the environment: one atomic per entry instead of the sorted, merged scatter -- the same bits, for measurement.
 * params == NULL: ratio 0.95, tol 0.001 read, max_iters 1000, iter_block 32.
 * Errors, RATTLE_ERR_ARG before the device is looked at, in this order: a NULL pointer; k outside 1..8; a count[r] > k; a filled slot with
 * a target outside [0, n_targets); ratio not in (0, 1]; tol negative, NaN or >= 2^20; max_iters == 0.  Then RATTLE_ERR_STATE on a context
 * that is one rank of several.  n_reads == 0 or n_targets == 0: zeros, iterations 0, converged 1.  The context's loaded reads and index
 * are left as they are.  rattle_hip_kernel_stats: id 10, the ordering and the start as one launch group, each iter_block as one (their
 * launches are counted one by one), the posterior as one. */
typedef struct { double ratio, tol; uint32_t max_iters, iter_block; } rattle_abundance_params;
typedef struct {
    uint32_t n_targets, n_reads, k, iterations; int converged; uint64_t n_placed;
    uint64_t *units; double *est_reads, *cpm; uint32_t *compatible_reads;   /* [n_targets] */
    uint64_t *delta;                                                        /* [iterations] */
    double *posterior;                                                      /* [n_reads * k] */
} rattle_abundance;
int  rattle_hip_abundance(rattle_ctx *ctx, const rattle_candidates *cands, uint32_t n_targets, const rattle_abundance_params *params,
                          rattle_abundance **out);
void rattle_hip_abundance_free(rattle_abundance *a);

/* ------------------------------------------------------------------------------------
 * align_pairs: WHERE on its transcript every placed read lies (kernel E, csrc/pair_align.hip); the reference has no counterpart.
 * target_of_read and rev are exactly rattle_assignment::target and ::rev: read r is aligned to target target_of_read[r] (-1: not
 * submitted), reverse-complemented first when rev[r] == 1 (A<->T, C<->G, U complements to A).  Only A, C, G, T, U occur; two letters
 * match iff they are equal after U is read as T.  The alignment is a Smith-Waterman local alignment with match +5, mismatch -4 and
 * gap -8 PER GAPPED COLUMN: the match, mismatch and gap-open values of `correct`'s engine (a15), but with LINEAR gaps, deliberately not
 * affine (affine gaps and other scorings: rattle_hip_align_pairs_scored, below) -- that is what makes the record below derivable
 * without a traceback (the device writes no traceback matrix):
 *   H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), H[i-1][j] - 8, H[i][j-1] - 8),  H[0][*] = H[*][0] = 0,  i over the read, j over the target
 * and it is fully determined: a cell with H == 0 begins a new alignment (a path never runs through a zero); predecessors that tie are
 * taken diagonal, then up (a read base against a gap), then left (a target base against a gap); the end cell is the largest H, ties to
 * the smallest i, then the smallest j; no positive cell: no alignment.  Per read:
 *   status      0 aligned; 1 no positive cell, or one of the two sequences empty; 2 skipped: len(q) * len(t) > max_cells; 3 not submitted
 *   score       H of the end cell
 *   q_start, q_end, t_start, t_end   0-based, end-exclusive; q_* on the read AS GIVEN (PAF): for rev == 1 they are Lq - e and Lq - s of
 *               the reverse-complemented coordinates
 *   matches, mismatches, q_gap (read bases against a gap), t_gap (target bases against a gap)
 * (zeros where status != 0).  Every cell carries (start_i, start_j, matches) of its path, taken from the predecessor the rule picks;
 * with the spans sq, st:  mismatches = (8 (sq + st) - 21 matches + score) / 12,  q_gap = sq - matches - mismatches,  t_gap = st - matches
 * - mismatches.  One 40-byte record per submitted read is all that returns to the host.
 * RATTLE_ERR_ARG, before the device is looked at: a NULL pointer, a target index >= n_targets, a rev other than 0 or 1, a byte outside
 * ACGTU in a submitted read or in a target a submitted read names, a sequence of 2^31 bases or more.  RATTLE_ERR_STATE: a context
 * without a device, and, before anything is exchanged, a context that is one rank of several (sharded jobs are not built).
 */
typedef struct { uint64_t max_cells;   /* 0 = no limit */
                 uint32_t pair_chunk;  /* pairs in flight; 0 = default; the result does not depend on it */ } rattle_align_params;
typedef struct { uint32_t n; uint8_t *status; int32_t *score;
                 uint32_t *q_start, *q_end, *t_start, *t_end, *matches, *mismatches, *q_gap, *t_gap; } rattle_alignment;
int  rattle_hip_align_pairs(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                            const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                            const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                            const rattle_align_params *params, rattle_alignment **out);
void rattle_hip_alignment_free(rattle_alignment *a);

/* ------------------------------------------------------------------------------------
 * align_cigars: align_pairs, and WHICH columns of every alignment disagree (kernel F, csrc/pair_cigar.hip, after kernel E on the same
 * uploaded sequences).  *out is field for field what rattle_hip_align_pairs returns for the same arguments.  The CIGAR of read r is
 * ops[offset[r] .. offset[r + 1]), each op  length << 4 | code  with BAM's codes, in the extended set:
 *   7 '='  a read base on an equal target base (after U is read as T)     8 'X'  a read base on an unequal target base
 *   1 'I'  a read base against a gap (counted in q_gap)                   2 'D'  a target base against a gap (counted in t_gap)
 * It is the path the rule of align_pairs picks (diagonal, then up, then left; it begins behind a zero cell), read from its start to its
 * end on the strand that was aligned: the read reverse-complemented first when rev[r] == 1, the target always forward -- PAF's order on
 * both strands.  Runs are merged; there is no clipping op (q_start and q_end say what is clipped).  So the summed lengths of '=', 'X',
 * 'I', 'D' are matches, mismatches, q_gap, t_gap of the record, '=' + 'X' + 'I' = q_end - q_start and '=' + 'X' + 'D' = t_end - t_start.
 * A read whose status is not 0 has no ops: offset[r + 1] == offset[r].  (A run of 2^28 columns or more would come in pieces.)
 * Kernel F works on the rectangle (q_start, q_end] x (t_start, t_end] of kernel E's record alone: it records 2 bits per cell there
 * (16 bytes per 64 cells), walks them back on the device, and only the ops and one count per pair return to the host.  The code bytes
 * of the pairs in flight are capped at 4 GiB (pair_chunk bounds their number as it does for kernel E); a pair that alone needs more
 * runs alone, and if its allocation fails the call ends with RATTLE_ERR_HIP and nothing is returned.  The result depends on neither.
 * Errors: those of rattle_hip_align_pairs, checked in the same order before the context is looked at; cigars == NULL is RATTLE_ERR_ARG.
 * rattle_hip_kernel_stats: kernel F is id 7, one launch per sub-chunk (the gather of the ops is not counted); kernel E's launches of the
 * call count under id 6 as before.  alg_bytes of id 7, per aligned pair with R = q_end - q_start rows and C = t_end - t_start columns:
 *   R + C  (the rectangle's sequence bytes)  +  16 * (ceil(R / 64) * (C - 1) + R)  (code records written)  +  4 * ops  +  4  (the count)
 */
typedef struct { uint32_t n; uint64_t *offset /* n + 1 */; uint32_t *ops /* len << 4 | op */; } rattle_cigars;
int  rattle_hip_align_cigars(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                             const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                             const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                             const rattle_align_params *params, rattle_alignment **out, rattle_cigars **cigars);
void rattle_hip_cigars_free(rattle_cigars *c);

/* ------------------------------------------------------------------------------------
 * align_pairs_scored, align_cigars_scored: the two calls above with AFFINE gaps and a scoring the caller chooses (the three-state forms
 * of kernels E and F: the <true> instantiations in csrc/pair_align.hip and csrc/pair_cigar.hip).  The scoring is four positive magnitudes, spoa's
 * convention: match +match, mismatch -mismatch, the first gapped column of a gap -gap_open, every further one -gap_extend;
 *   1 <= match <= 64, 1 <= mismatch <= 64, 1 <= gap_extend <= gap_open <= 64
 * so {5, 4, 8, 6} is `correct`'s engine, {5, 4, 8, 8} the linear rule of align_pairs and {2, 4, 4, 2} minimap2's.  Gotoh's recurrence:
 *   U[i][j] = max(H[i-1][j] - open, U[i-1][j] - extend)     a read base against a gap      U[0][*] = -inf
 *   L[i][j] = max(H[i][j-1] - open, L[i][j-1] - extend)     a target base against a gap    L[*][0] = -inf
 *   H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])                          H[0][*] = H[*][0] = 0
 * fully determined as align_pairs is: a cell with H == 0 begins a new alignment; in H ties go diagonal, then U, then L; in U and in L
 * OPEN WINS A TIE WITH EXTEND; the end cell is the largest H, ties to the smallest i, then the smallest j.  Since H >= U and H >= L, no
 * path runs through a cell whose H is 0, and with gap_open == gap_extend the path is cell for cell the linear one.  The structs returned,
 * their fields and their free functions are those of align_pairs and align_cigars; every state of every cell carries (start_i, start_j,
 * matches, mismatches) of its path, and q_gap, t_gap follow from the spans.  A CIGAR's 'I' and 'D' runs are the gaps of the path.
 * These two ALWAYS run the three-state kernels, for {5, 4, 8, 8} too (ids 8 and 9 of rattle_hip_kernel_stats; ids 6 and 7 do not move):
 * alg_bytes of id 8 is that of id 6, of id 9 that of id 7 with 32 in place of 16 (4 bits per cell: H's 2-bit code, "U extends",
 * "L extends").  The strip of id 8 takes 40 bytes per column of a read longer than 64 bases, that of id 9 8 bytes.
 * Errors: those of rattle_hip_align_pairs (rattle_hip_align_cigars), checked in the same order; then, still before the device is looked
 * at, RATTLE_ERR_ARG for scoring == NULL, a magnitude outside the limits above or gap_extend > gap_open, and a submitted pair with
 * match * min(Lq, Lt) > 2^31 - 1 (its score might not fit the record).
 */
typedef struct { uint32_t match, mismatch, gap_open, gap_extend; } rattle_align_scoring;
int  rattle_hip_align_pairs_scored(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                                   const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                                   const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                                   const rattle_align_params *params, const rattle_align_scoring *scoring, rattle_alignment **out);
int  rattle_hip_align_cigars_scored(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                                    const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                                    const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                                    const rattle_align_params *params, const rattle_align_scoring *scoring, rattle_alignment **out,
                                    rattle_cigars **cigars);

/* ------------------------------------------------------------------------------------
 * align_pairs_mode, align_cigars_mode (ABI 4): the four calls above with an alignment MODE.  scoring == NULL is the linear form (5, 4, 8, 8
 * on the two-state kernels), any other the affine form.  RATTLE_ALIGN_LOCAL returns the bytes of the call it stands for (align_pairs /
 * align_pairs_scored, align_cigars / align_cigars_scored).  RATTLE_ALIGN_READ aligns every read END TO END and leaves the target's ends
 * free (semi-global): nothing of the read is clipped, so an overhang or a foreign exon shows as an I run or as X columns at the end of
 * the line, and the scores of a read on two targets are scores of the same thing.  The <*, true> instantiations of kernels E and F.
 * With i over the read (reverse-complemented first where rev == 1), j over the target and (m, x, o, e) the scoring:
 *   H[0][j] = 0 for j = 0..Lt          U[0][*] = -inf        (the alignment may begin at any target position)
 *   H[i][0] = U[i][0] = -(o + (i-1) e) L[*][0] = -inf        (read bases before the target's first base: a gap)
 *   U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)
 *   L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)
 *   H[i][j] = max(H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])           -- no zero floor: a cell with H == 0 is an ordinary cell
 * Ties as in the local mode: in H diagonal, then U, then L; in U and in L open wins a tie with extend.  The end cell is the largest
 * H[Lq][j] over j = 1..Lt, ties to the smallest j.  The path goes back to row 0 and ends in (0, t_start); row 0 has no left moves, and a
 * path that reaches column 0 goes straight up, the rows left being one I run.  So an alignment may begin and end with an I run, never
 * with a D run.  Per read:
 *   status      0 for every submitted pair of two non-empty sequences; 1 (a sequence is empty), 2 and 3 as in align_pairs
 *   score       H of the end cell: may be zero or negative
 *   q_start = 0 and q_end = Lq, on either strand;  t_start, t_end from the path, t_end - t_start may be 0 (the whole read one I run)
 *   matches, mismatches, q_gap, t_gap as in align_pairs; in the linear form mismatches = (8 (Lq + st) - 21 matches + score) / 12 holds
 * CIGAR: the same op set, no clipping op; '=' + 'X' + 'I' = Lq and '=' + 'X' + 'D' = t_end - t_start.  Kernel F works on the rectangle
 * (0, Lq] x (t_start, t_end] with this mode's borders (top row H' = 0, U' = L' = -inf; left column H' = U' = -(o + (i-1) e), L' = -inf),
 * which reproduces the path (DESIGN.md has the lemma, tests/test_align_ends_ref.py checks it).  A pair with t_end == t_start does not go
 * to kernel F: the host writes its one op, Lq << 4 | I, and it does not count in alg_bytes.
 * rattle_hip_kernel_stats: the launches count under the ids of their gap form (6 and 7, 8 and 9), alg_bytes by the same formulas.
 * Errors: those of the call the scoring selects, in their order; then, still before the device is looked at, RATTLE_ERR_ARG for a mode
 * that is neither of the two, and in read mode for a submitted pair with gap_open + gap_extend * (Lq - 1) >= 2^29 (the kernels' minus
 * infinity, -2^30, has to stay below every score).
 */
#define RATTLE_ALIGN_LOCAL 0
#define RATTLE_ALIGN_READ  1
int  rattle_hip_align_pairs_mode(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                                 const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                                 const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                                 const rattle_align_params *params, const rattle_align_scoring *scoring /* NULL: the linear form */, int mode,
                                 rattle_alignment **out);
int  rattle_hip_align_cigars_mode(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                                  const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                                  const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                                  const rattle_align_params *params, const rattle_align_scoring *scoring /* NULL: the linear form */, int mode,
                                  rattle_alignment **out, rattle_cigars **cigars);

/* ------------------------------------------------------------------------------------
 * align_pileup (ABI 4): align_cigars_mode, and what the aligned reads say about EVERY BASE of every target (kernel G,
 * csrc/pair_pileup.hip, behind kernel F's gather on the ops that lie on the device; tests/pileup_ref.py is the contract in plain Python).
 * *out, and *cigars when asked for, are what rattle_hip_align_cigars_mode returns for the same arguments.  With cigars == NULL the
 * compact ops are NOT copied to the host (the per-pair counts still are: the offsets on the device need them).
 * One table over the concatenated targets: n = target_offsets[n_targets] positions, position p is byte p of target_concat, eight uint32
 * counts per position, as eight arrays (the table is planar on the device too: a wavefront on 64 consecutive columns of a run adds into
 * at most four contiguous segments).  All counts are on the TARGET's strand.  Walk the CIGAR of every read with status 0 as align_cigars
 * defines it -- the read reverse-complemented first when rev == 1, the target forward, U read as T -- from t_start, j the target position
 * and i the row of the aligned read:
 *   a, c, g, t at j      a column of an '=' or 'X' op whose READ base (on the aligned strand) is that letter
 *   del at j             a column of a 'D' op
 *   ins at j             an 'I' op that is NEITHER THE FIRST NOR THE LAST op of the read's CIGAR, once per op, at the target position of
 *                        the column that follows it (the base to its right)
 *   starts at t_start, ends at t_end - 1     a read whose rectangle has at least one column (t_end > t_start)
 * depth = a + c + g + t + del.  A leading or trailing I run is not counted: it occurs in RATTLE_ALIGN_READ only and is the read's
 * overhang, what the local mode would have clipped.  A read-mode pair with t_end == t_start (the host-written single I op) and a read
 * with status 1, 2 or 3 add nothing.  So the four letter arrays sum to matches + mismatches over the aligned reads, del to their t_gap,
 * starts and ends each to the number of status-0 reads with a column, and ins > 0 at a position implies depth > 0 there.  The counts
 * are integers, so they do not depend on the order the device adds them in: two runs give the same bytes, and neither pair_chunk nor
 * the cap on the code bytes changes them.  A count cannot overflow (n_reads is a uint32).  (A run of 2^28 columns or more comes in
 * pieces and an I run would count once per piece; no input within the other limits reaches that.)
 * The table is zeroed once on the device, added to by one launch per sub-chunk of kernel F that has an op, and copied to the host once,
 * 32 n bytes.  The eight arrays are ONE allocation, freed by rattle_hip_pileup_free alone.
 * Errors: those of rattle_hip_align_cigars_mode, in their order, with pileup == NULL (in place of cigars == NULL) RATTLE_ERR_ARG.  A
 * failed allocation of the table, on the host or the device, is RATTLE_ERR_HIP and nothing is returned.
 * rattle_hip_kernel_stats: kernel G is id 11, one launch per sub-chunk of kernel F that has an op; kernels E and F count under their ids
 * as in align_cigars_mode, and the other calls never launch id 11.  alg_bytes of id 11, per aligned pair with a column, R rows:
 *   4 * ops + R  (the ops and the read bases read)  +  4 * (matches + mismatches + t_gap + internal I ops + 2)  (the adds made)
 * Every launch adds its pairs' share but the 4 bytes per internal I op: the host never sees the ops, so that share is counted from the
 * ins array and added ONCE, when the call ends and the table is back.  Stats read while the call runs do not hold it yet.
 */
typedef struct { uint64_t n;  /* target_offsets[n_targets] */
                 uint32_t *a, *c, *g, *t, *del, *ins, *starts, *ends; } rattle_pileup;
int  rattle_hip_align_pileup(rattle_ctx *ctx, const uint8_t *target_concat, const uint64_t *target_offsets, uint32_t n_targets,
                             const uint8_t *read_concat, const uint64_t *read_offsets, uint32_t n_reads,
                             const int32_t *target_of_read /* -1: not submitted */, const uint8_t *rev,
                             const rattle_align_params *params, const rattle_align_scoring *scoring /* NULL: the linear form */, int mode,
                             rattle_alignment **out, rattle_cigars **cigars /* may be NULL */, rattle_pileup **pileup);
void rattle_hip_pileup_free(rattle_pileup *p);

/* ------------------------------------------------------------------------------------
 * a15  spoa engine + graph as called from /root/reference/correct.cpp:395-405,428-436,520-532
 * (createAlignmentEngine(kSW,5,-4,-8,-6); align + add_alignment per sequence;
 * generate_multiple_sequence_alignment).  Packs are independent; pack p holds sequences
 * [pack_first[p], pack_first[p+1]) of the concatenated input, aligned in that order.
 * Result: for each pack its MSA width and rows (one row per sequence, '-' for gaps).
 * Letters: every byte except 0 (the padding of the device's rows) and '-' (the gap of the rows returned) is a letter; a sequence that
 * holds one of the two is refused with RATTLE_ERR_ARG, before the device is looked at.  Two letters match iff their bytes are equal
 * (T and U, upper and lower case differ), as in the reference.  One limit the reference does not have: an MSA column holds at most
 * five distinct letters (A, C, G, T and U fit); a pack that would need a sixth ends the call with RATTLE_ERR_ARG and a message that
 * names the pack and the limit.
 */
typedef struct {
    uint32_t n_packs;
    uint32_t *width;        /* [n_packs]  MSA columns */
    uint64_t *row_offset;   /* [n_seqs+1] byte offset of each sequence's row in `rows` */
    char *rows;             /* rows of all packs back to back */
    uint64_t counters[8];   /* DP cells, alignments, graph nodes (sum of final sizes), rows, DP cells computed, certified bands, failed band certificates */
} rattle_msa_set;

int rattle_hip_poa_msa(rattle_ctx *ctx, const uint8_t *seq_concat, const uint64_t *offsets, uint32_t n_seqs,
                       const uint32_t *pack_first, uint32_t n_packs, rattle_msa_set **out);
void rattle_hip_msa_set_free(rattle_msa_set *ms);


/* ------------------------------------------------------------------------------------
 * a14-a20  correct_reads   /root/reference/correct.cpp:311-563 (signature correct.hpp:44)
 * Pack building (strided split, in-place reverse complement of `rev` members), POA #1 over
 * the raw reads of every pack, fix_msa_ends, column vote + per-read correction, POA #2 over
 * the corrected reads, pack consensus, POA #3 over the pack consensi of multi-pack clusters.
 * All POAs of one stage run in a single device pass (kernel C); the post-MSA logic
 * (correct.cpp:32-309) is kernel D on the device, in the reference's double arithmetic and
 * accumulation order.
 * Reads are given in FILE order with qualities (main.cpp:386); clusters index them by seq_id.
 * Outputs follow the reference's single-thread order: packs in queue order, pack consensi
 * collected in pack order (the reference's multi-thread run uses completion order).
 * Headers are not handled here: the caller derives them from read_id / cluster_id / gene_id.
 */
struct rattle_read_set_s;      /* rattle_read_set, defined below */
typedef struct {
    double min_occ, gap_occ, err_ratio;   /* 0.3, 0.3, 30.0 */
    int split, min_reads;                 /* 200, 5 */
    int n_threads;                        /* host threads for pack planning / output assembly; 0 = all cores */
    char vote_order[8];                   /* column-vote tie order, 6 symbols; "" = "U-GTCA", the
                                             iteration order of the reference's unordered_map
                                             (correct.cpp:105-110,174) under libstdc++ */
    /* Order in which a multi-pack cluster's pack consensi enter POA #3 (correct.cpp:469,520-526).  The
     * reference collects them in worker COMPLETION order when n_threads > 1; the default here is pack
     * order (the reference's single-thread order).  Optional override for n_pack_orders clusters:
     * cluster pack_order_cluster[i] takes its packs in the order
     * pack_order_perm[pack_order_offsets[i] .. pack_order_offsets[i+1]) -- a permutation of 0..np-1 over
     * the cluster's packs that passed the min_reads test, in queue order. */
    uint32_t n_pack_orders;
    const uint32_t *pack_order_cluster;
    const uint32_t *pack_order_offsets;
    const uint32_t *pack_order_perm;
    /* A pack whose POA does not fit the device (the DP record of one alignment outgrows the HBM left for
     * the arena; 100 kb reads need > 10^10 cells per alignment in the reference as well) is SKIPPED, not
     * fatal: its reads go to `uncorrected` untouched, it contributes no consensus, and it is listed in
     * rattle_correction::skipped.  max_pack_cells > 0 additionally skips, before any device work, every
     * pack whose largest alignment would need more than that many DP cells by the bound
     * (6 * longest read + 64) * longest read; 0 = no such limit. */
    uint64_t max_pack_cells;
    /* Optional (ABI 3; NULL = off): called ONCE, from a thread of the library, as soon as this call's corrected reads are
     * complete in host memory -- the consensus stages (POA #2 / #3) still run on the device, so a caller can format and
     * write corrected.fq meanwhile (the reference writes its three files after correct_reads returns, main.cpp:405-408).
     * `corrected` is the set the call will return in rattle_correction::corrected (same pointers, read-only here),
     * `corrected_pack` its per-record pack index.  Not called when the call fails before that point or has no pack. */
    void (*corrected_ready)(void *user, const struct rattle_read_set_s *corrected, const uint32_t *corrected_pack);
    void *corrected_ready_user;
} rattle_correct_params;

typedef struct rattle_read_set_s {
    uint32_t n;
    int32_t *read_id;       /* original read index, or -1 for a consensus */
    int32_t *cluster_id;    /* index of the cluster in the input cluster set */
    int32_t *n_reads;       /* consensi: reads summed over the cluster's packs; else 0 */
    uint64_t *off;          /* [n+1] */
    char *seq;
    char *qual;
} rattle_read_set;

/* Packs (stage 1, 2: POA #1 / #2 of a pack) or clusters (stage 3: POA #3) that were not processed. */
typedef struct {
    uint32_t n;
    int32_t *cluster_id;    /* [n] */
    uint32_t *pack;         /* [n] index of the pack among the cluster's queued packs (stage 3: 0) */
    uint32_t *stage;        /* [n] 1: POA #1 did not fit (reads -> uncorrected), 2: POA #2 (no pack consensus),
                                   3: POA #3 (no cluster consensus), 0: max_pack_cells rule */
    uint64_t *read_off;     /* [n+1] range of the entry's reads in read_id */
    int32_t *read_id;       /* original read indices */
} rattle_skip_list;

typedef struct {
    rattle_read_set corrected, uncorrected, consensi;
    uint64_t counters[8];   /* [0] DP cells (the reference's count: graph rows x sequence columns of every alignment), [1] alignments, [2] packs queued,
                             * [3] packs skipped, [4] reads in skipped packs, [5] DP cells the device computed (fewer where the exact band for
                             * near-identical sequences was certified), [6] alignments with a certified band, [7] failed band certificates */
    rattle_skip_list skipped;
    /* global pack index of every corrected / uncorrected record (0xFFFFFFFF: member of a pack that never
     * entered the queue); what rattle_hip_correction_gather orders the merged result by */
    uint32_t *corrected_pack, *uncorrected_pack;
} rattle_correction;

/* (A context that clustered its reads holds their k-mer index, 12-20 bytes per base.  `correct` does not use it and sizes its arena by
 * the free memory: when the index exceeds 24 GB it is released here, and the next rattle_hip_cluster_reads without a new
 * rattle_hip_load_reads returns RATTLE_ERR_STATE "no reads loaded".  rattle_hip_cluster_unsorted loads by itself and is unaffected.) */
int rattle_hip_correct_reads(rattle_ctx *ctx, const uint8_t *seq_concat, const uint8_t *qual_concat,
                             const uint64_t *offsets, uint32_t n_reads, uint32_t n_clusters,
                             const uint32_t *cluster_offsets, const int32_t *member_id, const uint8_t *member_rev,
                             const rattle_correct_params *params, rattle_correction **out);
void rattle_hip_correction_free(rattle_correction *c);
/* The per-read correction report: what the per-read correction (correct.cpp:196-309) did to every corrected read.  Off by default;
 * rattle_hip_set_correction_report(ctx, 1) makes the following rattle_hip_correct_reads calls on this context launch the report form
 * of the post-MSA kernel in stage 1, which counts, for every row of a pack over the columns of its voting window after
 * fix_msa_ends, the branch that handled each column (nt: the row's symbol, c: the column winner):
 *   match          nt is a base and nt == c
 *   substituted    nt and c are different bases, the winner's share reaches min_occ and the error test passes: c is emitted
 *   mismatch_kept  nt and c are different bases and nt is emitted
 *   inserted       nt == '-', c is a base and its share reaches gap_occ: c is emitted
 *   deleted        nt is a base, c == '-' and its share reaches gap_occ: nothing is emitted
 *   gap_kept       nt is a base, c == '-' below gap_occ: nt is emitted
 * (a gap that stays a gap is not counted).  With trim_front / trim_back, the bases fix_msa_ends erased at either end:
 *   out_len = match + substituted + mismatch_kept + inserted + gap_kept
 *   in_len  = trim_front + trim_back + match + substituted + mismatch_kept + deleted + gap_kept
 * No output of correct_reads changes with the switch.  The counters travel inside the result object, behind the public struct;
 * rattle_hip_correction_report copies them out (n == corrected.n, every array parallel to corrected.read_id; release with
 * rattle_hip_correction_report_free).  RATTLE_ERR_STATE if the correction was made with the switch off -- or, for a result of
 * rattle_hip_correction_gather, if ANY rank made its share with the switch off -- or is not an object of this library. */
typedef struct {
    uint32_t n;
    uint32_t *in_len, *out_len, *trim_front, *trim_back;
    uint32_t *match, *substituted, *mismatch_kept, *inserted, *deleted, *gap_kept;
} rattle_correction_report;
int rattle_hip_set_correction_report(rattle_ctx *ctx, int on);
int rattle_hip_correction_report(const rattle_correction *c, rattle_correction_report **out);
void rattle_hip_correction_report_free(rattle_correction_report *r);

/* The consensus support: how many reads stand behind every base of every consensus.  Off by default;
 * rattle_hip_set_consensus_support(ctx, 1) makes the consensus stages of the following rattle_hip_correct_reads calls on this context
 * launch the report form of the post-MSA kernel's mode 2.  For every record of `consensi` and every base j of it, two values counted
 * in READS, support[j] <= depth[j] and depth[j] >= 1:
 *   level 2, the consensus of one pack (POA #2 over its corrected reads + the column vote).  Base j is the winner of a column k;
 *     depth = the rows whose voting window after fix_msa_ends covers k, gaps included (the vote's total), support = the winner's
 *     count.  The rows are corrected reads.  A cluster with a single queued pack takes that pack's consensus as its own
 *     (correct.cpp:547-549) and its support with it; a pack consensus that is a copy of a single sequence (min_reads = 0, what
 *     `polish` uses) has 1 / 1 for every base.
 *   level 3, the consensus of a cluster of several packs (POA #3 over its pack consensi + the column vote).  Row i is pack consensus
 *     i with its level-2 values sup_i[], dep_i[] per base.  Base j is the winner w of a column K; of the rows whose window
 *     [rfirst_i, rlast_i] covers K, support[j] is the sum of sup_i[b] over the rows that hold w at K (b: that base's index in row
 *     i), and depth[j] the sum of dep_i[b'] over all of them, b' being the row's base at K or, where the row has '-' at K, the row's
 *     last base at a column below K (it exists: a window starts on a base).
 * pack_support / pack_depth are the vote's own winner count / total of the column, in rows of the last MSA: equal to support / depth
 * at level 2, counts of pack consensi at level 3.  A cluster whose POA #3 was skipped has no consensus and so no record.
 * No output of correct_reads changes with the switch.  The values travel inside the result object, behind the public struct;
 * rattle_hip_consensus_support copies them out (release with rattle_hip_consensus_support_free).  RATTLE_ERR_STATE if the correction
 * was made with the switch off or is not an object of this library.  Sharded jobs carry no support yet: with the switch on, a context
 * that is one rank of several gets RATTLE_ERR_STATE from rattle_hip_correct_reads before anything is exchanged, on every rank alike,
 * and the result of rattle_hip_correction_gather has none. */
typedef struct {
    uint32_t n;                 /* == consensi.n, parallel to consensi.read_id */
    uint8_t  *level;            /* 2: the votes of POA #2 (one pack), 3: composed through POA #3 */
    uint64_t *off;              /* [n+1], == consensi.off */
    uint32_t *support, *depth;  /* per base, reads */
    uint32_t *pack_support, *pack_depth;   /* per base, rows of the last MSA */
} rattle_consensus_support;
int  rattle_hip_set_consensus_support(rattle_ctx *ctx, int on);
int  rattle_hip_consensus_support(const rattle_correction *c, rattle_consensus_support **out);
void rattle_hip_consensus_support_free(rattle_consensus_support *s);

/* Optional: allocate the POA arena of correct_reads ahead of time (a caller can overlap the seconds a > 100 GB allocation takes
 * with reading its input).  bytes is a hint, clamped to what the device has free; correct_reads grows the arena if it must. */
int rattle_hip_reserve_arena(rattle_ctx *ctx, uint64_t bytes);

/* ------------------------------------------------------------------------------------
 * One job over the GPUs of a node.  The reference parallelises the same axes with host
 * threads: the strided candidate loop of a seed (cluster.cpp:138-158,189-209), the gene clusters of the
 * --iso level (main.cpp:281-318) and the pack queue of `correct` (correct.cpp:377-392).  Here a context
 * can be one RANK of nranks (one process or thread per GPU, every rank holding the same reads and making
 * the same calls):
 *   cluster_reads / cluster_unsorted : each rank scores its share of the candidates of a seed batch
 *                                      (cyclic by candidate position), hit lists are all-gathered, every
 *                                      rank resolves them identically -> identical results on all ranks;
 *   cluster_subsets                  : gene clusters LPT-assigned to ranks by size, results all-gathered;
 *   correct_reads                    : packs LPT-assigned by the cost proxy L_0 * sum L_j; both POAs of a
 *                                      pack on one GPU; pack consensi all-gathered; POA #3 groups
 *                                      LPT-assigned; every rank returns ITS packs' corrected / uncorrected
 *                                      reads and ALL consensi; rattle_hip_correction_gather reassembles
 *                                      the single-GPU result (same order, same bytes) on the root.
 * Transports: RCCL over xGMI (rattle_hip_comm_init; device buffers, the library's own stream) or a
 * caller-supplied all-gather on host buffers (rattle_hip_set_exchange; MPI / gloo / tests).
 */
/* all ranks call with their `send` (send_bytes == recv_bytes[rank]); recv receives the nranks pieces
 * back to back in rank order.  Returns 0 on success. */
typedef int (*rattle_allgatherv_fn)(void *user, const void *send, uint64_t send_bytes, void *recv, const uint64_t *recv_bytes);
int rattle_hip_set_exchange(rattle_ctx *ctx, int rank, int nranks, rattle_allgatherv_fn fn, void *user);
#define RATTLE_COMM_ID_BYTES 128
int rattle_hip_comm_unique_id(uint8_t *id_out /* RATTLE_COMM_ID_BYTES, from rank 0, to be handed to every rank */);
int rattle_hip_comm_init(rattle_ctx *ctx, int rank, int nranks, const uint8_t *id);
int rattle_hip_comm_destroy(rattle_ctx *ctx);
/* statistics of the exchange since context creation: collective calls, payload bytes received */
int rattle_hip_comm_stats(rattle_ctx *ctx, uint64_t *calls, uint64_t *bytes);
/* Collective self-test of the attached transport (every rank calls it): one ragged all-gather-v and one gather
 * to the last rank, contents verified.  0, or RATTLE_ERR_HIP with the damaged piece named.  A launcher runs it
 * once after rattle_hip_comm_init / rattle_hip_set_exchange, before it trusts the transport with a job. */
int rattle_hip_comm_probe(rattle_ctx *ctx);
/* Collective: merges the per-rank results of rattle_hip_correct_reads on `root` (*merged is NULL on the
 * other ranks).  With nranks == 1 it returns a copy.  The correction report travels with the records: the merged
 * result has one (equal to the single-GPU one) if every rank's share has. */
int rattle_hip_correction_gather(rattle_ctx *ctx, const rattle_correction *local, int root, rattle_correction **merged);

/* The work list of correct_reads without a device (pack building correct.cpp:328-370 and the static
 * assignment to ranks), for callers that schedule themselves and for the CPU tests of the sharding. */
typedef struct {
    uint32_t n_packs;
    uint32_t *pack_first;   /* [n_packs+1] member range */
    int32_t *member_id;     /* read ids, pack after pack */
    uint8_t *member_rev;
    int32_t *pack_cluster;  /* [n_packs] */
    uint32_t *pack_local;   /* [n_packs] index among the cluster's queued packs */
    uint64_t *pack_cost;    /* [n_packs] L_0 * sum L_j */
    uint32_t *pack_owner;   /* [n_packs] rank */
    uint32_t n_unqueued;    /* members of packs that never enter the queue (<= min_reads, or max_pack_cells) */
    int32_t *unqueued_id;
    int32_t *unqueued_cluster;
} rattle_pack_plan;
int rattle_hip_plan_packs(const uint64_t *offsets, uint32_t n_reads, uint32_t n_clusters, const uint32_t *cluster_offsets,
                          const int32_t *member_id, const uint8_t *member_rev, const rattle_correct_params *params, int nranks,
                          rattle_pack_plan **out);
void rattle_hip_pack_plan_free(rattle_pack_plan *p);
/* longest-processing-time-first: items by cost descending (ties: lower index) to the least loaded rank (ties: lower rank) */
int rattle_hip_lpt_assign(const uint64_t *cost, uint32_t n, int nranks, uint32_t *owner_out);

/* Test hook, needs no device: phred_symbol's value `-10*log10(p)+33` (utils.cpp:6-8, before the narrowing to
 * char) through the threshold table the post-MSA kernel bisects and through the host libm.  Returns the number
 * of explicit exceptions the table carries. */
int rattle_hip_debug_phred_symbol(double p, int *table_value, int *libm_value);

/* Test hook: ONE evaluation of the greedy clustering (cluster_together over a list of rectangles, as a greedy step hands them to
 * the device: kernel A's survivor list, the count pass for |common|, the exact rejection on it, the full pass and the verdicts)
 * on the loaded reads, with what it computed on the way.  Rectangle r: seeds x candidates, or, triangular, the seeds against
 * each other (pairs s < c); thr is its bit-vector threshold.  count_pass: 0 = as the driver picks it, 1 = seed-major,
 * 2 = per-pair search, 3 = seed-batch k-mer index.  Only t_s, t_v, use_hc and is_rna of params are read. */
typedef struct {
    const uint32_t *seed_ids;
    uint32_t n_seeds;
    const uint32_t *cand_ids;   /* ignored when triangular */
    uint32_t n_cands;
    int triangular;
    double thr;
} rattle_debug_rect;

typedef struct {
    uint32_t n;
    uint32_t *rect, *seed, *cand;   /* rectangle; seed and candidate index within it */
    uint8_t *strand;
    int32_t *count;                 /* survivors: the count pass's result (|common| or its upper bound); else 0 */
} rattle_debug_pairs;

typedef struct {
    rattle_debug_pairs survivors;   /* kernel A's survivors */
    rattle_debug_pairs kept;        /* the survivors past the exact rejection double(k * count) / min_len >= t_s */
    rattle_debug_pairs hits;        /* accepted pairs */
    uint64_t *counters;             /* [n_rects * 8]: the rectangle's work counters as in rattle_cluster_set */
    int count_pass;                 /* bit 0: the seed-major count pass ran, bit 1: the per-pair search ran, bit 2: the index pass ran */
    uint64_t filter_launches;       /* kernel A launches (one more per survivor-capacity retry) */
    uint64_t oversize_pairs;        /* pairs that went through the oversize full pass */
    /* [hits.n] each, parallel to hits: what the report form of the verdict kernel wrote for the accepted pair (on a context with
       rattle_hip_set_cluster_report on, else NULL) */
    int32_t *hit_bases, *hit_hc_bases;
    double *hit_variance;
} rattle_debug_eval;

int rattle_hip_debug_evaluate(rattle_ctx *ctx, const rattle_cluster_params *params, int count_pass, const rattle_debug_rect *rects,
                              uint32_t n_rects, rattle_debug_eval **out);
void rattle_hip_debug_evaluate_free(rattle_debug_eval *e);

/* Test hook: the post-MSA kernel (fix_msa_ends, column vote, per-read correction or pack consensus) ALONE on a given MSA, launched
 * by the code `correct` launches it with, and everything it wrote.  The MSA is given the way the POA kernel hands it over: per pack
 * its rows (sequences without gaps) and width, per base its MSA column.  In every pack of width > 0 the columns of a row must be
 * strictly increasing and below the width, and the bases A, C, G, T or U; a pack of width 0 is what a skipped pack looks like (its
 * columns are not read).  mode 1: after POA #1 (qualities required; reads corrected), mode 2: after POA #2 / #3 (pack consensus).
 * Only min_occ, gap_occ, err_ratio and vote_order of params are read. */
typedef struct {
    uint32_t n_packs;
    const uint32_t *pack_first;   /* [n_packs+1] row range of each pack, pack_first[0] == 0 */
    const uint32_t *width;        /* [n_packs]   MSA columns */
    const uint64_t *off;          /* [n_rows+1]  base range of each row, off[0] == 0 */
    const uint8_t *seq;           /* bases of all rows back to back */
    const uint8_t *qual;          /* their quality bytes; may be NULL in mode 2 */
    const uint32_t *col;          /* [n_bases]   MSA column of every base */
} rattle_debug_msa;

typedef struct {
    uint32_t n_packs, n_rows;
    int mode;
    uint64_t n_cols;              /* sum of the widths */
    uint64_t *moff;               /* [n_packs] byte offset of the pack's rows x width matrix (a multiple of 16) */
    uint64_t *coff;               /* [n_packs] offset of the pack's columns in the per-column arrays */
    int32_t *rfirst, *rlast;      /* [n_rows]  voting window after fix_msa_ends: first / last column, width / -1 if the row was blanked
                                               (rows of a pack of width 0: 0 / -1) */
    uint32_t *tfront, *tback;     /* [n_rows]  bases fix_msa_ends erased at the front / at the back (mode 1, else NULL) */
    uint32_t *olen;               /* [n_rows]  length of the corrected read (mode 1, else NULL) */
    uint64_t *out_off;            /* [n_rows+1] corrected reads back to back (mode 1, else NULL) */
    uint8_t *out_seq, *out_qual;
    uint8_t *cons;                /* [n_cols]  column winner ('-' where nothing voted) */
    uint8_t *flag;                /* [n_cols]  bit 0: winner's share >= gap_occ, bit 1: >= min_occ (mode 1, else NULL) */
    uint8_t *sym;                 /* [n_cols]  phred_symbol of the winner's mean error (mode 1; meaningful where the winner is a base) */
    double *err;                  /* [n_cols]  the winner's mean error (mode 1; meaningful where the winner is a base) */
    uint32_t *cons_len;           /* [n_packs] length of the pack consensus (mode 2, else NULL) */
    uint8_t *consensus;           /* [n_cols]  the winners without gaps, cons_len[p] bytes at coff[p] (mode 2, else NULL) */
    /* [n_rows] each: the counters of the correction report (mode 1 on a context with rattle_hip_set_correction_report on, else NULL) */
    uint32_t *match, *substituted, *mismatch_kept, *inserted, *deleted, *gap_kept;
} rattle_debug_post;

int rattle_hip_debug_post_msa(rattle_ctx *ctx, const rattle_correct_params *params, int mode /* 1 | 2 */, const rattle_debug_msa *in,
                              rattle_debug_post **out);
void rattle_hip_debug_post_msa_free(rattle_debug_post *p);

/* Test hook: the report form of the post-MSA kernel's mode 2 (the consensus support) ALONE on given MSAs, through the driver's own
 * stage layout and launch.  The MSAs are given and checked as for rattle_hip_debug_post_msa.  sup / dep: a support and a depth for
 * every base, which makes every pack a level-3 pack (rows that are pack consensi); both NULL: level 2 (rows that are reads).
 * Returns per pack the consensus (cons_len[p] bytes at coff[p]) and, at the same index, support and depth of every base -- at level 3
 * also pack_support and pack_depth, at level 2 they are NULL.  On a context with rattle_hip_set_consensus_support off all four are
 * NULL.  Only vote_order of params is read. */
typedef struct {
    uint32_t n_packs;
    const uint32_t *pack_first;   /* [n_packs+1] row range of each pack, pack_first[0] == 0 */
    const uint32_t *width;        /* [n_packs]   MSA columns */
    const uint64_t *off;          /* [n_rows+1]  base range of each row, off[0] == 0 */
    const uint8_t *seq;           /* bases of all rows back to back */
    const uint32_t *col;          /* [n_bases]   MSA column of every base */
    const uint32_t *sup, *dep;    /* [n_bases]   support / depth of every base, or both NULL */
} rattle_debug_support_msa;

typedef struct {
    uint32_t n_packs;
    int level;                    /* 2 | 3 */
    uint64_t n_cols;              /* sum of the widths */
    uint64_t *coff;               /* [n_packs] where the pack's consensus and its values start */
    uint32_t *cons_len;           /* [n_packs] */
    uint8_t *consensus;           /* [n_cols] */
    uint32_t *support, *depth, *pack_support, *pack_depth;   /* [n_cols] */
} rattle_debug_support;

int rattle_hip_debug_consensus_support(rattle_ctx *ctx, const rattle_correct_params *params, const rattle_debug_support_msa *in,
                                       rattle_debug_support **out);
void rattle_hip_debug_consensus_support_free(rattle_debug_support *d);

/* ------------------------------------------------------------------------------------
 * Per-kernel timing measured with HIP events on the stream the kernels run on.
 * kernel: 0 kmer_extract, 1 bv_filter, 2 pair_score, 3 poa_align, 4 post_msa, 5 the per-read reduction of
 * assign (alg_bytes: the bytes of its records copied to the host), 6 pair_align (kernel E; alg_bytes: the sequence bytes read plus
 * the record bytes written), 7 pair_cigar (kernel F; alg_bytes: see align_cigars), 8 and 9 their three-state forms
 * (align_pairs_scored, align_cigars_scored), 10 the abundance EM (csrc/abundance.hip), 11 pair_pileup (kernel G; alg_bytes: see
 * align_pileup).  Accumulated since
 * the last reset: total milliseconds, number of launches, algorithmic bytes moved.
 */
int rattle_hip_kernel_stats(rattle_ctx *ctx, int kernel, double *total_ms, uint64_t *launches, uint64_t *alg_bytes);
int rattle_hip_kernel_stats_reset(rattle_ctx *ctx);
/* (ABI 4) Host wall time of the stages of the calls made on this context since the last reset, in milliseconds:
 * [0] reserved, [1] `correct` stage 1 (POA #1 + correction of every pack, correct.cpp:395-426), [2] stage 2a (POA #2 of the packs of the
 * many-pack clusters, :427-470), [3] stage 2b + 3a (POA #2 of the other packs beside POA #3 of the many-pack clusters, :489-556),
 * [4] stage 3b (POA #3 of the other clusters), [5..7] reserved.  A measurement aid for the benchmark harness (which stage a slow
 * step was slow in); the reference has no counterpart. */
int rattle_hip_stage_ms(rattle_ctx *ctx, double ms_out[8], int reset);

#ifdef __cplusplus
}
#endif
#endif /* RATTLE_HIP_H */
