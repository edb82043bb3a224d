"""The candidate list of `assign` on the device against the oracle's brute force (tests/assign_top_ref.py over the accepted comparisons
of tests/assign_ref.py): every field of every slot and the counts, doubles bit for bit, and in every call the record beside the list
equals plain assign_loaded's.  The cases are those of tests/test_gpu_assign.py: isoform families with every count pass (cuts and
unused slots), a sequence at three target indices (the cut inside a tie, within a batch and across batches), the target batch's
edges with every later slot arriving through the merge, the 401-match pair as slot 0, 1 and 2, empties and thresholds, read chunks in
shuffled order, and no trace left on the context."""
import numpy as np
import pytest

import assign_ref
import assign_top_ref
import constructed
from rattle_amd import synth
from test_gpu_assign import FAMILY_SEED, PASSES, edges_case, family_case, noisy
from test_gpu_cluster_eval import Ref, revcomp, rnd

pytestmark = pytest.mark.gpu


def check(ctx, acc, T, R, K, label, **kw):
    """assign_loaded_top(T, R, K) against the oracle's accepted comparisons acc: the list, the record, and the record of the plain call"""
    rec, cands = ctx.assign_loaded_top(T, R, K, **kw)
    bad = assign_ref.same(rec, ctx.assign_loaded(T, R, **kw))
    assert not bad, (label, "the record differs from assign_loaded's", bad[:8])
    bad = assign_ref.same(rec, assign_ref.reduce_best(len(R), acc))
    assert not bad, (label, "record", bad[:8])
    bad = assign_top_ref.same(cands, assign_top_ref.reduce_top(len(R), acc, K))
    assert not bad, (label, bad[:8])
    return rec, cands


# ---- family ---------------------------------------------------------------------------------------------------------------------
_family = {}


def family_acc(oracle, k, both):
    if k not in _family:
        seqs, T, R = family_case(k, both, FAMILY_SEED[k])
        acc = assign_ref.accepted_comparisons(Ref(oracle, seqs, k, both), T, R, 0.4, 0.2, 1000000.0)
        nt = assign_top_ref.n_targets(len(R), acc)
        assert (nt > 3).sum() >= 20 and ((nt == 1) | (nt == 2)).sum() >= 20, (k, np.bincount(nt))     # cuts, and unused slots
        _family[k] = (seqs, T, R, acc)
    return _family[k]


@pytest.mark.parametrize("count_pass", PASSES)
@pytest.mark.parametrize("k,both", [(10, True), (11, False)], ids=["k10-cdna", "k11-rna"])
def test_family(gpu_ctx, oracle, k, both, count_pass):
    seqs, T, R, acc = family_acc(oracle, k, both)
    gpu_ctx.load_reads(seqs, k, both)
    for K in (1, 2, 3, 8):
        check(gpu_ctx, acc, T, R, K, f"family k={k} {count_pass} K={K}", is_rna=not both, count_pass=count_pass)


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def test_ties(gpu_ctx, oracle):
    """The same sequence at target indices 3, 11 and 17 (one batch; with target_batch = 8 one copy per batch; with 3 and 1 further
    apart): K = 2 keeps 3 and 11 -- the cut falls inside the tie and 17 is dropped, in the batch or in the merge --, K = 3 all three with
    equal score bits.  A target equal to its own reverse complement is ONE candidate, forward.  The reverse complement of a target:
    reverse when both strands are compared, no candidate under is_rna."""
    rng = np.random.default_rng(21)
    tx = [t.tobytes() for t in synth.transcriptome(20, 1, seed=31, exon=(25, 40))[0]]
    half = rnd(rng, 140)
    pal = half + revcomp(half)
    assert revcomp(pal) == pal
    targets = list(tx[:20])
    targets[11] = targets[17] = targets[3]
    targets[9] = pal
    reads = [noisy(rng, targets[3]), targets[3], pal, noisy(rng, pal), revcomp(tx[5]), noisy(rng, revcomp(tx[6])), noisy(rng, tx[12])]
    seqs = targets + reads
    T = np.arange(20, dtype=np.uint32); R = np.arange(20, len(seqs), dtype=np.uint32)
    for both in (True, False):
        acc = assign_ref.accepted_comparisons(Ref(oracle, seqs, 10, both), T, R, 0.4, 0.2, 1000000.0)
        gpu_ctx.load_reads(seqs, 10, both)
        for batch in (0, 8, 1, 3):
            for K in (2, 3):
                rec, c = check(gpu_ctx, acc, T, R, K, f"ties both={both} batch={batch} K={K}", is_rna=not both, target_batch=batch)
                for r in (0, 1):
                    assert c["target"][r].tolist() == [3, 11, 17][:K] and c["count"][r] == K
                    assert len(set(c["score"][r].view(np.uint64).tolist())) == 1 and (c["rev"][r] == 0).all()
                assert c["count"][2] == 1 and c["target"][2, 0] == 9 and c["rev"][2, 0] == 0            # the palindrome: one candidate
                assert c["target"][3, 0] == 9
                if both:
                    assert rec["n_accepted"][2] == 2
                    assert c["target"][4, 0] == 5 and c["rev"][4, 0] == 1 and c["target"][5, 0] == 6 and c["rev"][5, 0] == 1
                else:
                    assert c["count"][4] == 0 and c["count"][5] == 0 and (c["target"][4] == -1).all() and (c["score"][5] == -1.0).all()
                assert c["target"][6, 0] == 12 and c["rev"][6, 0] == 0


# ---- batch edges ----------------------------------------------------------------------------------------------------------------
_edge_acc = {}


@pytest.mark.parametrize("batch", [32, 1])
def test_batch_edges(gpu_ctx, oracle, batch):
    """65 targets in batches of 32 and of 1 (every slot beyond the first then arrives through the merge) against 255, 256 and 257
    reads, K = 4.  The boundary at index 32 lies inside a gene: reads whose best isoform is in the later batch and whose further
    candidates are in the earlier one make the merge put a later batch's entries AHEAD of the call's."""
    E = edges_case(oracle)
    gpu_ctx.load_reads(E["seqs"], 10, True)
    T = np.arange(65, dtype=np.uint32)
    for nr in (255, 256, 257):
        R = np.arange(65, 65 + nr, dtype=np.uint32)
        if nr not in _edge_acc:
            _edge_acc[nr] = assign_ref.accepted_comparisons(E["ref"], T, R, 0.4, 0.2, 1000000.0)
        acc = _edge_acc[nr]
        want = assign_top_ref.reduce_top(nr, acc, 4)
        across = 0
        for r in range(nr):
            t = want["target"][r, :want["count"][r]]
            across += any(t[i] >= 32 and (t[i + 1:] < 32).any() for i in range(len(t)))
        assert across >= 10, across
        check(gpu_ctx, acc, T, R, 4, f"edges batch={batch} nr={nr}", target_batch=batch)


# ---- oversize pairs -------------------------------------------------------------------------------------------------------------
def test_oversize_pairs(gpu_ctx, oracle):
    """The 401-match fragment pair of tests/constructed.py (its res / var come from the oversize relaunch) as (target, read): slot 0
    beside a mutated copy of the target; slot 1 behind a wider fragment of the same sequence at a lower index, which reaches the same
    score; slot 2 behind two such fragments -- absent with K = 2, the last slot with K = 3."""
    rng = np.random.default_rng(8)
    a, b, m = constructed.fragment_pair(10, 700, 401)
    assert m == 401
    at = a.find(b)
    wide = a[max(0, at - 15):at + len(b) + 15]
    wider = a[max(0, at - 30):at + len(b) + 30]
    assert len({a, wide, wider}) == 3
    weak = noisy(rng, a, 0.05, 0.0)
    others = [rnd(rng, 300) for _ in range(6)]
    top = float(len(b) - 1) / float(len(b))
    for label, targets, slot in (("slot 0", others[:3] + [weak] + others[3:] + [a], 0), ("slot 1", [wide] + others + [a], 1),
                                 ("slot 2", [wide] + others[:3] + [wider] + others[3:] + [a], 2)):
        seqs = targets + [b, noisy(rng, others[1])]
        nt = len(targets)
        T = np.arange(nt, dtype=np.uint32); R = np.arange(nt, len(seqs), dtype=np.uint32)
        ref = Ref(oracle, seqs, 10, True)
        acc = assign_ref.accepted_comparisons(ref, T, R, 0.4, 0.2, 1000000.0)
        assert ref.verdicts[(nt - 1, nt, 0)][4] == 401                                 # the pair (a, b): past PS_MCAP = 400
        full = assign_top_ref.reduce_top(len(R), acc, 8)
        assert full["count"][0] >= slot + 1 and full["target"][0, slot] == nt - 1 and full["score"][0, slot] == top
        assert (full["score"][0, :slot] == top).all() and (full["target"][0, :slot] < nt - 1).all()
        gpu_ctx.load_reads(seqs, 10, True)
        assert gpu_ctx.debug_evaluate([(T, R, 0.4)], 0.2)["oversize_pairs"] >= 1
        for batch in (0, 4, 1):
            for cp in PASSES:
                for K in ((2, 3) if slot == 2 else (3,)):
                    _, c = check(gpu_ctx, acc, T, R, K, f"oversize {label} batch={batch} {cp} K={K}", target_batch=batch, count_pass=cp)
                    assert ((c["target"][0] == nt - 1).nonzero()[0].tolist() == [slot]) == (slot < K)
                    assert (nt - 1 in c["target"][0].tolist()) == (slot < K)


# ---- empties and thresholds -----------------------------------------------------------------------------------------------------
def test_empties_and_thresholds(gpu_ctx, oracle):
    """The case of test_gpu_assign.py::test_roles_and_empties: reads longer than their targets, reads shorter than k, empty sides, a t_s
    nothing reaches, a median t_v, use_hc (hc_bases / min_len orders the slots), bv_threshold 0."""
    rng = np.random.default_rng(77)
    tx = [t.tobytes() for t in synth.transcriptome(6, 3, seed=78, exon=(30, 60))[0]]
    tx = [t for t in tx if len(t) >= 260]
    targets = [t[40:240] for t in tx]
    reads = [noisy(rng, tx[i % len(tx)]) if i % 3 else revcomp(noisy(rng, tx[i % len(tx)])) for i in range(60)]
    reads += [b"ACGTACGTA", b"ACGTACGTAC", b"A", rnd(rng, 9)]           # shorter than k, exactly k (no k-mer either), one base
    seqs = targets + reads
    nt = len(targets)
    T = np.arange(nt, dtype=np.uint32); R = np.arange(nt, len(seqs), dtype=np.uint32)
    ref = Ref(oracle, seqs, 10, True)
    gpu_ctx.load_reads(seqs, 10, True)
    K = 2
    acc = assign_ref.accepted_comparisons(ref, T, R, 0.4, 0.2, 1000000.0)
    ntar = assign_top_ref.n_targets(len(R), acc)
    print("[empties] accepting targets per read:", np.bincount(ntar))
    assert (ntar[:60] > K).sum() >= 3 and (ntar[:60] == 1).sum() >= 5 and (ntar[60:] == 0).all()      # cuts, unused slots, no k-mer
    for cp in PASSES:
        _, c = check(gpu_ctx, acc, T, R, K, f"long reads {cp}", count_pass=cp)
        assert (c["count"][60:] == 0).all() and (c["target"][60:] == -1).all()
    check(gpu_ctx, assign_ref.accepted_comparisons(ref, T, R, 0.0, 0.2, 1000000.0), T, R, K, "thr 0", bv_threshold=0.0)
    for t, r in ((T[:0], R), (T, R[:0]), (T[:0], R[:0])):
        _, c = check(gpu_ctx, [], t, r, K, "empty")
        assert c["target"].shape == (len(r), K)
    check(gpu_ctx, [], T, R, K, "t_s 2", t_s=2.0)
    var = np.array([a[7] for a in acc])
    assert len(var) > 50 and var.min() < np.median(var)
    check(gpu_ctx, [], T, R, K, "t_v min", t_v=float(var.min()))
    tv = float(np.median(var))
    mid = assign_ref.accepted_comparisons(ref, T, R, 0.4, 0.2, tv)
    assert 0 < len(mid) < len(acc)
    check(gpu_ctx, mid, T, R, K, "t_v median", t_v=tv)
    hc = assign_ref.accepted_comparisons(ref, T, R, 0.4, 0.2, 1000000.0, use_hc=True)
    want, plain = assign_top_ref.reduce_top(len(R), hc, K), assign_top_ref.reduce_top(len(R), acc, K)
    assert (want["score"] != plain["score"]).any() and (want["target"] != plain["target"]).any()      # the other score orders otherwise
    for cp in ("auto", "index"):
        check(gpu_ctx, hc, T, R, K, f"use_hc {cp}", use_hc=True, count_pass=cp)


# ---- chunks and order -----------------------------------------------------------------------------------------------------------
def test_chunks_and_order(gpu_ctx, oracle):
    """assign_top() on 257 reads in shuffled order, in chunks of 100, 64 and 257 with several target batches, equals one chunk, equals
    assign_loaded_top on the same ids, equals the oracle; the record beside it is assign()'s."""
    E = edges_case(oracle)
    rng = np.random.default_rng(91)
    pool, reads = E["seqs"][:65], E["seqs"][65:]
    tperm = rng.permutation(40); rperm = rng.permutation(257)
    targets = [pool[i] for i in tperm]; shuffled = [reads[i] for i in rperm]
    acc = assign_ref.accepted_comparisons(E["ref"], tperm, 65 + rperm, 0.4, 0.2, 1000000.0)
    K = 3
    want, want_rec = assign_top_ref.reduce_top(257, acc, K), assign_ref.reduce_best(257, acc)
    assert (want["count"] == K).sum() >= 20 and (want["count"] < K).sum() >= 20
    rec, one = gpu_ctx.assign_top(targets, shuffled, K)
    assert not assign_top_ref.same(one, want) and not assign_ref.same(rec, want_rec)
    assert not assign_ref.same(rec, gpu_ctx.assign(targets, shuffled))
    for chunk, batch in ((100, 0), (100, 16), (64, 7), (257, 0), (257, 1), (256, 0)):
        rec, c = gpu_ctx.assign_top(targets, shuffled, K, read_chunk=chunk, target_batch=batch)
        bad = assign_top_ref.same(c, one)
        assert not bad and not assign_ref.same(rec, want_rec), (chunk, batch, bad[:8])
    gpu_ctx.load_reads(targets + shuffled, 10, True)
    check(gpu_ctx, acc, np.arange(40), np.arange(40, 297), K, "loaded")
    ref1 = Ref(oracle, E["seqs"], 10, False)
    acc1 = assign_ref.accepted_comparisons(ref1, tperm, 65 + rperm, 0.4, 0.2, 1000000.0)
    rec, c = gpu_ctx.assign_top(targets, shuffled, K, is_rna=True, read_chunk=100)
    assert not assign_top_ref.same(c, assign_top_ref.reduce_top(257, acc1, K)) and not assign_ref.same(rec, assign_ref.reduce_best(257, acc1))


# ---- no side effect -------------------------------------------------------------------------------------------------------------
def test_assign_top_leaves_the_context_as_it_was(gpu_ctx):
    """cluster_reads before and after an assign_loaded_top on the same loaded reads: the same clusters"""
    seqs = synth.reads(300, 7, 3, True, seed=5, exon=(40, 90))[0]
    seqs.sort(key=lambda s: -len(s))
    gpu_ctx.load_reads(seqs, 10, True)
    ids = np.arange(len(seqs), dtype=np.uint32)
    before = gpu_ctx.cluster_reads()
    rec, c = gpu_ctx.assign_loaded_top(ids[:40], ids[40:], 4, target_batch=16)
    assert (c["count"] > 1).sum() > 0 and (rec["target"] == c["target"][:, 0]).all()          # the reduction ran in between
    after = gpu_ctx.cluster_reads()
    assert before.as_list() == after.as_list() and len(before.main_id) > 3
