"""`assign` on the device against the oracle's brute force (tests/assign_ref.py: cluster_together over every (target, read, strand),
then best / second_score / n_accepted in plain Python): every field of every read, doubles bit for bit.  Families of isoforms where
many targets accept a read, every count pass, ties across strands, targets and target batches, the edges of the target batch and of
kernel A's 32 x 256 tile, pairs past kernel B's LDS match capacity as winner and as runner-up, reads longer than their targets and
shorter than k, empty sides, thresholds that reject everything, read chunks in shuffled order, and no trace left on the context."""
import numpy as np
import pytest

import assign_ref
import constructed
from rattle_amd import synth
from test_gpu_cluster_eval import Ref, revcomp, rnd

pytestmark = pytest.mark.gpu

PASSES = ("auto", "seed", "search", "index")
FAMILY_SEED = {10: 1, 11: 1}           # synth.reads seeds at which the oracle sees >= 20 assigned, unassigned and multiply accepted reads


def noisy(rng, s, sub=0.03, indel=0.01):
    """a read of s: substitutions, and a few single-base insertions / deletions"""
    out = bytearray()
    for b in s:
        u = rng.random()
        if u < indel:
            continue
        if u < indel + sub:
            b = b"ACGT"[int(rng.integers(0, 4))]
        out.append(b)
        if rng.random() < indel:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
    return bytes(out)


def expect(got, want, label):
    bad = assign_ref.same(got, want)
    assert not bad, (label, bad[:8])


# ---- family ---------------------------------------------------------------------------------------------------------------------
def family_case(k, both, seed):
    """600 reads of 12 genes x 3 isoforms; the first 48 reads of the genes 0 .. 8 are the targets, so the reads of the genes 9 .. 11
    have nothing to sit on.  Returns (sequences, target ids, read ids)."""
    seqs, _, tid, _ = synth.reads(600, 12, 3, both, seed=seed, exon=(40, 90))
    gene = synth.transcriptome(12, 3, exon=(40, 90))[1][tid]
    targets = np.nonzero(gene < 9)[0][:48]
    reads = np.setdiff1d(np.arange(len(seqs)), targets)
    return seqs, targets.astype(np.uint32), reads.astype(np.uint32)


_family = {}


def family_ref(oracle, k, both):
    if k not in _family:
        seqs, T, R = family_case(k, both, FAMILY_SEED[k])
        ref = Ref(oracle, seqs, k, both)
        want = assign_ref.brute_force(ref, T, R, 0.4)
        assert len(T) == 48 and (want["target"] >= 0).sum() >= 20 and (want["target"] < 0).sum() >= 20 and (want["n_accepted"] > 1).sum() >= 20
        _family[k] = (seqs, T, R, want)
    return _family[k]


@pytest.mark.parametrize("count_pass", PASSES)
@pytest.mark.parametrize("k,both", [(10, True), (11, False)], ids=["k10-cdna", "k11-rna"])
def test_family(gpu_ctx, oracle, k, both, count_pass):
    seqs, T, R, want = family_ref(oracle, k, both)
    gpu_ctx.load_reads(seqs, k, both)
    got = gpu_ctx.assign_loaded(T, R, is_rna=not both, count_pass=count_pass)
    expect(got, want, f"family k={k} {count_pass}")
    if count_pass == "auto":
        print(f"[family k={k}] assigned {(want['target'] >= 0).sum()}, unassigned {(want['target'] < 0).sum()}, "
              f"accepted by several {(want['n_accepted'] > 1).sum()}, with a runner-up {(want['second_score'] >= 0).sum()}, "
              f"reverse {(want['rev'] == 1).sum()}")


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def test_ties(gpu_ctx, oracle):
    """The same sequence at target indices 3 and 17 (one batch, and with target_batch = 8 two batches apart): 3 wins and the copy is the
    runner-up with the same score.  A target equal to its own reverse complement: forward.  A read that is the reverse complement of
    a target: reverse when both strands are compared, unassigned under is_rna."""
    rng = np.random.default_rng(21)
    tx = [t.tobytes() for t in synth.transcriptome(20, 1, seed=31, exon=(25, 40))[0]]
    half = rnd(rng, 140)
    pal = half + revcomp(half)
    assert revcomp(pal) == pal
    targets = list(tx[:20])
    targets[17] = targets[3]
    targets[9] = pal
    reads = [noisy(rng, targets[3]), targets[3], pal, noisy(rng, pal), revcomp(tx[5]), noisy(rng, revcomp(tx[6])), noisy(rng, tx[12])]
    seqs = targets + reads
    T = np.arange(20, dtype=np.uint32); R = np.arange(20, len(seqs), dtype=np.uint32)
    for both in (True, False):
        ref = Ref(oracle, seqs, 10, both)
        want = assign_ref.brute_force(ref, T, R, 0.4)
        gpu_ctx.load_reads(seqs, 10, both)
        for batch in (0, 8, 1, 3):
            got = gpu_ctx.assign_loaded(T, R, is_rna=not both, target_batch=batch)
            expect(got, want, f"ties both={both} batch={batch}")
            for r in (0, 1):
                assert got["target"][r] == 3 and got["second_score"][r] == got["score"][r] and got["n_accepted"][r] >= 2
            assert got["target"][2] == 9 and got["rev"][2] == 0 and got["target"][3] == 9
            if both:
                assert got["n_accepted"][2] == 2 and got["second_score"][2] == -1.0        # both strands of one target: no runner-up
                assert got["target"][4] == 5 and got["rev"][4] == 1 and got["target"][5] == 6 and got["rev"][5] == 1
            else:
                assert got["target"][4] == -1 and got["target"][5] == -1 and got["n_accepted"][4] == 0
            assert got["target"][6] == 12 and got["rev"][6] == 0


# ---- batch and tile edges -------------------------------------------------------------------------------------------------------
_edges = {}


def edges_case(oracle):
    """65 transcripts (13 genes x 5 isoforms) as the target pool and 257 reads: five of each of the transcripts 0, 30, 31, 32 and 64,
    the rest spread over the pool.  One Ref over all of them: its verdict cache serves every (nt, nr)."""
    if not _edges:
        rng = np.random.default_rng(44)
        pool = [t.tobytes() for t in synth.transcriptome(13, 5, seed=45, exon=(20, 45))[0]]
        assert len(pool) == 65 and len(set(pool)) == 65
        src = [t for t in (0, 30, 31, 32, 64) for _ in range(5)] + [int(x) for x in rng.integers(0, 65, 257 - 25)]
        reads = [noisy(rng, pool[t]) if rng.random() < 0.5 else revcomp(noisy(rng, pool[t])) for t in src]
        seqs = pool + reads
        _edges.update(seqs=seqs, src=np.array(src), ref=Ref(oracle, seqs, 10, True))
    return _edges


@pytest.mark.parametrize("nt", [31, 32, 33, 65])
def test_batch_and_tile_edges(gpu_ctx, oracle, nt):
    """target_batch = 32 with 31, 32, 33 and 65 targets against 255, 256 and 257 reads (kernel A tiles 32 seeds by 256 candidates).  The
    true transcripts of the first 25 reads sit at index 0, at the last index of the first batch, at the first of the second and at the
    last overall (where the pool reaches that far)."""
    E = edges_case(oracle)
    gpu_ctx.load_reads(E["seqs"], 10, True)
    T = np.arange(nt, dtype=np.uint32)
    for nr in (255, 256, 257):
        R = np.arange(65, 65 + nr, dtype=np.uint32)
        want = assign_ref.brute_force(E["ref"], T, R, 0.4)
        got = gpu_ctx.assign_loaded(T, R, target_batch=32)
        expect(got, want, f"edges nt={nt} nr={nr}")
        for t in (0, 30, 31, 32, 64):                                 # the oracle places the chosen reads on the edges they were made for
            if t < nt:
                assert (want["target"][:25][E["src"][:25] == t] == t).sum() >= 3, (nt, t)
        assert (want["target"] < 0).sum() >= (10 if nt < 65 else 0) and (want["n_accepted"] > 1).sum() >= 20


# ---- oversize pairs -------------------------------------------------------------------------------------------------------------
def test_oversize_pairs(gpu_ctx, oracle):
    """The 401-match fragment pair of tests/constructed.py (one match more than kernel B's LDS list holds: the oversize relaunch fills
    its res / var in place) as (target, read).  Its score is (L - 1) / L for the read's length L, the most a comparison with a read of
    L bases can reach, so no target can beat it.  Best of two accepting targets: beside a mutated copy of the target.  Runner-up: a
    wider fragment of the same sequence reaches the same score at a LOWER index and wins the tie; second_score is then the score the
    oversize pass computed, in the same batch and across batches."""
    rng = np.random.default_rng(8)
    a, b, m = constructed.fragment_pair(10, 700, 401)
    assert m == 401
    at = a.find(b)
    wide = a[max(0, at - 15):at + len(b) + 15]
    weak = noisy(rng, a, 0.05, 0.0)
    others = [rnd(rng, 300) for _ in range(6)]
    for label, targets, winner in (("best", others[:3] + [weak] + others[3:] + [a], 7), ("runner-up", [wide] + others + [a], 0)):
        seqs = targets + [b, noisy(rng, others[1])]
        T = np.arange(len(targets), dtype=np.uint32); R = np.arange(len(targets), len(seqs), dtype=np.uint32)
        ref = Ref(oracle, seqs, 10, True)
        want = assign_ref.brute_force(ref, T, R, 0.4)
        assert want["target"][0] == winner and want["n_accepted"][0] >= 2 and want["second_score"][0] > 0
        assert ref.verdicts[(len(targets) - 1, len(targets), 0)][4] == 401           # the pair (a, b): past PS_MCAP = 400
        if label == "runner-up":
            assert want["second_score"][0] == want["score"][0] == float(len(b) - 1) / float(len(b))
        gpu_ctx.load_reads(seqs, 10, True)
        seen = gpu_ctx.debug_evaluate([(T, R, 0.4)], 0.2)
        assert seen["oversize_pairs"] >= 1
        for batch in (0, 4, 1):
            for cp in PASSES:
                expect(gpu_ctx.assign_loaded(T, R, target_batch=batch, count_pass=cp), want, f"oversize {label} batch={batch} {cp}")


# ---- roles and empties ----------------------------------------------------------------------------------------------------------
def test_roles_and_empties(gpu_ctx, oracle):
    rng = np.random.default_rng(77)
    tx = [t.tobytes() for t in synth.transcriptome(6, 3, seed=78, exon=(30, 60))[0]]
    # reads longer than every target: the targets are 200-base windows of the transcripts.  (The bit-vector filter divides by the LARGER
    # 6-mer set of the two, cluster.cpp:19: at 0.4 a target much shorter than the read does not pass it whatever its role.)
    tx = [t for t in tx if len(t) >= 260]
    targets = [t[40:240] for t in tx]
    reads = [noisy(rng, tx[i % len(tx)]) if i % 3 else revcomp(noisy(rng, tx[i % len(tx)])) for i in range(60)]
    reads += [b"ACGTACGTA", b"ACGTACGTAC", b"A", rnd(rng, 9)]           # shorter than k, exactly k (no k-mer either), one base
    assert len(tx) >= 10 and max(map(len, targets)) < min(map(len, reads[:60]))
    seqs = targets + reads
    nt = len(targets)
    T = np.arange(nt, dtype=np.uint32); R = np.arange(nt, len(seqs), dtype=np.uint32)
    ref = Ref(oracle, seqs, 10, True)
    gpu_ctx.load_reads(seqs, 10, True)
    want = assign_ref.brute_force(ref, T, R, 0.4)
    assert (want["target"][:60] >= 0).sum() >= 40 and (want["target"][60:] == -1).all()
    assert (want["min_len"][:60][want["target"][:60] >= 0] == 200).all()      # the target is the shorter one
    for cp in PASSES:
        expect(gpu_ctx.assign_loaded(T, R, count_pass=cp), want, f"long reads {cp}")
    # bv_threshold 0: the forward bypass lets every pair through, the short reads included
    expect(gpu_ctx.assign_loaded(T, R, bv_threshold=0.0), assign_ref.brute_force(ref, T, R, 0.0), "thr 0")
    # empty sides
    for t, r in ((T[:0], R), (T, R[:0]), (T[:0], R[:0])):
        got = gpu_ctx.assign_loaded(t, r)
        expect(got, assign_ref.unassigned(len(r)), "empty")
    # a t_s nothing reaches; a t_v at the smallest variance of an accepted comparison (var < t_v: nothing), and one in the middle
    expect(gpu_ctx.assign_loaded(T, R, t_s=2.0), assign_ref.unassigned(len(R)), "t_s 2")
    var = np.array([a[7] for a in assign_ref.accepted_comparisons(ref, T, R, 0.4, 0.2, 1000000.0)])
    assert len(var) > 50 and var.min() < np.median(var)
    expect(gpu_ctx.assign_loaded(T, R, t_v=float(var.min())), assign_ref.unassigned(len(R)), "t_v min")
    mid = assign_ref.brute_force(ref, T, R, 0.4, t_v=float(np.median(var)))
    assert 0 < (mid["target"] >= 0).sum() and (mid["n_accepted"] < want["n_accepted"]).any()
    expect(gpu_ctx.assign_loaded(T, R, t_v=float(np.median(var))), mid, "t_v median")
    # use_hc: the score is hc_bases / min_len
    hc = assign_ref.brute_force(ref, T, R, 0.4, use_hc=True)
    assert (hc["score"] != want["score"]).any()
    for cp in ("auto", "index"):
        expect(gpu_ctx.assign_loaded(T, R, use_hc=True, count_pass=cp), hc, f"use_hc {cp}")


# ---- chunks and order -----------------------------------------------------------------------------------------------------------
def test_chunks_and_order(gpu_ctx, oracle):
    """assign() on 257 reads in shuffled order, 100 at a time, equals one chunk, equals assign_loaded on the same ids, equals the oracle."""
    E = edges_case(oracle)
    rng = np.random.default_rng(91)
    pool, reads = E["seqs"][:65], E["seqs"][65:]
    tperm = rng.permutation(40); rperm = rng.permutation(257)
    targets = [pool[i] for i in tperm]; shuffled = [reads[i] for i in rperm]
    assert [len(s) for s in shuffled] != sorted((len(s) for s in shuffled), reverse=True)
    want = assign_ref.brute_force(E["ref"], tperm, 65 + rperm, 0.4)
    one = gpu_ctx.assign(targets, shuffled)
    expect(one, want, "one chunk")
    for chunk, batch in ((100, 0), (100, 16), (64, 7), (257, 0), (256, 0)):
        expect(gpu_ctx.assign(targets, shuffled, read_chunk=chunk, target_batch=batch), want, f"chunk {chunk} batch {batch}")
    gpu_ctx.load_reads(targets + shuffled, 10, True)
    expect(gpu_ctx.assign_loaded(np.arange(40), np.arange(40, 297)), want, "loaded")
    # under is_rna the reads are indexed on one strand
    ref1 = Ref(oracle, E["seqs"], 10, False)
    expect(gpu_ctx.assign(targets, shuffled, is_rna=True, read_chunk=100), assign_ref.brute_force(ref1, tperm, 65 + rperm, 0.4), "rna chunks")


# ---- no side effect -------------------------------------------------------------------------------------------------------------
def test_assign_leaves_the_context_as_it_was(gpu_ctx):
    """cluster_reads before and after an assign on the same loaded reads: the same clusters, and with the report on the same report."""
    seqs = synth.reads(300, 7, 3, True, seed=5, exon=(40, 90))[0]
    seqs.sort(key=lambda s: -len(s))
    gpu_ctx.load_reads(seqs, 10, True)
    ids = np.arange(len(seqs), dtype=np.uint32)
    for report in (False, True):
        gpu_ctx.set_cluster_report(report)
        try:
            before = gpu_ctx.cluster_reads()
            got = gpu_ctx.assign_loaded(ids[:40], ids[40:], target_batch=16)
            assert (got["target"] >= 0).sum() > 0 and got["n_accepted"].sum() > 0          # the reduction ran in between
            after = gpu_ctx.cluster_reads()
        finally:
            gpu_ctx.set_cluster_report(False)
        assert before.as_list() == after.as_list() and len(before.main_id) > 3
        assert (before.report() is None) == (not report)
        if report:
            a, b = before.report(), after.report()
            assert len(a["into"]) == len(seqs) - len(before.main_id)
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), f
