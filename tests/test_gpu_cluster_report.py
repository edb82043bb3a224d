"""The cluster report end to end (rattle_hip_set_cluster_report / rattle_hip_cluster_report): every absorption of the greedy
clustering is one join, and the joins alone rebuild the cluster set.

600 synthetic reads of 21 transcripts (7 genes x 3 isoforms, exons of 65 .. 115 nt: reads of about 300 .. 700 nt), on both strands and,
in a second run, on one (is_rna); default thresholds.  The read seed was picked with the oracle so that the merge passes do absorb
clusters (the oracle's clustering stopped after the initial pass has more clusters than the full one): joins with pass >= 1 exist.

For every entry point the report is held to
  (a) the cluster set: equal to the one made with the switch off, and to the oracle's;
  (b) n_joins == n_items - n_clusters;
  (c) per join: bases / hc_bases / variance are oracle.pair_score(into, absorbed, strand) bit for bit, score == bases / min_len in
      double arithmetic, score >= t_s, variance < t_v and not NaN, bv_threshold the pass's threshold B, B - f, ..., 0;
  (d) the replay: from singletons with rev 0, every join in order XORs its rev into the members of the cluster holding `absorbed` and
      appends them to the cluster holding `into`; what is left are the set's clusters, cluster by cluster, as (read, rev) sets;
  (e) the order: by pass, then by the absorbed item's position in that pass's item list."""
import ctypes as C
import threading

import numpy as np
import pytest

from rattle_amd import _lib, synth
from rattle_amd.api import Context, pack_reads

pytestmark = pytest.mark.gpu

K, ISO_K = 10, 11
T_S, T_V, ISO_T_S, ISO_T_V = 0.2, 1000000.0, 0.3, 25.0
BV_B, BV_MIN, BV_F = 0.4, 0.2, 0.05
READ_SEED = 3


def thresholds_by_pass(B=BV_B, b=BV_MIN, f=BV_F):
    """the bit-vector threshold of pass 0, 1, ... (cluster.cpp:171, :251-255), in the driver's own double arithmetic"""
    out, t, last = [B], B - f, False
    while t >= b or last:
        out.append(t)
        if last:
            break
        t = t - f
        if t < b:
            last, t = True, 0.0
    return out


@pytest.fixture(scope="module")
def data():
    """reads in processing order (stable, longest first) and the same reads shuffled, with the order that sorts them"""
    seqs = synth.reads(600, 7, 3, True, seed=READ_SEED, exon=(65, 115))[0]
    rna = synth.reads(300, 7, 3, False, seed=READ_SEED + 1, exon=(65, 115))[0]
    by_len = lambda s: [s[i] for i in sorted(range(len(s)), key=lambda i: -len(s[i]))]
    rng = np.random.default_rng(8)
    shuffled = [seqs[i] for i in rng.permutation(len(seqs))]
    order = sorted(range(len(shuffled)), key=lambda i: -len(shuffled[i]))
    return {"cdna": by_len(seqs), "rna": by_len(rna), "shuffled": shuffled, "order": order}


@pytest.fixture(scope="module")
def scorer(oracle):
    cache = {}

    def score(a, b, k, strand):
        key = (a, b, k, int(strand))
        if key not in cache:
            cache[key] = oracle.pair_score(a, b, k, int(strand), dist_cap=1)[:4]
        return cache[key]
    return score


def members(cl):
    return [frozenset((s[0], s[1]) for s in mem) for _, mem in cl.as_list()]


def select(rep, mask):
    return {f: v[mask] for f, v in rep.items()}


def check_joins(rep, seq_of, item_ids, want_members, scorer, k=K, t_s=T_S, t_v=T_V, level=0, label=""):
    """(b) .. (e) for one clustering: rep its joins, seq_of[id] the read behind an id, item_ids the ids in the item order of the initial
    pass, want_members the cluster set's (id, rev) sets in cluster order"""
    n = len(rep["into"])
    assert n == len(item_ids) - len(want_members), (label, n, len(item_ids), len(want_members))                        # (b)
    assert (rep["level"] == level).all()
    thr = thresholds_by_pass()
    # (c)
    for q in range(n):
        a, b = int(rep["into"][q]), int(rep["absorbed"][q])
        bases, hc, nd, var = scorer(seq_of[a], seq_of[b], k, rep["rev"][q])
        got = (int(rep["bases"][q]), int(rep["hc_bases"][q]), rep["variance"][q:q + 1].view(np.uint64)[0])
        assert got == (bases, hc, np.array([var]).view(np.uint64)[0]), (label, q, a, b, got, (bases, hc, var))
        mn = min(len(seq_of[a]), len(seq_of[b]))
        assert int(rep["min_len"][q]) == mn and rep["score"][q] == float(bases) / float(mn), (label, q)
        assert rep["bv_threshold"][q] == thr[int(rep["pass"][q])], (label, q, rep["bv_threshold"][q], int(rep["pass"][q]))
    assert (rep["score"] >= t_s).all() and (rep["variance"] < t_v).all() and not np.isnan(rep["variance"]).any()
    # (d) + (e)
    clusters = [[(i, 0)] for i in item_ids]
    where = {i: c for i, c in zip(item_ids, clusters)}
    assert (np.diff(rep["pass"].astype(np.int64)) >= 0).all(), label
    for p in np.unique(rep["pass"]):
        at = {id(c): x for x, c in enumerate(clusters)}
        gone, last_item = set(), -1
        for q in np.nonzero(rep["pass"] == p)[0]:
            src, dst = where[int(rep["absorbed"][q])], where[int(rep["into"][q])]
            assert src is not dst and id(src) not in gone and id(dst) not in gone, (label, q)
            assert at[id(src)] > last_item, (label, "order within pass", int(p), q)                                     # (e)
            last_item = at[id(src)]
            moved = [(i, r ^ int(rep["rev"][q])) for i, r in src]
            dst.extend(moved)
            for i, _ in moved:
                where[i] = dst
            gone.add(id(src))
        clusters = [c for c in clusters if id(c) not in gone]
    assert [frozenset(c) for c in clusters] == want_members, label
    return int((rep["pass"] >= 1).sum())


def plain_and_reported(gpu_ctx, call):
    """call() with the switch off, then on: the two cluster sets (equal) -- the second with its report"""
    gpu_ctx.set_cluster_report(False)
    off = call()
    gpu_ctx.set_cluster_report(True)
    try:
        on = call()
    finally:
        gpu_ctx.set_cluster_report(False)
    if isinstance(off, tuple):          # (clusters, gene ids, number of genes): the caller compares
        return off, on
    assert off.report() is None
    assert on.as_list() == off.as_list() and on.report() is not None
    return off, on


@pytest.mark.parametrize("mode", ["cdna", "rna"])
def test_cluster_reads(gpu_ctx, oracle, data, scorer, mode):
    seqs, is_rna = data[mode], mode == "rna"
    gpu_ctx.load_reads(seqs, K, not is_rna)
    off, on = plain_and_reported(gpu_ctx, lambda: gpu_ctx.cluster_reads(is_rna=is_rna))
    want, _ = oracle.cluster_reads(seqs, k=K, is_rna=is_rna)
    assert on.as_list() == want                                                                                       # (a)
    merged = check_joins(on.report(), seqs, list(range(len(seqs))), members(on), scorer, label=mode)
    if is_rna:
        assert not on.report()["rev"].any()
    else:
        # the merge passes absorb clusters: the oracle's clustering without them (cluster.cpp:171 never entered) has more clusters
        initial_only, _ = oracle.cluster_reads(seqs, k=K, bvb=BV_B)
        assert merged >= 1 and merged == len(initial_only) - len(want), (merged, len(initial_only), len(want))
        assert on.report()["rev"].any() and not on.report()["rev"].all()
    print(f"[cluster report {mode}] {len(seqs)} reads, {len(want)} clusters, {len(on.report()['into'])} joins, {merged} in merge passes")
    # off again after on: no report again
    assert gpu_ctx.cluster_reads(is_rna=is_rna).report() is None


def test_cluster_subset_and_subsets(gpu_ctx, oracle, data, scorer):
    """ids are positions in the subset; three subsets in one call (lockstep jobs), one of a single read: no joins"""
    seqs = data["cdna"]
    n = len(seqs)
    gpu_ctx.load_reads(seqs, K, True)
    sub = np.arange(0, n, 2, dtype=np.uint32)
    off, on = plain_and_reported(gpu_ctx, lambda: gpu_ctx.cluster_reads(subset=sub))
    sseq = [seqs[i] for i in sub]
    assert on.as_list() == oracle.cluster_reads(sseq, k=K)[0]
    check_joins(on.report(), sseq, list(range(len(sub))), members(on), scorer, label="subset")
    subsets = [np.arange(0, n, 3, dtype=np.uint32)[:150], np.array([5], np.uint32), np.arange(1, n, 3, dtype=np.uint32)]
    gpu_ctx.set_cluster_report(False)
    plain = gpu_ctx.cluster_subsets(subsets)
    assert all(c.report() is None for c in plain)
    gpu_ctx.set_cluster_report(True)
    try:
        got = gpu_ctx.cluster_subsets(subsets)
    finally:
        gpu_ctx.set_cluster_report(False)
    for t, (ids, cl, pl) in enumerate(zip(subsets, got, plain)):
        sseq = [seqs[i] for i in ids]
        assert cl.as_list() == pl.as_list() == oracle.cluster_reads(sseq, k=K)[0]
        check_joins(cl.report(), sseq, list(range(len(ids))), members(cl), scorer, label=f"subsets[{t}]")
    assert len(got[1].report()["into"]) == 0 and len(got[0].report()["into"]) > 0 and len(got[2].report()["into"]) > 0


def test_cluster_unsorted(gpu_ctx, oracle, data, scorer):
    """shuffled input: ids of the joins in the caller's order, like the members"""
    reads, order = data["shuffled"], data["order"]
    cat, off_ = pack_reads(reads)
    off, on = plain_and_reported(gpu_ctx, lambda: gpu_ctx.cluster_unsorted_packed(cat, off_, k=K))
    want, _ = oracle.cluster_reads([reads[i] for i in order], k=K)
    assert on.as_list() == [((order[m[0]], m[1], -1), [(order[s[0]], s[1], -1) for s in mem]) for m, mem in want]
    merged = check_joins(on.report(), reads, list(order), members(on), scorer, label="unsorted")
    assert merged >= 1


def test_cluster_iso_unsorted(gpu_ctx, data, scorer):
    """level-0 joins of the gene clustering (n - n_genes), then the level-1 joins of every gene in gene order (n - n_clusters in all)"""
    reads, order = data["shuffled"], data["order"]
    n = len(reads)
    pos = {r: p for p, r in enumerate(order)}
    cat, off_ = pack_reads(reads)
    (cl0, gid0, ng0), (cl, gid, ng) = plain_and_reported(gpu_ctx, lambda: gpu_ctx.cluster_iso_unsorted_packed(cat, off_, k=K, iso_k=ISO_K))
    assert cl0.report() is None and cl.as_list() == cl0.as_list() and list(gid) == list(gid0) and ng == ng0
    rep = cl.report()
    lv = rep["level"]
    assert (np.diff(lv.astype(np.int64)) >= 0).all() and int((lv == 0).sum()) == n - ng and int((lv == 1).sum()) == n - len(cl.main_id)
    # level 0 is the plain clustering of the same reads
    gene = gpu_ctx.cluster_unsorted_packed(cat, off_, k=K)
    assert len(gene.main_id) == ng
    check_joins(select(rep, lv == 0), reads, list(order), members(gene), scorer, label="iso level 0")
    # level 1, gene by gene: every gene's reads in its subset order (longest first, ties: the later processing position first)
    gene_of = {}
    for g, (_, mem) in enumerate(gene.as_list()):
        for s in mem:
            gene_of[s[0]] = g
    one = select(rep, lv == 1)
    jg = np.array([gene_of[int(i)] for i in one["into"]], np.int64)
    assert (np.diff(jg) >= 0).all() and all(gene_of[int(a)] == g for a, g in zip(one["absorbed"], jg))
    mem_all = members(cl)
    genes_checked = 0
    for g, (_, mem) in enumerate(gene.as_list()):
        ids = sorted((s[0] for s in mem), key=lambda r: (-len(reads[r]), -pos[r]))
        want = [m for m, gg in zip(mem_all, gid) if gg == g]
        check_joins(select(one, jg == g), reads, ids, want, scorer, k=ISO_K, t_s=ISO_T_S, t_v=ISO_T_V, level=1, label=f"iso gene {g}")
        genes_checked += 1
    assert genes_checked == ng and len(cl.main_id) > ng


class ThreadExchange:
    """an all-gather-v on host buffers between the threads of this process"""

    def __init__(self, n):
        self.n, self.bar, self.send = n, threading.Barrier(n), [b""] * n

    def fn(self, rank):
        def f(user, send, send_bytes, recv, recv_bytes):
            try:
                self.send[rank] = C.string_at(send, send_bytes) if send_bytes else b""
                self.bar.wait(timeout=120)
                at = 0
                for r in range(self.n):
                    if recv_bytes[r]:
                        C.memmove(recv + at, self.send[r], int(recv_bytes[r]))
                    at += int(recv_bytes[r])
                self.bar.wait(timeout=120)
                return 0
            except Exception:          # never unwind through the C frame
                return 1
        return _lib.ALLGATHERV_FN(f)


def test_a_sharded_job_refuses_the_report_on_every_rank(data):
    """world of two over the host transport, both ranks on the one GPU: with the switch on every clustering entry point is a state
    error before any collective (no rank waits for another); with it off again the same contexts run a sharded job"""
    seqs = data["cdna"][:200]
    cat, off = pack_reads(seqs)
    X = ThreadExchange(2)
    results, errors = [None, None], [[], []]

    def rank(r):
        c = Context(0)
        try:
            thunk = X.fn(r)
            _lib.check(c.lib.rattle_hip_set_exchange(c.h, r, 2, thunk, None))
            c.load_reads(seqs, K, True)
            c.set_cluster_report(True)
            sub = np.arange(0, 100, dtype=np.uint32)
            for name, call in (("cluster_reads", lambda: c.cluster_reads()), ("cluster_subset", lambda: c.cluster_reads(subset=sub)),
                               ("cluster_subsets", lambda: c.cluster_subsets([sub, sub[:10]])),
                               ("cluster_unsorted", lambda: c.cluster_unsorted_packed(cat, off)),
                               ("cluster_iso_unsorted", lambda: c.cluster_iso_unsorted_packed(cat, off))):
                try:
                    call()
                    errors[r].append((name, "no error"))
                except _lib.RattleError as e:
                    if "error -3" not in str(e) or "one rank of several" not in str(e):
                        errors[r].append((name, str(e)))
            c.set_cluster_report(False)
            c.load_reads(seqs, K, True)
            results[r] = c.cluster_reads().as_list()
        except Exception as e:
            errors[r].append(("rank", repr(e)))
            X.bar.abort()
        finally:
            c.close()

    th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert errors == [[], []], errors
    single = Context(0)
    try:
        single.load_reads(seqs, K, True)
        want = single.cluster_reads().as_list()
    finally:
        single.close()
    assert results[0] == want and results[1] == want
