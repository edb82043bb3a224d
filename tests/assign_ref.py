"""The oracle's side of `assign` (include/rattle_hip.h): every (target, read, strand) through cluster_together as `Ref` of
tests/test_gpu_cluster_eval.py restates it -- the bit-vector filter (Ref.tables) and the score / variance verdict of oracle.pair_score
(Ref.verdict) -- and, on top, the per-read reduction in plain Python.  No count bound, no batches, no device: the brute force the
GPU tests hold the library to, field by field and bit by bit."""
import numpy as np

FIELDS = (("target", np.int32), ("rev", np.uint8), ("bases", np.int32), ("hc_bases", np.int32), ("min_len", np.uint32),
          ("score", np.float64), ("variance", np.float64), ("second_score", np.float64), ("n_accepted", np.uint32))


def unassigned(n):
    rec = {f: np.zeros(n, t) for f, t in FIELDS}
    rec["target"][:] = -1
    rec["score"][:] = -1.0
    rec["second_score"][:] = -1.0
    return rec


def reduce_best(n_reads, accepted):
    """accepted: (read, target, strand, score, bases, hc_bases, min_len, variance) of every accepted comparison, in any order.
    best: the largest score, ties to the lowest target, then forward; second_score: the largest score of another target, else -1."""
    per = [[] for _ in range(n_reads)]
    for a in accepted:
        per[a[0]].append(a)
    rec = unassigned(n_reads)
    for r, got in enumerate(per):
        if not got:
            continue
        best = min(got, key=lambda a: (-a[3], a[1], a[2]))
        others = [a[3] for a in got if a[1] != best[1]]
        for f, v in zip(("target", "rev", "score", "bases", "hc_bases", "min_len", "variance"), best[1:]):
            rec[f][r] = v
        rec["second_score"][r] = max(others) if others else -1.0
        rec["n_accepted"][r] = len(got)
    return rec


def accepted_comparisons(ref, tids, rids, thr, t_s, t_v, use_hc=False):
    """every (t, strand) of every read that cluster_together(T[t], R[r]) accepts; ref: a Ref over the loaded reads"""
    tids = np.asarray(tids, np.int64); rids = np.asarray(rids, np.int64)
    if len(tids) == 0 or len(rids) == 0:
        return []
    surv = ref.tables(tids, rids, thr, False)[0]
    out = []
    for st in range(len(surv)):
        for s, c in zip(*np.nonzero(surv[st])):
            i, j = int(tids[s]), int(rids[c])
            if min(len(ref.reads[i]), len(ref.reads[j])) == 0:
                continue                                              # 0 / 0: NaN, never accepted
            if ref.verdict(i, j, st, t_s, t_v, use_hc)[0]:
                bases, hc, _, var, _ = ref.verdicts[(i, j, st)]
                mn = min(len(ref.reads[i]), len(ref.reads[j]))
                out.append((int(c), int(s), st, float(hc if use_hc else bases) / float(mn), bases, hc, mn, var))
    return out


def brute_force(ref, tids, rids, thr, t_s=0.2, t_v=1000000.0, use_hc=False):
    return reduce_best(len(rids), accepted_comparisons(ref, tids, rids, thr, t_s, t_v, use_hc))


def same(got, want):
    """every field of every read; doubles by their bits.  Returns the list of differences (empty: equal)."""
    bad = []
    for f, t in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.shape != w.shape:
            bad.append((f, "shape", g.shape, w.shape))
            continue
        ne = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0] if t is np.float64 else np.nonzero(g != w)[0]
        bad += [(f, int(r), g[r], w[r]) for r in ne[:5]]
    return bad
