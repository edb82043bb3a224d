"""The oracle's side of the candidate list of `assign` (include/rattle_hip.h, "The candidate list"): over the accepted comparisons of
tests/assign_ref.py, in plain Python, collapse per target (the better strand, forward on a tie), sort (score descending, ties to the
lower target index), cut at K.  No batches, no device."""
import numpy as np

FIELDS = (("target", np.int32), ("rev", np.uint8), ("bases", np.int32), ("hc_bases", np.int32), ("min_len", np.uint32),
          ("score", np.float64), ("variance", np.float64))


def unused(n, K):
    c = {f: np.zeros((n, K), t) for f, t in FIELDS}
    c["count"] = np.zeros(n, np.uint32)
    c["target"][:] = -1
    c["score"][:] = -1.0
    return c


def ranked(got):
    """the accepted comparisons of ONE read as its full candidate list: one per target, in order"""
    per = {}
    for a in got:
        b = per.get(a[1])
        if b is None or (-a[3], a[2]) < (-b[3], b[2]):
            per[a[1]] = a
    return sorted(per.values(), key=lambda a: (-a[3], a[1]))


def reduce_top(n_reads, accepted, K):
    """accepted: (read, target, strand, score, bases, hc_bases, min_len, variance) of every accepted comparison, in any order"""
    per = [[] for _ in range(n_reads)]
    for a in accepted:
        per[a[0]].append(a)
    c = unused(n_reads, K)
    for r, got in enumerate(per):
        lst = ranked(got)[:K]
        c["count"][r] = len(lst)
        for j, a in enumerate(lst):
            for f, v in zip(("target", "rev", "score", "bases", "hc_bases", "min_len", "variance"), a[1:]):
                c[f][r, j] = v
    return c


def n_targets(n_reads, accepted):
    """accepting targets per read"""
    seen = [set() for _ in range(n_reads)]
    for a in accepted:
        seen[a[0]].add(a[1])
    return np.array([len(s) for s in seen], np.int64)


def same(got, want):
    """every field of every slot and the counts; doubles by their bits.  Returns the list of differences (empty: equal)."""
    bad = []
    for f, t in FIELDS + (("count", np.uint32),):
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append((f, "shape", g.shape, g.dtype, w.shape, w.dtype))
            continue
        ne = np.argwhere(g.view(np.uint64) != w.view(np.uint64)) if t is np.float64 else np.argwhere(g != w)
        bad += [(f, tuple(int(x) for x in at), g[tuple(at)], w[tuple(at)]) for at in ne[:5]]
    return bad
