"""The abundance rule (include/rattle_hip.h, "abundance"; DESIGN.md "abundance") twice: `scalar`, plain Python ints and floats read after
read, and `vector`, numpy on uint64 with np.add.at.  Integer fixed point: an abundance is a whole number of units of 2^-32 read, every
read hands out exactly ONE = 2^32 units per iteration, so sums are exact in any order and the two forms -- and the device -- agree bit
for bit.  Both return the dict Context.abundance returns."""
import numpy as np

ONE = 1 << 32
FIELDS = ("units", "est_reads", "cpm", "compatible_reads", "delta", "posterior", "iterations", "converged", "n_placed")


def compatible(cands, ratio):
    """[n, k] bool: slot j < count[r] with score[r, j] >= ratio * score[r, 0] (one double multiply, one compare); slot 0 of a read
    with a candidate always"""
    count = np.asarray(cands["count"], np.int64)
    score = np.asarray(cands["score"], np.float64)
    n, k = score.shape
    with np.errstate(invalid="ignore"):
        ok = score >= (np.float64(ratio) * score[:, :1])
    ok[:, 0] = True
    return ok & (np.arange(k)[None, :] < count[:, None])


def tol_units(tol):
    return int(float(tol) * 4294967296.0)


def _result(A, compat, deltas, post, converged, n_placed):
    A = [int(a) for a in A]
    return {"units": np.array(A, np.uint64), "est_reads": np.array([float(a) / 4294967296.0 for a in A], np.float64),
            "cpm": np.array([float(a) / float(n_placed * ONE) * 1e6 if n_placed else 0.0 for a in A], np.float64),
            "compatible_reads": np.array(compat, np.uint32), "delta": np.array(deltas, np.uint64), "posterior": post,
            "iterations": len(deltas), "converged": int(converged), "n_placed": int(n_placed)}


def _empty(n, k, nt):
    return _result([0] * nt, [0] * nt, [], np.zeros((n, k)), True, 0)


def scalar(cands, n_targets, ratio=0.95, tol=1e-3, max_iters=1000, states=None):
    """the rule read after read; states: a list that receives the state after every iteration (for the tests of the mass)"""
    target = np.asarray(cands["target"], np.int64)
    n, k = target.shape
    if n == 0 or n_targets == 0:
        return _empty(n, k, n_targets)
    ok = compatible(cands, ratio)
    reads = [[int(target[r, j]) if ok[r, j] else -1 for j in range(k)] for r in range(n)]
    placed = [r for r in range(n) if reads[r][0] >= 0]
    A = [0] * n_targets
    compat = [0] * n_targets
    for r in placed:
        slots = [j for j in range(k) if reads[r][j] >= 0]
        s = ONE // len(slots)
        for j in slots:
            A[reads[r][j]] += s if j else ONE - s * (len(slots) - 1)
        for t in set(reads[r][j] for j in slots):
            compat[t] += 1

    def shares(r, A):
        sh = [0] * k
        D = sum(A[reads[r][j]] for j in range(k) if reads[r][j] >= 0)
        for j in range(1, k):
            if reads[r][j] >= 0:
                sh[j] = int(float(A[reads[r][j]]) / float(D) * 4294967296.0)
        sh[0] = max(0, ONE - sum(sh))
        return sh

    lim = tol_units(tol)
    deltas, converged = [], False
    while len(deltas) < max_iters and not converged:
        B = [0] * n_targets
        for r in placed:
            for j, v in enumerate(shares(r, A)):
                if reads[r][j] >= 0:
                    B[reads[r][j]] += v
        deltas.append(max(abs(b - a) for a, b in zip(A, B)))
        A = B
        if states is not None:
            states.append(list(A))
        converged = deltas[-1] <= lim
    post = np.zeros((n, k))
    for r in placed:
        for j, v in enumerate(shares(r, A)):
            post[r, j] = float(v) / 4294967296.0
    return _result(A, compat, deltas, post, converged, len(placed))


def vector(cands, n_targets, ratio=0.95, tol=1e-3, max_iters=1000):
    """the same rule on whole arrays"""
    target = np.asarray(cands["target"], np.int64)
    n, k = target.shape
    if n == 0 or n_targets == 0:
        return _empty(n, k, n_targets)
    ok = compatible(cands, ratio)
    T = np.where(ok, target, 0)
    c = ok.sum(1).astype(np.uint64)
    placed = c > 0
    s = np.where(placed, np.uint64(ONE) // np.maximum(c, np.uint64(1)), np.uint64(0))
    start = np.where(ok, s[:, None], np.uint64(0)).astype(np.uint64)
    start[:, 0] = np.where(placed, np.uint64(ONE) - s * (np.maximum(c, np.uint64(1)) - np.uint64(1)), np.uint64(0))
    A = np.zeros(n_targets, np.uint64)
    np.add.at(A, T[ok], start[ok])
    compat = np.zeros(n_targets, np.int64)
    first = ok.copy()
    for j in range(1, k):
        for i in range(j):
            first[:, j] &= ~(ok[:, i] & (target[:, i] == target[:, j]))
    np.add.at(compat, T[first], 1)

    def shares(A):
        a = np.where(ok, A[T], np.uint64(0)).astype(np.uint64)
        D = a.sum(1, dtype=np.uint64)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = a.astype(np.float64) / D.astype(np.float64)[:, None] * 4294967296.0
        sh = np.where(ok, q, 0.0).astype(np.uint64)
        sh[:, 0] = 0
        rest = sh.sum(1, dtype=np.uint64)
        sh[:, 0] = np.where(placed & (rest < np.uint64(ONE)), np.uint64(ONE) - np.minimum(rest, np.uint64(ONE)), np.uint64(0))
        return sh

    lim = tol_units(tol)
    deltas, converged = [], False
    while len(deltas) < max_iters and not converged:
        sh = shares(A)
        B = np.zeros(n_targets, np.uint64)
        np.add.at(B, T[ok], sh[ok])
        deltas.append(int(np.where(B > A, B - A, A - B).max()))
        A = B
        converged = deltas[-1] <= lim
    post = np.where(ok, shares(A).astype(np.float64) / 4294967296.0, 0.0)
    return _result(A, compat, deltas, post, converged, int(placed.sum()))


def same(a, b):
    """the first field in which two results differ by their bits, or None"""
    for f in FIELDS:
        x, y = a[f], b[f]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                return f
        elif x != y:
            return f
    return None


def lists(n, k, n_targets, rng, family=8, skew=1.2, empty=0.0, ratio=0.95):
    """hand-built candidate lists without sequences: every read draws a family of `family` neighbouring targets by a skewed draw, takes
    up to k distinct members, the scores descending from a random top, some below ratio * top; a share `empty` of the reads has none"""
    nf = max(1, n_targets // family)
    w = 1.0 / np.arange(1, nf + 1) ** skew
    fam = rng.choice(nf, size=n, p=w / w.sum())
    count = np.zeros(n, np.uint32)
    target = np.full((n, k), -1, np.int32)
    score = np.full((n, k), -1.0)
    for r in range(n):
        if rng.random() < empty:
            continue
        members = np.arange(fam[r] * family, min(n_targets, (fam[r] + 1) * family))
        pw = 1.0 / np.arange(1, len(members) + 1) ** skew
        c = int(rng.integers(1, min(k, len(members)) + 1))
        pick = rng.choice(members, size=c, replace=False, p=pw / pw.sum())
        top = rng.uniform(0.3, 0.9)
        sc = np.sort(top * rng.uniform(ratio - 0.06, 1.0, size=c))[::-1]
        count[r] = c
        target[r, :c] = pick
        score[r, :c] = sc
    return {"count": count, "target": target, "score": score}
