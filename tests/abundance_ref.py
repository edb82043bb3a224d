"""The abundance rule (include/rattle_hip.h, "abundance"; DESIGN.md "abundance") twice: `scalar`, plain Python ints and floats read after
read, and `vector`, numpy on uint64 with np.add.at.  Integer fixed point: an abundance is a whole number of units of 2^-32 read, every
read hands out exactly ONE = 2^32 units per iteration, so sums are exact in any order and the two forms -- and the device -- agree bit
for bit.  Both return the dict Context.abundance returns.

Behind them the candidate lists the tests are made of: `lists`, the family draw, and the lists aimed at the device code's own edges
(csrc/abundance.hip), each with a `*_holds` function that says, from the list alone, whether it holds the work it is named for:

  scan_rounds_case     n_targets + 1 histogram entries across the 1024-entry rounds of the scan, slot-0 targets on both sides of every
                       round edge, with and without the reads of the last bin (no candidate), one index of an edge left unnamed
  leftover_case        one wavefront on target 0 whose slot 1 names 9 (8) distinct targets: one more than (as many as) em_add_matched sums
  spread_case          256 reads on target 0, k = 8, no later-slot target named by more than 7 of them: more than 8 distinct targets in
                       every later slot of any 64 of them; optionally every fifth read alone on target 0
  empty_wavefront_case, run_to_the_edge_case   whole wavefronts of reads without a candidate, behind a mixed wavefront or behind a run
                       that ends on lane 63
  odd_lists, odd_hand  what no assignment makes and the ABI accepts: a target twice in a read, an incompatible slot in front of a
                       compatible one, a negative best score; count, target and score drawn independently
  beyond_2_53_case     2^21 + 5000 reads on target 0: its abundance and the sums of em_shares pass 2^53, where uint64 -> double rounds"""
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


# ---- lists aimed at the edges of csrc/abundance.hip ---------------------------------------------------------------------------------
SCAN = 1024                                  # entries per round of em_scan_kernel
WAVE = 64
SUMMED = 8                                   # EM_ROUNDS: the distinct targets em_add_matched sums per slot of a wavefront


def from_targets(target, score=None):
    """the list of an [n, k] array of targets, -1 behind the last slot a read uses; every score 0.5 unless given"""
    target = np.asarray(target, np.int32)
    used = target >= 0
    count = used.sum(1).astype(np.uint32)
    assert (used == (np.arange(target.shape[1])[None, :] < count[:, None])).all()
    score = np.full(target.shape, 0.5) if score is None else np.asarray(score, np.float64)
    return {"count": count, "target": target, "score": np.where(used, score, -1.0)}


def slot0(cands):
    """the slot-0 target of every read with a candidate: what the device sorts the reads by"""
    return np.asarray(cands["target"])[np.asarray(cands["count"]) > 0, 0]


SCAN_NT = (1023, 1024, 1025, 2047, 2048, 2049, 3077)
SCAN_UNNAMED = ((1025, 1023), (2049, 1024))   # (n_targets, the index nobody names): the last entry of round 0, the first of round 1


def scan_rounds_case(nt, empties, unnamed=None):
    """About 700 reads, k = 4, from `lists` with its targets sent through a fixed permutation of range(nt) (the draw itself names low
    indices), then three reads each forced onto the slot-0 targets at both sides of the scan's round edges and on nt - 1.  empties: a
    tenth of the reads has no candidate (key nt, the last histogram entry).  unnamed: an index no slot of any read names."""
    rng = np.random.default_rng(nt + (7 if empties else 0))
    cands = lists(700, 4, nt, rng, empty=0.1 if empties else 0.0)
    perm = np.random.default_rng(1000 + nt).permutation(nt).astype(np.int32)
    target = cands["target"]
    target[:] = np.where(target >= 0, perm[np.maximum(target, 0)], -1)
    forced = [f for f in sorted({SCAN - 2, SCAN - 1, SCAN, SCAN + 1, 2 * SCAN - 2, 2 * SCAN - 1, 2 * SCAN, 2 * SCAN + 1, nt - 1})
              if f < nt and f != unnamed]
    for i, f in enumerate(np.repeat(forced, 3)):
        r = 5 + 13 * i                                                          # (spread over the reads; 27 at the most)
        cands["count"][r] = 2
        target[r] = (f, (f + 512) % nt, -1, -1)
        cands["score"][r] = (0.8, 0.79, -1.0, -1.0)
    if unnamed is not None:
        for r, j in np.argwhere(target == unnamed):                            # cut the read in front of the name, or move it to nt - 1
            if j >= cands["count"][r]:
                continue
            if j == 0:
                cands["count"][r], target[r], cands["score"][r] = 1, (nt - 1, -1, -1, -1), (0.8, -1.0, -1.0, -1.0)
            else:
                cands["count"][r], target[r, j:], cands["score"][r, j:] = j, -1, -1.0
    return cands


def scan_rounds_holds(cands, nt, empties, unnamed=None):
    """slot-0 targets in every 1024-block of range(nt), on both sides of every round edge there is, on nt - 1; the last bin filled or
    empty as asked; `unnamed` in no slot"""
    t0 = slot0(cands)
    named = np.bincount(t0, minlength=nt) > 0
    edges = [f for f in (SCAN - 2, SCAN - 1, SCAN, SCAN + 1, 2 * SCAN - 1, 2 * SCAN, nt - 1) if f < nt and f != unnamed]
    used = np.arange(4)[None, :] < cands["count"][:, None]
    none = int((cands["count"] == 0).sum())
    return bool(all(named[b:b + SCAN].any() for b in range(0, nt, SCAN)) and named[edges].all() and len(named) == nt
                and (none > 20 if empties else none == 0)
                and (unnamed is None or not (cands["target"][used] == unnamed).any()))


LEFTOVER_NT = 16


def leftover_case(distinct):
    """64 reads with slot 0 = target 0 -- sorted to positions 0 .. 63, the first wavefront -- of which 63 name 1 + i % distinct in slot 1
    and one names nothing; behind them 30 reads on the targets 10 .. 15"""
    rows = [[0, 1 + i % distinct] for i in range(63)] + [[0, -1]] + [[10 + i % 6, 1 + i % 3 if i % 2 else -1] for i in range(30)]
    return from_targets(rows)


def leftover_holds(cands, distinct):
    run = cands["target"][cands["target"][:, 0] == 0]
    s1 = run[:, 1][run[:, 1] >= 0]
    return bool(len(run) == WAVE and len(np.unique(s1)) == distinct and len(s1) == 63 and (slot0(cands) > 0).sum() == 30)


SPREAD_NT = 301


def spread_case(alone_every=0):
    """256 reads on target 0 with k = 8: slot j >= 1 of read i names 1 + (8 i + j) % 300.  alone_every = 5: every fifth read has no
    later slot, so the first lane of a wavefront that still has something to add is seldom lane 0"""
    i = np.arange(256)[:, None]
    j = np.arange(8)[None, :]
    target = np.where(j == 0, 0, 1 + (8 * i + j) % 300)
    if alone_every:
        target[::alone_every, 1:] = -1
    return from_targets(target)


def spread_holds(cands, alone_every=0):
    """One run of exactly four wavefronts, in whatever order the scatter leaves its reads.  Per later slot no target is named by more
    than `most` <= 7 reads; the wavefront with the most reads that have later slots holds at least a quarter of them, `busiest`, and
    so at least busiest / most > 8 distinct targets in every later slot.  With no read alone that is every wavefront."""
    target = cands["target"]
    most = max(int(np.bincount(target[:, j][target[:, j] >= 0]).max()) for j in range(1, 8))
    naming = int((target[:, 1] >= 0).sum())
    busiest = -(-naming // 4)
    return bool((target[:, 0] == 0).all() and len(target) == 4 * WAVE and most <= 7 and -(-busiest // most) > SUMMED
                and (naming == len(target)) == (not alone_every) and ((target[:, 1:] >= 0).all(1) == (target[:, 1] >= 0)).all())


def empty_wavefront_case():
    """300 reads, k = 3, two of every three without a candidate: 100 placed reads on five targets, sorted in front of 200 others"""
    rows = []
    for i in range(300):
        m, t = i // 3, (0, 0, 0, 1, 1, 2, 3, 4)[(i // 3) % 8]
        rows.append([t, (t + 1) % 5 if m % 2 else -1, (t + 2) % 5 if m % 4 == 1 else -1] if i % 3 == 0 else [-1, -1, -1])
    return from_targets(rows), 5


def run_to_the_edge_case():
    """62 reads on target 0 and 130 on target 1, which ends on lane 63 of the third wavefront, then 70 reads without a candidate"""
    rows = [[0, 2]] * 31 + [[-1, -1]] * 70 + [[1, 2 if i % 3 else -1] for i in range(130)] + [[0, -1]] * 31
    return from_targets(rows), 3


def empty_wavefronts(cands):
    """the wavefronts, after the sort by slot 0, that hold no read with a candidate"""
    placed, n = int((cands["count"] > 0).sum()), len(cands["count"])
    return max(0, n // WAVE - -(-placed // WAVE))


ODD_NT, ODD_RATIO = 6, 0.9


def odd_lists(k, seed=9, n=90):
    """count, target and score of every slot drawn independently (the draw of tests/test_abundance_ref.py): read under ODD_RATIO"""
    rng = np.random.default_rng(seed)
    return {"count": rng.integers(0, k + 1, n).astype(np.uint32), "target": rng.integers(0, ODD_NT, (n, k)).astype(np.int32),
            "score": rng.uniform(-0.2, 1.0, (n, k))}


def odd_hand():
    """(2, 2, 2); (1, 3, 1); and a read whose slot 1 is one ulp below the ratio and whose slot 2 is at it.  Under ODD_RATIO the
    compatible reads are ODD_HAND_COMPATIBLE: a read counts once for a target it names three times or twice, and target 4 has none"""
    top = 0.7
    edge = ODD_RATIO * top
    return {"count": np.array([3, 3, 3], np.uint32), "target": np.array([[2, 2, 2], [1, 3, 1], [0, 4, 5]], np.int32),
            "score": np.array([[0.5, 0.5, 0.5], [0.6, 0.6, 0.6], [top, np.nextafter(edge, 0.0), edge]])}


ODD_HAND_COMPATIBLE = [1, 1, 1, 1, 0, 1]


def odd_holds(cands, ratio=ODD_RATIO):
    """what the list has that no assignment makes: (a target twice among a read's compatible slots, an incompatible slot in front of
    a compatible one, a negative best score of a read with a candidate)"""
    ok = compatible(cands, ratio)
    target = np.asarray(cands["target"])
    k = target.shape[1]
    twice = any((ok[:, i] & ok[:, j] & (target[:, i] == target[:, j])).any() for j in range(k) for i in range(j))
    hole = any((~ok[:, j] & ok[:, j + 1]).any() for j in range(1, k - 1))
    negative = bool(((np.asarray(cands["score"])[:, 0] < 0) & (np.asarray(cands["count"]) > 0)).any())
    return bool(twice), bool(hole), negative


BEYOND_N = (1 << 21) + 5000


def beyond_2_53_case(handing_over=0):
    """2^21 + 5000 reads with slot 0 = target 0, the first 3000 of them with target 1 in slot 1 at an equal score: the abundance of
    target 0, and the D of every read, pass 2^53 units.  handing_over: that many more reads (1, 0), which give all but one unit of
    2^32 to target 0 once target 1 has decayed -- target 1 settles at exactly that many units."""
    target = np.full((BEYOND_N + handing_over, 2), -1, np.int32)
    target[:, 0] = 0
    target[:3000, 1] = 1
    target[BEYOND_N:] = (1, 0)
    return from_targets(target)
