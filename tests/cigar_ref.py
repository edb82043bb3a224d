"""The contract of `align_cigars` (include/rattle_hip.h) in plain Python, on top of tests/align_ref.py: the CIGAR of a pair is the path
align_ref.walk returns from align_ref.end_cell of align_ref.fill, read from its start to its end on the strand that was aligned (the read
reverse-complemented first on strand 1, the transcript always forward), in the extended set with runs merged:

  =  a diagonal step with equal letters (U read as T)      X  a diagonal step with unequal letters
  I  an up step: a read base against a gap (q_gap)         D  a left step: a transcript base against a gap (t_gap)

  full(q, t)            record (on the sequences handed over, align_ref.FIELDS order) and ops [(letter, length)] from the whole matrix
  rectangle(q, t, rec)  what kernel F does: the same recurrence over rows (q_start, q_end] x columns (t_start, t_end] alone, walked back
                        from its last cell; returns (ops, score of that cell, the cell the walk ended in)
  cigars(...)           the CIGAR string of every read of a case, b"" where the status is not 0; remembered per pair

and the cases aimed at kernel F's own edges (blocks of 64 rows counted from the rectangle's first row, windows of 64 steps in the walk).
No device, no numpy in the recurrences."""
import numpy as np

import align_ref as R

OP = {"I": 1, "D": 2, "=": 7, "X": 8}          # BAM's numbers


def ops_of_path(q: bytes, t: bytes, path):
    """[(letter, length)] of a path as align_ref.walk returns it (cells, end first), from its start to its end"""
    q, t = q.translate(R._T), t.translate(R._T)
    ops = []
    cells = path[::-1]
    for (c, d), (a, b) in zip(cells, cells[1:]):        # a step from (c, d) to (a, b)
        if a == c + 1 and b == d + 1:
            o = "=" if q[a - 1] == t[b - 1] else "X"
        elif a == c + 1:
            o = "I"
        else:
            o = "D"
        if ops and ops[-1][0] == o:
            ops[-1][1] += 1
        else:
            ops.append([o, 1])
    return [(o, n) for o, n in ops]


def full(q: bytes, t: bytes):
    """the whole matrix: (record, ops); (align_ref.NONE, []) if nothing aligns"""
    if not q or not t:
        return R.NONE, []
    H = R.fill(q, t)
    score, i, j = R.end_cell(H)
    if score <= 0:
        return R.NONE, []
    path = R.walk(q, t, H, i, j)
    ops = ops_of_path(q, t, path)
    n = {o: sum(k for p, k in ops if p == o) for o in OP}
    si, sj = path[-1]
    return (0, score, si, i, sj, j, n["="], n["X"], n["I"], n["D"]), ops


def rectangle(q: bytes, t: bytes, rec, left=0):
    """The recurrence over the rectangle of `rec` alone (zeros on its top row and left column), walked back from its last cell.
    left: columns the rectangle is cut short by on the left (the test of the test).  Returns (ops, H' of the last cell, end of walk)."""
    _, _, si, i, sj, j = rec[:6]
    qq, tt = q[si:i], t[sj + left:j]
    H = R.fill(qq, tt)
    path = R.walk(qq, tt, H, len(qq), len(tt))
    return ops_of_path(qq, tt, path), H[len(qq)][len(tt)], path[-1]


def text(ops) -> bytes:
    return b"".join(b"%d%s" % (n, o.encode()) for o, n in ops)


def encode(ops) -> np.ndarray:
    """the ops as the library returns them: uint32, length << 4 | op"""
    return np.array([n << 4 | OP[o] for o, n in ops], np.uint32)


def sums(ops) -> dict:
    return {o: sum(k for p, k in ops if p == o) for o in OP}


_memo = {}


def pair(q: bytes, t: bytes, rev: int):
    """(record on the read as given, ops) of one pair: the strand applied as align_ref.align applies it"""
    key = (q, t, int(rev))
    if key not in _memo:
        rec, ops = full(R.revcomp(q) if rev else q, t)
        if rev and rec[0] == 0:
            rec = rec[:2] + (len(q) - rec[3], len(q) - rec[2]) + rec[4:]
        _memo[key] = (rec, ops)
    return _memo[key]


def cigars(targets, reads, target_of_read, rev, max_cells=0):
    """the CIGAR string of every read, b"" for a read that is not submitted, skipped or aligns nothing"""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0 or not q or not targets[x] or (max_cells and len(q) * len(targets[x]) > max_cells):
            out.append(b"")
        else:
            out.append(text(pair(q, targets[x], int(s))[1]))
    return out


def split(offsets, ops):
    """what Context.align_cigars returned, as one CIGAR string per read"""
    from rattle_amd import api
    return [api.cigar_bytes(ops[int(a):int(b)]) for a, b in zip(offsets, offsets[1:])]


# ---- cases for kernel F: (targets, reads, target_of_read, rev) ---------------------------------------------------------------------
EDGES = (1, 63, 64, 65, 127, 128, 129)


def _junk(rng, n: int, letters: bytes) -> bytes:
    return bytes(rng.choice(np.frombuffer(letters, np.uint8), n).tobytes())


def rect_case(seed=21):
    """Rectangles of 1, 63, 64, 65, 127, 128, 129 rows and columns that do not start at the matrix origin: 1 - 70 bases in front of the
    read (A and C only) and of the transcript (G and T only, so nothing aligns in front), then a common core; for every edge n the core as
    it is (n x n), with one base more in the transcript (n x n + 1, a D) and with one base more in the read (n + 1 x n, an I).  The blocks
    of kernel F, counted from the rectangle's first row, are not those of kernel E, counted from the read's.  And 129 x 129 at the
    origin."""
    rng = np.random.default_rng(seed)
    pairs = [(b"TTA", b"CCGCA", 0)]                                     # 1 x 1: the read's last base on the transcript's last
    k = 0
    for n in EDGES[1:]:
        core = R.rnd(rng, n)
        more = core[:n // 2] + bytes([b"ACGT"[(b"ACGT".index(core[n // 2]) + 1) % 4]]) + core[n // 2:]
        for q, t in ((core, core), (core, more), (more, core)):
            jq, jt = 1 + (23 * k) % 70, 1 + (37 * k + 11) % 70
            k += 1
            pairs.append((_junk(rng, jq, b"AC") + q, _junk(rng, jt, b"GT") + t + _junk(rng, 5 + k, b"GT"), 0))
    core = R.rnd(rng, 129)
    pairs.append((core, core, 0))
    return R.pairs_case(pairs)


def path_case(seed=22):
    """Paths aimed at the walk: a 70-base D run and a 70-base I run between 150-base exact flanks (a gap run across a window of 64 steps
    and across a block edge); an insertion of 5 read bases over rows 62 - 66 of the rectangle (an up move out of lane 0); match and
    mismatch alternating over 200 bases (a run in almost every column: the ops region's bound); homopolymers of unequal length (ties);
    strand 1, the read written with U, 30 bases of junk in front of a piece of 170."""
    rng = np.random.default_rng(seed)
    f1, f2, x = _junk(rng, 150, b"ACG"), _junk(rng, 150, b"ACG"), b"T" * 70       # (a gap is linear: only a run that matches nothing stays whole)
    a, b, ins = R.rnd(rng, 62), R.rnd(rng, 60), R.rnd(rng, 5)
    alt = R.rnd(rng, 200)
    alt2 = bytes(c if i % 2 == 0 else b"ACGT"[(b"ACGT".index(c) + 1 + i // 2 % 3) % 4] for i, c in enumerate(alt))
    t = R.rnd(rng, 260)
    q = _junk(rng, 30, b"ACGT") + R.mutate(rng, t[50:220], 0.08) + _junk(rng, 9, b"ACGT")
    return R.pairs_case([(f1 + f2, f1 + x + f2, 0), (f1 + x + f2, f1 + f2, 0), (a + ins + b, a + b, 0), (alt, alt2, 0),
                         (b"A" * 65, b"A" * 130, 0), (b"A" * 130, b"A" * 65, 0), (b"A" * 70, b"A" * 64, 0),
                         (R.revcomp(q).replace(b"T", b"U"), t, 1)])


CASES = {"rects": rect_case, "paths": path_case}
