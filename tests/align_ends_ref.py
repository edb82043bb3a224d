"""The contract of the READ mode of `align_pairs_mode` and `align_cigars_mode` (include/rattle_hip.h, RATTLE_ALIGN_READ) in plain Python,
twice, on top of tests/align_ref.py, tests/cigar_ref.py and tests/align_affine_ref.py, and the cases aimed at what the mode changes in
kernels E and F.

The read is aligned from its first base to its last, the transcript's ends are free (semi-global).  Scoring (m, x, o, e) as in
align_affine_ref; the linear form is 5,4,8,8.  With i over the read (reverse-complemented first on strand 1), j over the transcript:

  H[0][j] = 0 for j = 0..Lt          U[0][*] = -inf        (the alignment may begin at any transcript position)
  H[i][0] = U[i][0] = -(o + (i-1) e) L[*][0] = -inf        (read bases before the transcript's first base: a gap)
  U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)
  L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)
  H[i][j] = max(H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])           -- no zero floor

Ties as in align_affine_ref: in H diagonal, then U, then L; in U and L open wins a tie with extend.  The end cell is the largest
H[Lq][j] over j = 1..Lt, ties to the smallest j.  The walk goes back to row 0 and ends in (0, t_start); row 0 has no left moves, and a
walk that reaches column 0 goes straight up: the remaining rows are one I run.  The record has status 0, q_start = 0, q_end = Lq, a
score that may be zero or negative, and t_end - t_start may be 0 (the whole read one I run).

  fill(q, t, sc)        the three matrices
  walk(q, t, F, j, sc)  from H[Lq][j] back to row 0: the cells of the path (end first) and the (cell, state) pairs it visits
  full(q, t, sc)        fill, end cell, walk, count the columns: (record, ops)
  forward(q, t, sc)     what kernel E does: every state of every cell carries (start_j, matches, mismatches) of its path; row 0 starts
                        a path at its own column, column 0 at column 0
  rectangle(...)        what kernel F does: the same recurrence over columns (t_start, t_end] alone, with this mode's borders

No device, no numpy in the recurrences."""
import numpy as np

import align_affine_ref as A
import align_ref as R
import cigar_ref as CG

NEG = A.NEG
H_, U_, L_ = A.H_, A.U_, A.L_
CHEAP_GAP = (1, 64, 1, 1)                           # a mismatch costs more than any short gap: t_end == t_start occurs
SCORINGS = A.SCORINGS + (CHEAP_GAP,)


def border(i: int, sc) -> int:
    """H[i][0] = U[i][0], i >= 1"""
    return -(sc[2] + (i - 1) * sc[3])


def fill(q: bytes, t: bytes, sc):
    """(H, U, L), each (len(q) + 1) x (len(t) + 1) as a list of rows; NEG where the recurrence has minus infinity"""
    A.check_scoring(sc)
    m, x, o, e = sc
    q, t = q.translate(R._T), t.translate(R._T)
    n = len(t)
    pH, pU = [0] * (n + 1), [NEG] * (n + 1)
    H, U, L = [pH], [pU], [[NEG] * (n + 1)]
    for i, qc in enumerate(q, 1):
        b = border(i, sc)
        cH, cU, cL = [b] + [0] * n, [b] + [NEG] * n, [NEG] * (n + 1)
        h, l = b, NEG
        for j, tc in enumerate(t, 1):
            a, c = pH[j] - o, pU[j] - e
            u = a if a >= c else c
            a, c = h - o, l - e
            l = a if a >= c else c
            h = pH[j - 1] + (m if qc == tc else -x)
            if u > h:
                h = u
            if l > h:
                h = l
            cH[j], cU[j], cL[j] = h, u, l
        H.append(cH); U.append(cU); L.append(cL)
        pH, pU = cH, cU
    return H, U, L


def end_cell(H):
    """(score, j): the largest H of the last row over j >= 1, ties to the smallest j"""
    row = H[-1]
    best = max(row[1:])
    return best, row.index(best, 1)


def walk(q: bytes, t: bytes, F, j: int, sc):
    """From H of cell (Lq, j) back to row 0.  Returns (cells, end first; visits [(i, j, state)], end first).  In column 0 the walk goes
    up (the border is a gap straight down from (0, 0)); elsewhere as align_affine_ref.walk, without its stop at a zero."""
    m, x, o, e = sc
    H, U, L = F
    q, t = q.translate(R._T), t.translate(R._T)
    i = len(q)
    path, visits, state = [(i, j)], [], H_
    while i > 0:
        if j == 0:
            assert state == H_
            i -= 1
            path.append((i, 0))
            continue
        visits.append((i, j, state))
        if state == H_:
            h = H[i][j]
            if h == H[i - 1][j - 1] + (m if q[i - 1] == t[j - 1] else -x):
                i, j = i - 1, j - 1
                path.append((i, j))
            elif h == U[i][j]:
                state = U_
            else:
                assert h == L[i][j]
                state = L_
            continue
        M, di, dj = (U, 1, 0) if state == U_ else (L, 0, 1)
        opn, ext = H[i - di][j - dj] - o, M[i - di][j - dj] - e
        assert M[i][j] == max(opn, ext)
        if opn >= ext:
            state = H_
        i, j = i - di, j - dj
        path.append((i, j))
    return path, visits


def _record(q, t, F, sc):
    m, x, o, e = sc
    score, j = end_cell(F[0])
    path, visits = walk(q, t, F, j, sc)
    ops = CG.ops_of_path(q, t, path)
    n = CG.sums(ops)
    si, sj = path[-1]
    opens = sum(1 for o_, _ in ops if o_ in "ID")
    assert si == 0 and score == m * n["="] - x * n["X"] - o * opens - e * (n["I"] + n["D"] - opens)
    return (0, score, 0, len(q), sj, j, n["="], n["X"], n["I"], n["D"]), ops, visits


def full(q: bytes, t: bytes, sc):
    """the whole matrices: (record, ops); (align_ref.NONE, []) for an empty sequence"""
    if not q or not t:
        return R.NONE, []
    return _record(q, t, fill(q, t, sc), sc)[:2]


def forward(q: bytes, t: bytes, sc):
    """the forward-carried payload: no matrix, no walk.  A payload is (start_j, matches, mismatches); start_i is 0 everywhere."""
    A.check_scoring(sc)
    if not q or not t:
        return R.NONE
    m, x, o, e = sc
    q, t = q.translate(R._T), t.translate(R._T)
    n = len(t)
    Z = (0, 0, 0)
    pH, pU = [0] * (n + 1), [NEG] * (n + 1)
    pHp, pUp = [(j, 0, 0) for j in range(n + 1)], [Z] * (n + 1)
    for i, qc in enumerate(q, 1):
        b = border(i, sc)
        cH, cU, cHp, cUp = [b] + [0] * n, [b] + [NEG] * n, [Z] * (n + 1), [Z] * (n + 1)
        l, lp = NEG, Z
        for j in range(1, n + 1):
            eq = qc == t[j - 1]
            a, c = pH[j] - o, pU[j] - e
            u, up = (a, pHp[j]) if a >= c else (c, pUp[j])
            a, c = cH[j - 1] - o, l - e
            l, lp = (a, cHp[j - 1]) if a >= c else (c, lp)
            d = pH[j - 1] + (m if eq else -x)
            if d >= u and d >= l:
                sj, M, X = pHp[j - 1]
                hp = (sj, M + eq, X + (not eq))
            elif u >= l:
                hp = up
            else:
                hp = lp
            cH[j], cHp[j], cU[j], cUp[j] = max(d, u, l), hp, u, up
        pH, pU, pHp, pUp = cH, cU, cHp, cUp
    S = max(pH[1:])
    j = pH.index(S, 1)
    sj, M, X = pHp[j]
    sq, st = len(q), j - sj
    if tuple(sc) == A.LINEAR:                       # what the linear form of kernel E does: X from the score and the two spans
        X12 = 8 * (sq + st) - 21 * M + S
        assert X12 % 12 == 0 and X12 // 12 == X, (X12, X)
    assert sq - M - X >= 0 and st - M - X >= 0
    return (0, S, 0, sq, sj, j, M, X, sq - M - X, st - M - X)


def rectangle(q: bytes, t: bytes, rec, sc, left=0):
    """The recurrence over the rectangle of `rec` alone -- every row, columns (t_start, t_end] -- with this mode's borders, walked back
    from its last cell.  left: columns the rectangle is cut short by on the left (the test of the test).  Returns (ops, H' of the last
    cell, end of the walk, the three matrices).  With no column the walk is the border: one I run."""
    sj, j = rec[4], rec[5]
    tt = t[sj + left:j]
    F = fill(q, tt, sc)
    path, _ = walk(q, tt, F, len(tt), sc)
    return CG.ops_of_path(q, tt, path), F[0][len(q)][len(tt)], path[-1], F


_memo = {}


def pair(q: bytes, t: bytes, rev: int, sc, form="full"):
    """(record on the read as given, ops) of one pair.  q_start = 0 and q_end = Lq on either strand.  form "forward" has no ops."""
    key = (q, t, int(rev), tuple(sc), form)
    if key not in _memo:
        qq = R.revcomp(q) if rev else q
        _memo[key] = full(qq, t, sc) if form == "full" else (forward(qq, t, sc), None)
    return _memo[key]


def records(targets, reads, target_of_read, rev, sc, max_cells=0, form="full"):
    """what rattle_hip_align_pairs_mode returns in read mode: a dict of arrays (align_ref.FIELDS)"""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0:
            out.append(R.NOT_SUBMITTED)
        elif not q or not targets[x]:
            out.append(R.NONE)
        elif max_cells and len(q) * len(targets[x]) > max_cells:
            out.append(R.SKIPPED)
        else:
            out.append(pair(q, targets[x], int(s), sc, form)[0])
    return {f: np.array([r[k] for r in out], dt) for k, (f, dt) in enumerate(R.FIELDS)}


def cigars(targets, reads, target_of_read, rev, sc, max_cells=0):
    """the CIGAR string of every read, b"" for a read that is not submitted, skipped or has an empty sequence"""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0 or not q or not targets[x] or (max_cells and len(q) * len(targets[x]) > max_cells):
            out.append(b"")
        else:
            out.append(CG.text(pair(q, targets[x], int(s), sc)[1]))
    return out


# ---- cases for the read mode: (targets, reads, target_of_read, rev) -------------------------------------------------------------------
OVERHANGS = (1, 5, 63, 64, 65, 70)


def overhang_case(seed=41):
    """The read runs 1, 5, 63, 64, 65 and 70 bases past the transcript's start (pairs 0 - 5), past its end (6 - 11) and past both
    (12 - 17); the transcript is 120 random bases.  A leading overhang of n bases is an I run in rows 1 - n of column 0, the border: the
    70-base one crosses the block edge at row 64 there, the 65-base one ends in row 65, lane 0 of block 1.  A trailing one is an I run in
    the last n rows, in the transcript's last column."""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, 120)
    pairs = [(R.rnd(rng, n) + t[:100], t, 0) for n in OVERHANGS]
    pairs += [(t[20:] + R.rnd(rng, n), t, 0) for n in OVERHANGS]
    pairs += [(R.rnd(rng, n) + t + R.rnd(rng, n), t, 0) for n in OVERHANGS]
    return R.pairs_case(pairs)


def foreign_exon_parts(seed=42):
    """(A, X, B): two first exons of 40 bases that share no letter (A of A and C, X of G and T), and a common rest of 120"""
    rng = np.random.default_rng(seed)
    return CG._junk(rng, 40, b"AC"), CG._junk(rng, 40, b"GT"), R.rnd(rng, 120)


def foreign_exon_case():
    """The README's example: transcripts A+B and X+B, the read A+B on each.  Locally the read on X+B is 120= with q_start 40; in read mode
    its first 40 bases are on the line, and AS is lower than on A+B by what they cost."""
    a, x, b = foreign_exon_parts()
    return [a + b, x + b], [a + b, a + b], [0, 1], [0, 0]


EDGES = (1, 63, 64, 65, 127, 128, 129)
# the named pairs of ends_edge_case, behind the 49 crossed lengths
E_UNRELATED, E_ZERO_SCORE, E_ZERO_MID, E_TIE, E_NO_COLUMN, E_NO_COLUMN_LONG, E_ONE_ONE, E_ONE_ONE_X, E_ONE_ROW, E_ONE_COL, E_STRAND = range(49, 60)


def ends_edge_case(seed=43):
    """Reads of 1, 63 - 65, 127 - 129 bases against transcripts of the same lengths, crossed, pieces of one ancestor (pairs 0 - 48: every
    block and refill edge of both kernels, with overhangs wherever the read is the longer one); then
      49  unrelated sequences: a negative score
      50  4 matches and 5 mismatches: the score is exactly 0 under 5,4,*,*
      51  the same in front of 60 matches: H == 0 in the middle of the chosen path, passed through
      52  AAAA on A * 10: every end column from 4 on ties, t_end = 4 and t_start = 0
      53  CC on AA: under 1,64,1,1 the read is one I run, t_end == t_start
      54  70 C on 5 A: the same across a block edge
      55 - 58  Lq = 1 and Lt = 1, equal and unequal; one row; one column
      59  strand 1, the read written with U"""
    rng = np.random.default_rng(seed)
    base = R.rnd(rng, 160)
    pairs = []
    for lq in EDGES:
        for lt in EDGES:
            q, t = R.mutate(rng, base, 0.1), R.mutate(rng, base, 0.05)
            pairs.append(((q + R.rnd(rng, lq))[:lq], (t + R.rnd(rng, lt))[:lt], 0))
    tail = R.rnd(rng, 60)
    t = R.rnd(rng, 90)
    q = R.rnd(rng, 7) + R.mutate(rng, t[10:80], 0.08) + R.rnd(rng, 4)
    pairs += [(CG._junk(rng, 50, b"AC"), CG._junk(rng, 60, b"GT"), 0),
              (b"ACGTAAAAA", b"ACGTCCCCC", 0),
              (b"ACGTAAAAA" + tail, b"ACGTCCCCC" + tail, 0),
              (b"AAAA", b"A" * 10, 0),
              (b"CC", b"AA", 0),
              (b"C" * 70, b"A" * 5, 0),
              (b"A", b"A", 0), (b"A", b"C", 0), (b"G", R.rnd(rng, 10), 0), (R.rnd(rng, 10), b"G", 0),
              (R.revcomp(q).replace(b"T", b"U"), t, 1)]
    return R.pairs_case(pairs)


CASES = {"overhangs": overhang_case, "foreign_exon": foreign_exon_case, "ends_edges": ends_edge_case}
EDGE_CASES = A.EDGE_CASES + tuple(CASES)            # run under every scoring; the others under two


def all_cases():
    """name -> builder: those of the three references below, and the ones above"""
    return {**A.all_cases(), **CASES}
