"""The recurrence of kernels E and F once, in plain Python, over a scoring and a mode.  tests/align_affine_ref.py (LOCAL) and
tests/align_ends_ref.py (READ) state each contract in their docstrings and bind the functions below at their mode;
tests/align_sweep.py walks the same matrices under wrong rules.  tests/align_ref.py and cigar_ref.py stay the linear form written
independently, and tests/test_align_model.py holds this module to the answers the two per-mode modules gave when each had its own copy
(tests/golden/align_pairs_ref.json.gz).

Scoring (m, x, o, e), four positive magnitudes; i over the read, j over the transcript:

  U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)        U[0][*] = L[*][0] = -inf, H[0][*] = 0
  L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)
  H[i][j] = max(H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])      ties: diagonal, then U, then L; in U and L open before extend

What the mode decides, and nothing else:

                       LOCAL                                               READ
  H[i][0], U[i][0]     0, -inf                                             -(o + (i-1) e), both
  zero floor in H      yes; a zero cell begins an alignment                none
  end cell             largest H, ties to the smallest i, then j;          largest H[Lq][j] over j >= 1, ties to the smallest j;
                       status 1 if it is not positive                      always status 0
  the walk stops       at H == 0                                           in row 0; in column 0 it goes straight up
  forward payload      a diagonal step out of a zero cell starts at        row 0 starts a path at its own column; start_i is 0
                       the cell                                            everywhere (the kernel carries three words, not four)
  q_* on strand 1      Lq - q_end, Lq - q_start                            the same mapping, which leaves 0, Lq as they are

No device, no numpy in the recurrences."""
import numpy as np

import align_ref as R
import cigar_ref as CG

NEG = -(1 << 30)
LOCAL, READ = "local", "read"
MODES = (LOCAL, READ)
LINEAR = (5, 4, 8, 8)
H_, U_, L_ = 0, 1, 2                                # the states of a walk


def check_scoring(sc):
    m, x, o, e = sc
    assert 1 <= m <= 64 and 1 <= x <= 64 and 1 <= e <= o <= 64, sc


def border(i: int, sc, mode):
    """(H[i][0], U[i][0]), i >= 1"""
    if mode == LOCAL:
        return 0, NEG
    b = -(sc[2] + (i - 1) * sc[3])
    return b, b


def fill(q: bytes, t: bytes, sc, mode):
    """(H, U, L), each (len(q) + 1) x (len(t) + 1) as a list of rows; U and L hold NEG where the recurrence has minus infinity"""
    check_scoring(sc)
    assert mode in MODES
    m, x, o, e = sc
    q, t = q.translate(R._T), t.translate(R._T)
    n = len(t)
    pH, pU = [0] * (n + 1), [NEG] * (n + 1)
    H, U, L = [pH], [pU], [[NEG] * (n + 1)]
    for i, qc in enumerate(q, 1):
        h, u = border(i, sc, mode)
        cH, cU, cL = [h] + [0] * n, [u] + [NEG] * n, [NEG] * (n + 1)
        l = NEG
        for j, tc in enumerate(t, 1):
            a, b = pH[j] - o, pU[j] - e
            u = a if a >= b else b
            a, b = h - o, l - e
            l = a if a >= b else b
            h = pH[j - 1] + (m if qc == tc else -x)
            if u > h:
                h = u
            if l > h:
                h = l
            if h < 0 and mode == LOCAL:
                h = 0
            cH[j], cU[j], cL[j] = h, u, l
        H.append(cH); U.append(cU); L.append(cL)
        pH, pU = cH, cU
    return H, U, L


def end_cell(F, mode):
    """(score, i, j) of the cell the alignment ends in; LOCAL: (0, 0, 0) if no cell is positive"""
    H = F[0]
    if mode == LOCAL:
        return R.end_cell(H)
    row = H[-1]
    best = max(row[1:])
    return best, len(H) - 1, row.index(best, 1)


def walk(q: bytes, t: bytes, F, i: int, j: int, sc, mode, order="dul", open_wins=True):
    """From H of cell (i, j) back to where its alignment begins: LOCAL to the zero cell it begins behind, READ to row 0, straight up in
    column 0 (the border is one gap down from (0, 0)).  Returns (cells, end first; visits [(i, j, state)], end first).  In H the
    predecessors are tried in `order`, a string of d (diagonal), u (the state U) and l (the state L): "dul" is the rule, "udl" and "dlu"
    are wrong ones for the tests of the rule; a switch of state does not move.  In U the step goes up and lands in H if open >= extend
    reproduces U (open_wins=False: if open > extend, the opposite tie rule), else stays in U; L likewise to the left."""
    assert sorted(order) == ["d", "l", "u"]
    m, x, o, e = sc
    H, U, L = F
    q, t = q.translate(R._T), t.translate(R._T)
    path, visits, state = [(i, j)], [], H_
    while i > 0 and (j > 0 or mode == READ):
        if j == 0:
            assert state == H_
            i -= 1
            path.append((i, 0))
            continue
        visits.append((i, j, state))
        if state == H_:
            h = H[i][j]
            if h == 0 and mode == LOCAL:
                break
            for c in order:
                if c == "d" and h == H[i - 1][j - 1] + (m if q[i - 1] == t[j - 1] else -x):
                    i, j = i - 1, j - 1
                    path.append((i, j))
                    break
                if c == "u" and h == U[i][j]:
                    state = U_
                    break
                if c == "l" and h == L[i][j]:
                    state = L_
                    break
            else:
                raise AssertionError("no predecessor reproduces H")
            continue
        M, di, dj = (U, 1, 0) if state == U_ else (L, 0, 1)
        opn, ext = H[i - di][j - dj] - o, M[i - di][j - dj] - e
        assert M[i][j] == max(opn, ext)
        if opn > ext or (opn == ext and open_wins):
            state = H_
        i, j = i - di, j - dj
        path.append((i, j))
    return path, visits


def record(q, t, F, sc, mode):
    """(record, ops, visits) from filled matrices: end cell, walk, count the columns"""
    m, x, o, e = sc
    score, i, j = end_cell(F, mode)
    if mode == LOCAL and score <= 0:
        return R.NONE, [], []
    path, visits = walk(q, t, F, i, j, sc, mode)
    ops = CG.ops_of_path(q, t, path)
    n = CG.sums(ops)
    si, sj = path[-1]
    opens = sum(1 for o_, _ in ops if o_ in "ID")
    assert (F[0][si][sj] == 0) if mode == LOCAL else (si, i) == (0, len(q))
    assert score == m * n["="] - x * n["X"] - o * opens - e * (n["I"] + n["D"] - opens)
    return (0, score, si, i, sj, j, n["="], n["X"], n["I"], n["D"]), ops, visits


def full(q: bytes, t: bytes, sc, mode):
    """the whole matrices: (record, ops); (align_ref.NONE, []) for an empty sequence, and in LOCAL if nothing aligns"""
    if not q or not t:
        return R.NONE, []
    return record(q, t, fill(q, t, sc, mode), sc, mode)[:2]


def forward(q: bytes, t: bytes, sc, mode):
    """What kernel E does: no matrix, no walk.  Every state of every cell carries the payload (start_i, start_j, matches, mismatches) of
    the path the rule picks for it; a gap step copies the payload of the state it comes from; q_gap = sq - M - X, t_gap = st - M - X
    from the two spans."""
    check_scoring(sc)
    assert mode in MODES
    if not q or not t:
        return R.NONE
    local = mode == LOCAL
    m, x, o, e = sc
    q, t = q.translate(R._T), t.translate(R._T)
    n = len(t)
    Z = (0, 0, 0, 0)
    pH, pU, pUp = [0] * (n + 1), [NEG] * (n + 1), [Z] * (n + 1)
    pHp = [Z] * (n + 1) if local else [(0, j, 0, 0) for j in range(n + 1)]
    best = (0, 0, 0, Z)                             # score, i, j, payload
    for i, qc in enumerate(q, 1):
        h, u = border(i, sc, mode)
        cH, cU, cHp, cUp = [h] + [0] * n, [u] + [NEG] * n, [Z] * (n + 1), [Z] * (n + 1)
        l, lp = NEG, Z
        for j in range(1, n + 1):
            eq = qc == t[j - 1]
            a, b = pH[j] - o, pU[j] - e
            u, up = (a, pHp[j]) if a >= b else (b, pUp[j])
            a, b = cH[j - 1] - o, l - e
            l, lp = (a, cHp[j - 1]) if a >= b else (b, lp)
            d = pH[j - 1] + (m if eq else -x)
            h = max(d, u, l)
            cU[j], cUp[j] = u, up
            if local and h <= 0:
                continue                            # begins a new alignment: whatever continues from here takes its own coordinates
            if d >= u and d >= l:
                si, sj, M, X = (i - 1, j - 1, 0, 0) if local and pH[j - 1] == 0 else pHp[j - 1]
                hp = (si, sj, M + eq, X + (not eq))
            elif u >= l:
                hp = up
            else:
                hp = lp
            cH[j], cHp[j] = h, hp
            if local and h > best[0]:
                best = (h, i, j, hp)
        pH, pU, pHp, pUp = cH, cU, cHp, cUp
    if not local:
        S = max(pH[1:])
        j = pH.index(S, 1)
        best = (S, len(q), j, pHp[j])
    S, i, j, (si, sj, M, X) = best
    if local and S <= 0:
        return R.NONE
    sq, st = i - si, j - sj
    if tuple(sc) == LINEAR:                         # what the linear form of kernel E does: X from the score and the two spans
        X12 = 8 * (sq + st) - 21 * M + S
        assert X12 % 12 == 0 and X12 // 12 == X, (X12, X)
    assert sq - M - X >= 0 and st - M - X >= 0
    return (0, S, si, i, sj, j, M, X, sq - M - X, st - M - X)


def rectangle(q: bytes, t: bytes, rec, sc, mode, left=0):
    """What kernel F does: the recurrence over the rectangle of `rec` alone, with the mode's borders, walked back from its last cell
    (READ: the rectangle has every row, and with no column the walk is the border, one I run).  left: columns the rectangle is cut
    short by on the left (the test of the test).  Returns (ops, H' of the last cell, end of the walk, the three matrices)."""
    _, _, si, i, sj, j = rec[:6]
    qq, tt = q[si:i], t[sj + left:j]
    F = fill(qq, tt, sc, mode)
    path, _ = walk(qq, tt, F, len(qq), len(tt), sc, mode)
    return CG.ops_of_path(qq, tt, path), F[0][len(qq)][len(tt)], path[-1], F


_memo = {}


def pair(q: bytes, t: bytes, rev: int, sc, mode, form="full"):
    """(record on the read as given, ops) of one pair: the strand applied as align_ref.align applies it.  form "forward" has no ops."""
    key = (q, t, int(rev), tuple(sc), mode, form)
    if key not in _memo:
        qq = R.revcomp(q) if rev else q
        rec, ops = full(qq, t, sc, mode) if form == "full" else (forward(qq, t, sc, mode), None)
        if rev and rec[0] == 0:
            rec = rec[:2] + (len(q) - rec[3], len(q) - rec[2]) + rec[4:]
        _memo[key] = (rec, ops)
    return _memo[key]


def records(targets, reads, target_of_read, rev, sc, mode, max_cells=0, form="full"):
    """what the library returns for the case: a dict of arrays (align_ref.FIELDS).  Pairs are remembered per scoring and mode."""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0:
            out.append(R.NOT_SUBMITTED)
        elif not q or not targets[x]:
            out.append(R.NONE)
        elif max_cells and len(q) * len(targets[x]) > max_cells:
            out.append(R.SKIPPED)
        else:
            out.append(pair(q, targets[x], int(s), sc, mode, form)[0])
    return {f: np.array([r[k] for r in out], dt) for k, (f, dt) in enumerate(R.FIELDS)}


def cigars(targets, reads, target_of_read, rev, sc, mode, max_cells=0):
    """the CIGAR string of every read, b"" for a read that is not submitted, skipped or aligns nothing"""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0 or not q or not targets[x] or (max_cells and len(q) * len(targets[x]) > max_cells):
            out.append(b"")
        else:
            out.append(CG.text(pair(q, targets[x], int(s), sc, mode)[1]))
    return out


def bind(mode, *names):
    """the named functions with `mode` in its place behind the scoring: what a per-mode module offers under the signatures it always had"""
    def at(f):
        k = f.__code__.co_varnames.index("mode")
        return lambda *a, **kw: f(*a[:k], mode, *a[k:], **kw)
    return [at(globals()[n]) for n in names]
