"""The contract of `align_pairs_scored` and `align_cigars_scored` (include/rattle_hip.h) in plain Python, twice, on top of
tests/align_ref.py and tests/cigar_ref.py, and the cases aimed at the three-state kernels.

Gotoh's local alignment with a scoring (m, x, o, e) of four positive magnitudes: match +m, mismatch -x, the first gapped column of a gap
-o, every further one -e (spoa's convention: 8,6 is `correct`'s engine, 8,8 is linear); 1 <= m, x <= 64, 1 <= e <= o <= 64.  With i over
the read (reverse-complemented first on strand 1), j over the transcript, letters A, C, G, T = U:

  U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)     a read base against a gap        U[0][*] = -inf
  L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)     a transcript base against a gap  L[*][0] = -inf
  H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])                    H[0][*] = H[*][0] = 0

A cell with H == 0 begins a new alignment.  In H ties go diagonal, then U, then L; in U and in L open wins a tie with extend; the end cell
is the largest H, ties to the smallest i, then the smallest j.

Fact 1.  H >= U and H >= L on every cell (H is the maximum of a set that holds both).  A gap state on a path is positive: the gap ends
in a cell whose positive H equals its gap state, and every step back along the gap adds e or o.  So every cell a path visits in a gap
state has H >= U > 0 (H >= L > 0): no path runs through a cell whose H is 0, in any state, and since a gap state is entered only from
an H and left only into an H it equals, the first and the last column of every alignment are diagonal.

Fact 2.  With o == e, U[i][j] = max(H[i-1][j], U[i-1][j]) - o = H[i-1][j] - o by fact 1, open wins every tie, and so the path is cell
for cell the linear path of align_ref with gap -o.

  fill(q, t, sc)        the three matrices
  walk(q, t, F, i, j)   from the end cell back: the cells of the path (end first) and the (cell, state) pairs it visits
  traceback(q, t, sc)   the classic form: fill, end cell, walk, count the columns
  forward(q, t, sc)     what the kernel does: every state of every cell carries (start_i, start_j, matches, mismatches) of the path the
                        rule picks for it; a gap step copies the payload of the state it comes from, a diagonal step out of a zero
                        cell starts at the cell's own coordinates; q_gap = sq - M - X, t_gap = st - M - X from the two spans
  full / rectangle      record and ops from the whole matrices / from the rectangle of the record alone (cigar_ref's pair of forms)

No device, no numpy in the recurrences."""
import numpy as np

import align_ref as R
import cigar_ref as CG

NEG = -(1 << 30)
LINEAR, ENGINE, MM2, LONG = (5, 4, 8, 8), (5, 4, 8, 6), (2, 4, 4, 2), (5, 4, 12, 1)
SCORINGS = (LINEAR, ENGINE, MM2, LONG)
H_, U_, L_ = 0, 1, 2                                # the states of a walk


def check_scoring(sc):
    m, x, o, e = sc
    assert 1 <= m <= 64 and 1 <= x <= 64 and 1 <= e <= o <= 64, sc


def fill(q: bytes, t: bytes, sc):
    """(H, U, L), each (len(q) + 1) x (len(t) + 1) as a list of rows; U and L hold NEG where the recurrence has minus infinity (and on
    the borders, which no recurrence reads but through H)"""
    check_scoring(sc)
    m, x, o, e = sc
    q, t = q.translate(R._T), t.translate(R._T)
    n = len(t)
    pH, pU = [0] * (n + 1), [NEG] * (n + 1)
    H, U, L = [pH], [pU], [[NEG] * (n + 1)]
    for qc in q:
        cH, cU, cL = [0] * (n + 1), [NEG] * (n + 1), [NEG] * (n + 1)
        h, l = 0, NEG
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
            if h < 0:
                h = 0
            cH[j], cU[j], cL[j] = h, u, l
        H.append(cH); U.append(cU); L.append(cL)
        pH, pU = cH, cU
    return H, U, L


def walk(q: bytes, t: bytes, F, i: int, j: int, sc, open_wins: bool = True):
    """From H of cell (i, j) back to the zero cell its alignment begins behind.  Returns (cells, end first; visits [(i, j, state)], end
    first).  In H: diagonal if it reproduces the score, else U, else L (a switch of state does not move); in U the step goes up and lands
    in H if open >= extend reproduces U (open_wins=False: if open > extend -- the opposite tie rule, for the test of the rule), else
    stays in U; L likewise to the left."""
    m, x, o, e = sc
    H, U, L = F
    q, t = q.translate(R._T), t.translate(R._T)
    path, visits, state = [(i, j)], [], H_
    while i > 0 and j > 0:
        visits.append((i, j, state))
        if state == H_:
            h = H[i][j]
            if h == 0:
                break
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
        if opn > ext or (opn == ext and open_wins):
            state = H_
        i, j = i - di, j - dj
        path.append((i, j))
    return path, visits


def _record(q, t, F, sc):
    """(record, ops, visits) from filled matrices"""
    m, x, o, e = sc
    score, i, j = R.end_cell(F[0])
    if score <= 0:
        return R.NONE, [], []
    path, visits = walk(q, t, F, i, j, sc)
    ops = CG.ops_of_path(q, t, path)
    n = CG.sums(ops)
    si, sj = path[-1]
    opens = sum(1 for o_, _ in ops if o_ in "ID")
    assert F[0][si][sj] == 0 and score == m * n["="] - x * n["X"] - o * opens - e * (n["I"] + n["D"] - opens)
    return (0, score, si, i, sj, j, n["="], n["X"], n["I"], n["D"]), ops, visits


def full(q: bytes, t: bytes, sc):
    """the whole matrices: (record, ops); (align_ref.NONE, []) if nothing aligns"""
    if not q or not t:
        return R.NONE, []
    return _record(q, t, fill(q, t, sc), sc)[:2]


def traceback(q: bytes, t: bytes, sc):
    return full(q, t, sc)[0]


def forward(q: bytes, t: bytes, sc):
    """the forward-carried payload: no matrix, no walk.  A payload is (start_i, start_j, matches, mismatches)."""
    check_scoring(sc)
    if not q or not t:
        return R.NONE
    m, x, o, e = sc
    q, t = q.translate(R._T), t.translate(R._T)
    n = len(t)
    Z = (0, 0, 0, 0)
    pH, pU, pHp, pUp = [0] * (n + 1), [NEG] * (n + 1), [Z] * (n + 1), [Z] * (n + 1)
    best = (0, 0, 0, Z)                             # score, i, j, payload
    for i, qc in enumerate(q, 1):
        cH, cU, cHp, cUp = [0] * (n + 1), [NEG] * (n + 1), [Z] * (n + 1), [Z] * (n + 1)
        l, lp = NEG, Z
        for j in range(1, n + 1):
            eq = qc == t[j - 1]
            a, b = pH[j] - o, pU[j] - e
            u, up = (a, pHp[j]) if a >= b else (b, pUp[j])
            a, b = cH[j - 1] - o, l - e
            l, lp = (a, cHp[j - 1]) if a >= b else (b, lp)
            d = pH[j - 1] + (m if eq else -x)
            h = max(0, d, u, l)
            cU[j], cUp[j] = u, up
            if h == 0:
                continue                            # begins a new alignment: whatever continues from here takes its own coordinates
            if d >= u and d >= l:
                si, sj, M, X = (i - 1, j - 1, 0, 0) if pH[j - 1] == 0 else pHp[j - 1]
                hp = (si, sj, M + eq, X + (not eq))
            elif u >= l:
                hp = up
            else:
                hp = lp
            cH[j], cHp[j] = h, hp
            if h > best[0]:
                best = (h, i, j, hp)
        pH, pU, pHp, pUp = cH, cU, cHp, cUp
    S, i, j, (si, sj, M, X) = best
    if S <= 0:
        return R.NONE
    sq, st = i - si, j - sj
    assert sq - M - X >= 0 and st - M - X >= 0
    return (0, S, si, i, sj, j, M, X, sq - M - X, st - M - X)


def rectangle(q: bytes, t: bytes, rec, sc, left=0):
    """The recurrence over the rectangle of `rec` alone (H' = 0, U' = L' = -inf on its borders), walked back from its last cell.  left:
    columns the rectangle is cut short by on the left (the test of the test).  Returns (ops, H' of the last cell, end of the walk,
    the three matrices)."""
    _, _, si, i, sj, j = rec[:6]
    qq, tt = q[si:i], t[sj + left:j]
    F = fill(qq, tt, sc)
    path, _ = walk(qq, tt, F, len(qq), len(tt), sc)
    return CG.ops_of_path(qq, tt, path), F[0][len(qq)][len(tt)], path[-1], F


_memo = {}


def pair(q: bytes, t: bytes, rev: int, sc, form="full"):
    """(record on the read as given, ops) of one pair: the strand applied as align_ref.align applies it.  form "forward" has no ops."""
    key = (q, t, int(rev), tuple(sc), form)
    if key not in _memo:
        qq = R.revcomp(q) if rev else q
        rec, ops = full(qq, t, sc) if form == "full" else (forward(qq, t, sc), None)
        if rev and rec[0] == 0:
            rec = rec[:2] + (len(q) - rec[3], len(q) - rec[2]) + rec[4:]
        _memo[key] = (rec, ops)
    return _memo[key]


def records(targets, reads, target_of_read, rev, sc, max_cells=0, form="full"):
    """what rattle_hip_align_pairs_scored returns: a dict of arrays (align_ref.FIELDS).  Pairs are remembered per scoring."""
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
    """the CIGAR string of every read, b"" for a read that is not submitted, skipped or aligns nothing"""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0 or not q or not targets[x] or (max_cells and len(q) * len(targets[x]) > max_cells):
            out.append(b"")
        else:
            out.append(CG.text(pair(q, targets[x], int(s), sc)[1]))
    return out


# ---- cases for the three-state kernels: (targets, reads, target_of_read, rev) --------------------------------------------------------
def exon_pair(seed=5, flank=60, insert=40):
    """the pair of the README: two random flanks, a random insert in the transcript only"""
    rng = np.random.default_rng(seed)
    f1, x, f2 = R.rnd(rng, flank), R.rnd(rng, insert), R.rnd(rng, flank)
    return f1 + f2, f1 + x + f2


def gap_case(seed=31):
    """Exons that one sequence lacks, between 60-base flanks: a 40- and a 70-base insert in the read (one I run) and in the transcript
    (one D run).  Read side, rows counted from 0: the 70-base run behind a front flank cut to 50 bases lies in rows 50 - 119, the
    40-base run in rows 60 - 99 and a 10-base run in rows 60 - 69, so each crosses the block edge at row 64 in U, through the strip.
    (A 70-base gap costs 8 + 69 * 6 = 422 under 8,6, more than a 60-base flank earns, so only 12,1 spans it; 40 bases cost 242.)
    Then the four long-gap pairs again with 70 random bases in front of both sequences, so that the rectangle does not begin at 0:
    kernel F's blocks, counted from the rectangle's first row, are then not kernel E's."""
    rng = np.random.default_rng(seed)
    pairs = []
    f = [R.rnd(rng, 60) for _ in range(4)]
    x40, x70, x10 = R.rnd(rng, 40), R.rnd(rng, 70), R.rnd(rng, 10)
    pairs.append((f[0][10:] + x70 + f[1], f[0][10:] + f[1], 0))          # [0] I run in rows 50 - 119
    pairs.append((f[2] + x10 + f[3], f[2] + f[3], 0))                    # [1] I run in rows 60 - 69
    pairs.append((f[0] + x40 + f[1], f[0] + f[1], 0))                    # [2] I run in rows 60 - 99
    pairs.append((f[0] + f[1], f[0] + x40 + f[1], 0))                    # [3], [4] D runs of 40 and 70
    pairs.append((f[2] + f[3], f[2] + x70 + f[3], 0))
    for q, t, _ in list(pairs[:1]) + list(pairs[2:5]):
        pairs.append((R.rnd(rng, 70) + q, R.rnd(rng, 70) + t, 0))
    return R.pairs_case(pairs)


def block_edge_case(seed=32):
    """A gap that ends in row 64 exactly (its last I row is the last row of block 0, DP row 64), one that begins there (its first I row
    is DP row 65, lane 0 of block 1 -- its open comes through the strip), a 130-column D run across two refills, and a 150-row I run
    that crosses two block edges in U."""
    rng = np.random.default_rng(seed)
    a, b, c = R.rnd(rng, 60), R.rnd(rng, 64), R.rnd(rng, 70)
    g4, g12, g130, g150 = R.rnd(rng, 4), R.rnd(rng, 12), R.rnd(rng, 130), R.rnd(rng, 150)
    return R.pairs_case([(a + g4 + c, a + c, 0),            # I rows (1-based) 61 - 64
                         (b + g12 + c, b + c, 0),           # I rows 65 - 76
                         (a + c, a + g130 + c, 0),          # D columns 61 - 190
                         (a[:40] + g150 + c, a[:40] + c, 0)])      # I rows 41 - 190: blocks 0, 1 and 2


def homopolymer_case():
    """homopolymers and repeats of unequal length: under o = 2 e (8,4; 4,2) a gap of two columns ties with two gaps of one"""
    rng = np.random.default_rng(33)
    a, b = R.rnd(rng, 30), R.rnd(rng, 30)
    return R.pairs_case([(b"A" * 40, b"A" * 47, 0), (b"A" * 47, b"A" * 40, 0), (a + b"G" * 7 + b, a + b"G" * 10 + b, 0),
                         (a + b"G" * 10 + b, a + b"G" * 7 + b, 0), (a + b"GA" * 8 + b, a + b"AG" * 10 + b, 0),
                         (b"A" * 70 + a, b"A" * 66 + a, 0)])


CASES = {"gaps": gap_case, "block_edges": block_edge_case, "homopolymers": homopolymer_case}
EDGE_CASES = ("gaps", "block_edges", "homopolymers", "ties", "zero_crossing", "status")      # run under every scoring; the others under two


def all_cases():
    """name -> builder: align_ref's, cigar_ref's and the ones above"""
    return {**R.CASES, **CG.CASES, **CASES}
