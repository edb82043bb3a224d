"""The read mode's contract (tests/align_ends_ref.py) against itself, on the CPU: on every pair of every case, under the four scorings of
align_affine_ref and 1,64,1,1 -- fill + walk equals the forward-carried payload; the rectangle (0, Lq] x (t_start, t_end] with the mode's
borders gives the same ops, the corner score and a walk that ends in the corner (kernel F's lemma); no op list begins or ends with D; the
op sums are the record's counts and spans; the linear identity is exact.  Then the test of the test (a rectangle one column short loses
the path) and each constructed case on the edge it is named after.  No test hands a reference more than 2e6 cells."""
import pytest

import align_affine_ref as A
import align_ends_ref as E
import align_ref as R
import cigar_ref as CG

ALL = E.all_cases()
RUNS = [(n, sc) for n in sorted(ALL) for sc in E.SCORINGS]


def pairs_of(case):
    targets, reads, tor, rev = case
    return [(R.revcomp(q) if s else q, targets[x], q, s) for q, x, s in zip(reads, tor, rev) if x >= 0 and q and targets[x]]


@pytest.mark.parametrize("name,sc", RUNS, ids=[f"{n}-{'.'.join(map(str, sc))}" for n, sc in RUNS])
def test_walk_payload_rectangle_and_sums_agree(name, sc):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    m, x, o, e = sc
    for k, (qq, t, q, s) in enumerate(pairs_of(case)):
        rec, ops = E.pair(q, t, s, sc)
        assert rec == E.pair(q, t, s, sc, "forward")[0], (name, k)
        status, score, q_start, q_end, t_start, t_end, M, X, qg, tg = rec
        assert (status, q_start, q_end) == (0, 0, len(q)) and 0 <= t_start <= t_end <= len(t) and t_end >= 1
        got, corner, end, _ = E.rectangle(qq, t, rec, sc)
        assert got == ops and corner == score and end == (0, 0), (name, k)
        assert ops and ops[0][0] != "D" and ops[-1][0] != "D", (name, k, ops[:2], ops[-2:])
        n = CG.sums(ops)
        assert (n["="], n["X"], n["I"], n["D"]) == (M, X, qg, tg)
        assert M + X + qg == len(q) and M + X + tg == t_end - t_start
        if tuple(sc) == A.LINEAR:
            assert 12 * X == 8 * (len(q) + t_end - t_start) - 21 * M + score, (name, k)


def case_pair(name, k):
    targets, reads, tor, rev = E.CASES[name]()
    return reads[k], targets[tor[k]], rev[k]


def test_a_rectangle_one_column_short_loses_the_path():
    """overhangs[6]: the transcript's bases 20 - 119 and one more; the rectangle is columns (20, 120], and without column 21 the read's
    first base has no partner"""
    q, t, _ = case_pair("overhangs", 6)
    for sc in (A.LINEAR, A.ENGINE):
        rec, ops = E.full(q, t, sc)
        assert rec[4:6] == (20, 120) and ops == [("=", 100), ("I", 1)]
        short, corner, _, _ = E.rectangle(q, t, rec, sc, left=1)
        assert short != ops and corner < rec[1]


@pytest.mark.parametrize("sc", (A.LINEAR, A.ENGINE), ids=("5.4.8.8", "5.4.8.6"))
def test_the_overhangs_lie_where_the_case_says(sc):
    for k, n in enumerate(E.OVERHANGS):
        # past the start: an I run in rows 1 - n of column 0, then the transcript's first 100 bases
        rec, ops = E.full(*case_pair("overhangs", k)[:2], sc)
        assert ops == [("I", n), ("=", 100)] and rec[4:6] == (0, 100) and rec[1] == 500 + E.border(n, sc)
        # past both ends: the same run in front
        rec, ops = E.full(*case_pair("overhangs", 12 + k)[:2], sc)
        assert ops[0] == ("I", n) and ops[1][0] == "=" and rec[4:6] == (0, 120) and rec[8] == 2 * n
        # past the end: n read bases against a gap, up to the transcript's last column
        rec, ops = E.full(*case_pair("overhangs", 6 + k)[:2], sc)
        assert rec[4:6] == (20, 120) and rec[8] == n and rec[9] == 0
        if sc == A.ENGINE:
            assert sum(l for o, l in ops[1:] if o == "I") == n and ops[0][0] == "=" and ops[0][1] >= 96
    # the 65-base run ends in row 65, lane 0 of the second block; the 70-base one crosses the block edge in the border column
    q, t, _ = case_pair("overhangs", 4)
    path, _ = E.walk(q, t, E.fill(q, t, sc), E.end_cell(E.fill(q, t, sc)[0])[1], sc)
    assert [c for c in path if c[1] == 0] == [(i, 0) for i in range(65, -1, -1)] and (66, 1) in path
    q, t, _ = case_pair("overhangs", 5)
    assert E.full(q, t, sc)[1][0] == ("I", 70) and len(q) == 170


def test_the_foreign_exon_is_clipped_locally_and_on_the_line_in_read_mode():
    targets, reads, tor, rev = E.foreign_exon_case()
    a, x, b = E.foreign_exon_parts()
    assert (len(a), len(x), len(b)) == (40, 40, 120) and targets == [a + b, x + b] and reads == [a + b, a + b]
    rec, ops = CG.full(reads[1], targets[1])                               # local, linear: a clean fragment
    assert rec[:6] == (0, 600, 40, 160, 40, 160) and ops == [("=", 120)]
    assert A.full(reads[1], targets[1], A.ENGINE)[0][:6] == (0, 600, 40, 160, 40, 160)
    own, _ = E.full(reads[0], targets[0], A.LINEAR)
    rec, ops = E.full(reads[1], targets[1], A.LINEAR)
    assert own == (0, 800, 0, 160, 0, 160, 160, 0, 0, 0)
    assert rec == (0, 440, 0, 160, 0, 160, 120, 40, 0, 0) and ops == [("X", 40), ("=", 120)]
    assert own[1] - rec[1] == 40 * (5 + 4)                                 # what the 40 columns cost: 40 matches lost, 40 mismatches paid


def test_the_edge_pairs_sit_on_their_edges():
    targets, reads, tor, rev = E.ends_edge_case()
    assert [(len(q), len(targets[x])) for q, x in zip(reads[:49], tor[:49])] == [(a, b) for a in E.EDGES for b in E.EDGES]
    full = lambda k, sc: E.full(R.revcomp(reads[k]) if rev[k] else reads[k], targets[tor[k]], sc)
    for sc in (A.LINEAR, A.ENGINE):
        assert full(E.E_UNRELATED, sc)[0][1] < 0
        assert full(E.E_ZERO_SCORE, sc) == ((0, 0, 0, 9, 0, 9, 4, 5, 0, 0), [("=", 4), ("X", 5)])
        # the zero in the middle is passed through: the walk visits (9, 9), whose H is 0, and ends in (0, 0)
        q, t = reads[E.E_ZERO_MID], targets[tor[E.E_ZERO_MID]]
        F = E.fill(q, t, sc)
        path, _ = E.walk(q, t, F, E.end_cell(F[0])[1], sc)
        assert F[0][9][9] == 0 and (9, 9) in path and path[-1] == (0, 0)
        assert full(E.E_ZERO_MID, sc) == ((0, 300, 0, 69, 0, 69, 64, 5, 0, 0), [("=", 4), ("X", 5), ("=", 60)])
        assert full(E.E_TIE, sc)[0][:6] == (0, 20, 0, 4, 0, 4)
        assert full(E.E_ONE_ONE, sc)[1] == [("=", 1)] and full(E.E_ONE_ONE_X, sc)[1] == [("X", 1)]
    for k, n in ((E.E_NO_COLUMN, 2), (E.E_NO_COLUMN_LONG, 70), (E.E_ONE_ONE_X, 1), (E.E_UNRELATED, 50)):
        rec, ops = full(k, E.CHEAP_GAP)
        assert rec == (0, -n, 0, n, 1, 1, 0, 0, n, 0) and ops == [("I", n)]       # t_end == t_start: the read is one I run
        assert E.rectangle(reads[k], targets[tor[k]], rec, E.CHEAP_GAP)[:3] == ([("I", n)], -n, (0, 0))
    assert rev[E.E_STRAND] == 1 and b"U" in reads[E.E_STRAND] and b"T" not in reads[E.E_STRAND]
    assert len(reads[E.E_ONE_ROW]) == 1 and len(targets[tor[E.E_ONE_COL]]) == 1
    rec = E.pair(reads[E.E_STRAND], targets[tor[E.E_STRAND]], 1, A.ENGINE)[0]
    assert rec[2:4] == (0, len(reads[E.E_STRAND])) and rec[1] > 200
