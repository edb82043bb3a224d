"""The contract of `align_cigars` in plain Python (tests/cigar_ref.py) against itself, without a device.  On every pair of
align_ref.CASES and of cigar_ref.CASES that aligns: the record cigar_ref derives from its ops is align_ref.records' record, the ops' sums
are the record's counts and spans, and the rectangle lemma holds ("Kernel F") -- the recurrence over the rectangle of the
record alone, walked back from its last cell, gives the ops of the whole matrix, ends in the rectangle's first cell, and its last cell
holds the score.  The new cases are what their builders say they are.  And on one constructed pair a rectangle one column short on the left
loses the path: the lemma's test can fail."""
import pytest

import align_ref as R
import cigar_ref as CR

ALL = {**R.CASES, **CR.CASES}


def aligned_pairs(case):
    targets, reads, tor, rev = case
    return [(q, targets[x], int(s)) for q, x, s in zip(reads, tor, rev) if x >= 0 and q and targets[x]]


@pytest.mark.parametrize("name", sorted(ALL))
def test_sums_spans_and_the_rectangle_lemma(name):
    case = ALL[name]()
    want = R.records(*case)
    strings = CR.cigars(*case)
    n = 0
    for r, (q, x, s) in enumerate(zip(case[1], case[2], case[3])):
        if want["status"][r] != 0:
            assert strings[r] == b""
            continue
        rec, ops = CR.pair(q, case[0][x], int(s))
        assert rec == tuple(int(want[f][r]) for f, _ in R.FIELDS), (name, r)
        assert strings[r] == CR.text(ops) and all(k > 0 for _, k in ops) and all(a[0] != b[0] for a, b in zip(ops, ops[1:]))
        assert ops[0][0] in "=X" and ops[-1][0] == "="                  # a path begins behind a zero on a diagonal step and ends on a match
        n_ops = CR.sums(ops)
        assert (n_ops["="], n_ops["X"], n_ops["I"], n_ops["D"]) == rec[6:10]
        assert n_ops["="] + n_ops["X"] + n_ops["I"] == rec[3] - rec[2] and n_ops["="] + n_ops["X"] + n_ops["D"] == rec[5] - rec[4]
        # the lemma, on the strand that was aligned
        qa = R.revcomp(q) if s else q
        on_strand = rec[:2] + (len(q) - rec[3], len(q) - rec[2]) + rec[4:] if s else rec
        got, corner, end = CR.rectangle(qa, case[0][x], on_strand)
        assert got == ops and corner == rec[1] and end == (0, 0), (name, r)
        n += 1
    assert n == (want["status"] == 0).sum() and n >= 1


def test_the_new_cases_are_what_they_say():
    targets, reads, tor, rev = CR.rect_case()
    want = R.records(targets, reads, tor, rev)
    assert (want["status"] == 0).all() and R.cells((targets, reads, tor, rev)) <= 2_000_000
    rows, cols = want["q_end"] - want["q_start"], want["t_end"] - want["t_start"]
    assert set(CR.EDGES) <= set(rows.tolist()) and set(CR.EDGES) <= set(cols.tolist())
    assert (want["q_start"][:-1] > 0).all() and (want["t_start"][:-1] > 0).all()      # not at the origin (the last pair is)
    assert 70 in want["q_start"].tolist() or want["q_start"].max() > 64               # blocks counted from start_i are not kernel E's
    strings = CR.cigars(targets, reads, tor, rev)
    assert strings[0] == b"1=" and strings[-1] == b"129=" and (rows[0], cols[0]) == (1, 1)
    assert any(b"D" in s for s in strings) and any(b"I" in s for s in strings)

    case = CR.path_case()
    assert R.cells(case) <= 2_000_000
    s = CR.cigars(*case)
    assert b"70D" in s[0] and b"70I" in s[1]
    # an up move out of lane 0: an I on row 64 of the rectangle (which begins at the read's first base)
    rec, ops = CR.pair(case[1][2], case[0][2], 0)
    assert rec[2] == 0
    row, ups = 0, []
    for o, k in ops:
        if o == "I":
            ups += list(range(row, row + k))
        if o != "D":
            row += k
    assert 64 in ups
    assert len(CR.pair(case[1][3], case[0][3], 0)[1]) >= 150                          # a run in almost every column
    assert s[4] == b"65=" and s[5] == b"65=" and s[6] == b"64="                       # homopolymers: the first end cell, diagonal first
    assert case[3][7] == 1 and b"U" in case[1][7] and R.records(*case)["status"][7] == 0


def test_a_rectangle_one_column_short_loses_the_path():
    q = t = b"ACGGTCATTGCAAGCTTGCA"
    rec, ops = CR.full(q, t)
    assert CR.text(ops) == b"20=" and rec[:6] == (0, 100, 0, 20, 0, 20)
    assert CR.rectangle(q, t, rec) == ([("=", 20)], 100, (0, 0))
    got, corner, end = CR.rectangle(q, t, rec, left=1)
    assert got != ops and corner < 100 and end != (0, 0)
