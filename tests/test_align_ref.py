"""The contract of `align_pairs` as tests/align_ref.py states it, without a device: the classic fill + traceback and the forward-carried
payload agree on every built case, the identity for `mismatches` divides exactly, and each constructed case sits on the edge it is
named after -- the tie cases have a tied cell ON the optimal path, the zero-crossing case an interior zero a traceback without the zero
rule would walk through, the two-ends cases at least two cells with the best score."""
import numpy as np
import pytest

import align_ref as R

MAX_CELLS = 2_000_000          # what one test may hand a Python reference


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_two_forms_agree(name):
    case = R.CASES[name]()
    assert R.cells(case) <= MAX_CELLS
    a, b = R.records(*case), R.records(*case, form=R.forward)         # (forward() asserts that the division is exact and >= 0)
    assert not R.same(b, a), R.same(b, a)[:8]
    ok = a["status"] == 0
    sq, st = (a["q_end"] - a["q_start"]).astype(np.int64), (a["t_end"] - a["t_start"]).astype(np.int64)
    M, X, S = a["matches"].astype(np.int64), a["mismatches"].astype(np.int64), a["score"].astype(np.int64)
    assert (12 * X == 8 * (sq + st) - 21 * M + S)[ok].all()
    assert (S == 5 * M - 4 * X - 8 * (a["q_gap"].astype(np.int64) + a["t_gap"]))[ok].all()
    assert (sq == M + X + a["q_gap"])[ok].all() and (st == M + X + a["t_gap"])[ok].all()
    for f, _ in R.FIELDS[1:]:
        assert not a[f][~ok].any(), f


def tied_cells_on_path(q, t):
    """The cells of the optimal path that a tie rule decides: those where two predecessors reproduce the score (diagonal, up, left
    order), and the end cell if other cells hold the best score too (smallest i, smallest j order)."""
    H = R.fill(q, t)
    score, i, j = R.end_cell(H)
    pred = []
    for a, b in R.walk(q, t, H, i, j):
        if H[a][b] > 0:
            ways = [H[a - 1][b - 1] + (R.MATCH if q[a - 1] == t[b - 1] else R.MISMATCH), H[a - 1][b] + R.GAP, H[a][b - 1] + R.GAP]
            if ways.count(H[a][b]) > 1:
                pred.append((a, b))
    end = [(i, j)] if sum(row.count(score) for row in H) > 1 else []
    return pred, end


def test_the_tie_cases_have_a_tied_cell_on_the_optimal_path():
    """A repeat on a longer copy of itself runs down one diagonal, where no two predecessors can tie (up and left lie 13 below the
    diagonal): its tied cell is the END cell, which every shift of the repeat's period reaches with the same score.  The deleted base
    inside a run ties two PREDECESSORS: the gap can stand at any base of the run."""
    targets, reads, tor, _ = R.tie_cases()
    for k, (q, x) in enumerate(zip(reads, tor)):
        pred, end = tied_cells_on_path(q, targets[x])
        assert (pred if k >= 4 else end), (k, q, targets[x])
    rec = R.records(*R.tie_cases())
    # A*40 on A*47: the first cell of the best score ends it -- the whole read on the transcript's first 40 bases, no gap
    assert [int(rec[f][0]) for f, _ in R.FIELDS] == [0, 200, 0, 40, 0, 40, 40, 0, 0, 0]
    assert [int(rec[f][1]) for f, _ in R.FIELDS] == [0, 200, 0, 40, 0, 40, 40, 0, 0, 0]
    # the deleted base inside the run: one gapped column, on the side that lacks it
    assert (int(rec["q_gap"][4]), int(rec["t_gap"][4])) == (0, 1) and (int(rec["q_gap"][5]), int(rec["t_gap"][5])) == (1, 0)
    assert int(rec["matches"][4]) == 69 and int(rec["score"][4]) == 5 * 69 - 8


def test_the_zero_crossing_case_has_a_zero_on_the_path():
    targets, reads, _, _ = R.zero_crossing_case()
    q, t = reads[0], targets[0]
    H = R.fill(q, t)
    score, i, j = R.end_cell(H)
    stop, on = R.walk(q, t, H, i, j), R.walk(q, t, H, i, j, zero_rule=False)
    si, sj = stop[-1]
    assert si > 0 and sj > 0 and H[si][sj] == 0                       # an interior zero ...
    assert len(on) > len(stop) and on[:len(stop)] == stop             # ... that a walk without the rule goes on through
    assert on[-1] == (0, 0)
    rec = R.records(*R.zero_crossing_case())
    assert [int(rec[f][0]) for f, _ in R.FIELDS] == [0, 300, 9, 69, 9, 69, 60, 0, 0, 0]


def test_the_two_ends_cases_have_two_best_cells():
    targets, reads, tor, _ = R.two_ends_cases()
    rec = R.records(*R.two_ends_cases())
    for k, (q, x) in enumerate(zip(reads, tor)):
        H = R.fill(q, targets[x])
        score, i, j = R.end_cell(H)
        ends = [(a, b) for a, row in enumerate(H) for b, h in enumerate(row) if h == score]
        assert len(ends) >= 2 and (i, j) == min(ends)
        assert (int(rec["q_end"][k]), int(rec["t_end"][k])) == (i, j)
    assert int(rec["t_start"][0]) == 20 and int(rec["t_end"][0]) == 70 and int(rec["q_start"][1]) == 20 and int(rec["q_end"][1]) == 70


def test_the_strand_and_the_statuses():
    assert R.revcomp(b"AACGU") == b"ACGTT"
    targets, reads, tor, rev = R.strand_case()
    rec = R.records(targets, reads, tor, rev)
    # read 0: 70 bases of junk in front on the transcript's strand = behind on the read as given: q_* are mapped, not centred
    lq = len(reads[0])
    assert rec["status"][0] == 0 and rec["q_start"][0] <= 5 + 8 and abs(int(rec["q_end"][0]) - (lq - 70)) <= 8      # (chance matches in the junk)
    assert rec["score"][0] > 4 * rec["score"][1]
    st = R.records(*R.status_case())
    assert list(st["status"]) == [1, 1, 1, 3, 0]
    case = R.status_case()
    assert list(R.records(*case, max_cells=24 * 30 - 1)["status"]) == [1, 1, 1, 3, 2]
    assert list(R.records(*case, max_cells=24 * 30)["status"]) == [1, 1, 1, 3, 0]


def test_the_edge_case_meets_every_edge_with_both_sequences():
    targets, reads, tor, _ = R.edge_case()
    assert {(len(q), len(targets[x])) for q, x in zip(reads, tor)} == {(a, b) for a in R.EDGE_ROWS for b in R.EDGE_COLS}
    rec = R.records(*R.edge_case())
    big = [k for k, (q, x) in enumerate(zip(reads, tor)) if len(q) >= 127 and len(targets[x]) >= 127]
    assert all(rec["q_end"][k] - rec["q_start"][k] > 64 and rec["t_end"][k] - rec["t_start"][k] > 64 for k in big)     # across the edges
