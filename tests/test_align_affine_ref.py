"""The contract of `align_pairs_scored` / `align_cigars_scored` in plain Python (tests/align_affine_ref.py) against itself and against
the linear contract, without a device.  The fill-and-walk form and the forward form agree; H >= U and H >= L; scoring 5,4,8,8 gives
align_ref's records and cigar_ref's ops; the rectangle lemma holds for the three matrices ("Kernels E and F with three
states"); and every constructed case sits on the edge it is named after.  Every existing case runs under 5,4,8,8 and 5,4,8,6, the edge
and the new cases under 2,4,4,2 and 5,4,12,1 as well; no case hands a reference more than 2e6 cells."""
import pytest

import align_affine_ref as A
import align_ref as R
import cigar_ref as CR

ALL = A.all_cases()
RUNS = [(n, sc) for n in sorted(ALL) for sc in A.SCORINGS if sc in (A.LINEAR, A.ENGINE) or n in A.EDGE_CASES]


def submitted(case):
    targets, reads, tor, rev = case
    return [(r, q, targets[x], int(s)) for r, (q, x, s) in enumerate(zip(reads, tor, rev)) if x >= 0 and q and targets[x]]


def gap_runs(rec, ops, letter):
    """[(first, last)] of every run of `letter`: rows of the aligned strand for I, columns for D, counted from 0"""
    row, col, out = rec[2], rec[4], []
    for o, k in ops:
        if o == letter:
            out.append((row, row + k - 1) if letter == "I" else (col, col + k - 1))
        row += k if o != "D" else 0
        col += k if o != "I" else 0
    return out


@pytest.mark.parametrize("name,sc", RUNS, ids=[f"{n}-{'.'.join(map(str, sc))}" for n, sc in RUNS])
def test_the_two_forms_the_sums_and_the_rectangle_lemma(name, sc):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    want = A.records(*case, sc)
    bad = R.same(A.records(*case, sc, form="forward"), want)
    assert not bad, bad[:8]
    strings = A.cigars(*case, sc)
    n = 0
    for r, q, t, s in submitted(case):
        if want["status"][r] != 0:
            assert strings[r] == b""
            continue
        rec, ops = A.pair(q, t, s, sc)
        assert rec == tuple(int(want[f][r]) for f, _ in R.FIELDS)
        assert all(k > 0 for _, k in ops) and all(a[0] != b[0] for a, b in zip(ops, ops[1:]))
        assert ops[0][0] in "=X" and ops[-1][0] == "="                  # fact 1: the first and the last column are diagonal
        n_ops = CR.sums(ops)
        assert (n_ops["="], n_ops["X"], n_ops["I"], n_ops["D"]) == rec[6:10]
        assert n_ops["="] + n_ops["X"] + n_ops["I"] == rec[3] - rec[2] and n_ops["="] + n_ops["X"] + n_ops["D"] == rec[5] - rec[4]
        # the lemma, on the strand that was aligned
        qa = R.revcomp(q) if s else q
        on_strand = rec[:2] + (len(q) - rec[3], len(q) - rec[2]) + rec[4:] if s else rec
        got, corner, end, _ = A.rectangle(qa, t, on_strand, sc)
        assert got == ops and corner == rec[1] and end == (0, 0), (name, r)
        n += 1
    assert n == (want["status"] == 0).sum() and (n >= 1 or name == "status")


@pytest.mark.parametrize("name", sorted({**R.CASES, **CR.CASES}))
def test_5_4_8_8_is_the_linear_contract(name):
    """fact 2, on every existing case: the records of align_ref.traceback and the ops of cigar_ref"""
    case = ALL[name]()
    assert not R.same(A.records(*case, A.LINEAR), R.records(*case))
    assert A.cigars(*case, A.LINEAR) == CR.cigars(*case)


def test_h_is_at_least_u_and_l_on_whole_matrices():
    """fact 1 on the random case, and the rectangle's matrices nowhere above the full ones (the lemma's first step)"""
    case = R.random_case()
    for sc in (A.ENGINE, A.LONG):
        for r, q, t, s in submitted(case)[:20]:
            qa = R.revcomp(q) if s else q
            H, U, L = A.fill(qa, t, sc)
            assert all(h >= u and h >= l for hr, ur, lr in zip(H[1:], U[1:], L[1:]) for h, u, l in zip(hr[1:], ur[1:], lr[1:]))
            rec = A.full(qa, t, sc)[0]
            if rec[0] != 0:
                continue
            _, _, si, _, sj, _ = rec[:6]
            F = A.rectangle(qa, t, rec, sc)[3]
            for M2, M in zip(F, (H, U, L)):
                assert all(a <= b for i, row in enumerate(M2[1:], 1) for a, b in zip(row[1:], M[si + i][sj + 1:]))


def test_a_rectangle_one_column_short_loses_the_path():
    q, t = A.exon_pair()
    rec, ops = A.full(q, t, A.ENGINE)
    assert CR.text(ops) == b"60=40D60=" and rec[:6] == (0, 358, 0, 120, 0, 160)
    assert A.rectangle(q, t, rec, A.ENGINE)[:3] == ([("=", 60), ("D", 40), ("=", 60)], 358, (0, 0))
    got, corner, end, _ = A.rectangle(q, t, rec, A.ENGINE, left=1)
    assert got != ops and corner < 358 and end != (0, 0)


def test_the_pair_of_the_readme():
    """one alignment with one 40-base D run under 8,6 and under 8,1; the linear rule breaks it (score 323, 13 scattered gap columns)"""
    q, t = A.exon_pair()
    assert R.traceback(q, t) == A.traceback(q, t, A.LINEAR) and R.traceback(q, t)[1] == 323
    lin = CR.sums(A.full(q, t, A.LINEAR)[1])
    assert (lin["="], lin["X"], lin["I"] + lin["D"]) == (99, 17, 13)
    for sc in (A.ENGINE, (5, 4, 8, 1), A.MM2, A.LONG):
        assert CR.text(A.full(q, t, sc)[1]) == b"60=40D60="


def test_the_long_gaps_are_spanned_with_affine_gaps_only():
    """gap_case: pairs 0 - 4 at the origin, 5 - 8 = pairs 0, 2, 3, 4 behind 70 random bases.  A 40-base gap costs 320 under 8,8 (a 60-base
    flank earns 300: not spanned), 8 + 39 * 6 = 242 under 8,6 and 12 + 39 = 51 under 12,1 (spanned); a 70-base gap costs 422 under 8,6,
    which no 60-base flank pays for, and 81 under 12,1.  The read-side runs lie in the rows their builder names."""
    case = A.gap_case()
    assert R.cells(case) <= 2_000_000
    longest = {}
    for sc in (A.LINEAR, A.ENGINE, A.LONG):
        for r, q, t, s in submitted(case):
            rec, ops = A.pair(q, t, s, sc)
            longest[sc, r] = max([k for o, k in ops if o in "ID"] + [0])
    assert all(longest[A.LINEAR, r] < 10 for r in range(9))
    assert [longest[A.ENGINE, r] for r in (1, 2, 3, 6, 7)] == [10, 40, 40, 40, 40] and all(longest[A.ENGINE, r] < 10 for r in (0, 4, 5, 8))
    assert [longest[A.LONG, r] for r in range(9)] == [70, 10, 40, 40, 70, 70, 40, 40, 70]
    runs = [gap_runs(*A.pair(case[1][r], case[0][r], 0, A.LONG), "I") for r in range(3)]
    assert runs == [[(50, 119)], [(60, 69)], [(60, 99)]]                  # each crosses row 64, the block edge, in U
    for r in (6, 7):                                                     # behind the junk the rectangle does not begin at 0
        rec, ops = A.pair(case[1][r], case[0][r], 0, A.ENGINE)
        assert rec[2] > 0 and rec[4] > 0 and rec[2] % 64 != 0


def test_the_block_edge_case_sits_on_its_edges():
    case = A.block_edge_case()
    recs = [A.pair(case[1][r], case[0][r], 0, A.LONG) for r in range(4)]
    assert [CR.text(ops) for _, ops in recs] == [b"60=4I70=", b"64=12I70=", b"59=130D71=", b"39=150I71="]
    assert gap_runs(*recs[0], "I") == [(60, 63)]                          # ends in DP row 64, the last row of block 0
    assert gap_runs(*recs[1], "I") == [(64, 75)]                          # begins in DP row 65: lane 0 of block 1 opens from the strip
    assert gap_runs(*recs[2], "D") == [(59, 188)]                         # columns: across the refills at 64 and 128
    assert gap_runs(*recs[3], "I") == [(39, 188)]                         # rows: across the block edges at 64 and 128
    for sc in (A.ENGINE, A.MM2):
        assert [CR.text(A.pair(case[1][r], case[0][r], 0, sc)[1]) for r in range(2)] == [b"60=4I70=", b"64=12I70="]


def path_cells(case, sc):
    """(open / extend ties on path cells, path cells passed in a gap state whose H is larger than that state, pairs whose CIGAR the
    opposite tie rule changes)"""
    m, x, o, e = sc
    ties = above = differ = 0
    for r, q, t, s in submitted(case):
        qa = R.revcomp(q) if s else q
        F = A.fill(qa, t, sc)
        score, i, j = R.end_cell(F[0])
        if score <= 0:
            continue
        path, visits = A.walk(qa, t, F, i, j, sc)
        for a, b, state in visits:
            if state == A.H_:
                continue
            M, di, dj = (F[1], 1, 0) if state == A.U_ else (F[2], 0, 1)
            ties += F[0][a - di][b - dj] - o == M[a - di][b - dj] - e
            above += F[0][a][b] > M[a][b]
        other, _ = A.walk(qa, t, F, i, j, sc, open_wins=False)
        differ += CR.ops_of_path(qa, t, other) != CR.ops_of_path(qa, t, path)
    return ties, above, differ


def test_open_extend_ties_and_gap_states_below_h_lie_on_paths():
    """the tie rule decides a CIGAR (homopolymers under o = 2 e; the random case under 8,6), and a path passes in a gap state through
    cells whose H is larger than that state -- the walk must follow the state, not H"""
    ties, above, differ = path_cells(A.homopolymer_case(), A.MM2)
    assert ties >= 1 and differ >= 1
    ties, above, differ = path_cells(R.random_case(), A.ENGINE)
    assert ties >= 1 and above >= 1 and differ >= 1
    assert path_cells(A.gap_case(), A.LONG)[1] >= 1
    assert path_cells(A.gap_case(), A.LINEAR)[1] == 0                     # o == e: open always wins, a gap state is left after one step


def test_the_scoring_limits():
    for bad in ((0, 4, 8, 6), (65, 4, 8, 6), (5, 0, 8, 6), (5, 65, 8, 6), (5, 4, 65, 6), (5, 4, 8, 0), (5, 4, 6, 8)):
        with pytest.raises(AssertionError):
            A.fill(b"ACGT", b"ACGT", bad)
    for ok in ((1, 1, 1, 1), (64, 64, 64, 64), (64, 1, 64, 1)):
        A.check_scoring(ok)
    assert A.traceback(b"ACGT" * 8, b"ACGT" * 8, (64, 64, 64, 64)) == A.forward(b"ACGT" * 8, b"ACGT" * 8, (64, 64, 64, 64)) == (0, 2048, 0, 32, 0, 32, 32, 0, 0, 0)
