"""The cases of tests/align_sweep.py on the CPU: each sits where it claims, and a wrong rule changes it.  These are conditions on the
INPUTS of tests/test_gpu_pair_sweep.py, measured with the references' own matrices and a walk under a wrong rule -- not measurements of a
kernel; a seed that misses a floor is changed, never the floor.  And under every scoring of SWEEP_SCORINGS the two forms of both
references (fill + walk, and the forward-carried payload) agree on every case the device runs under it, so that what the device is
compared with there is not one implementation's opinion.  No test hands a reference more than 2e6 cells.

Counts, as measured (pairs whose CIGAR the wrong rule changes / those that change beyond DP row 64):
  shifted_tie_case, 108 pairs, 2,4,4,2     extend before open   local 9 / 9     read 9 / 9
                                           H order "udl"        local 27 / 25   read 54 / 52
  edges + random, 109 pairs, H order "dlu" 1,64,1,1 and 2,5,2,2 local 84 / 33   read 83 / 43"""
import pytest

import align_affine_ref as A
import align_ends_ref as E
import align_ref as R
import align_sweep as S
import cigar_ref as CG

ALL = S.all_cases()
STANDARD = (A.LINEAR, A.ENGINE, A.MM2)
FORMS = [(n, sc, mode) for n in S.SWEPT for sc in S.SWEEP_SCORINGS for mode in S.MODES]
FORMS += [("end_order", sc, mode) for sc in STANDARD for mode in S.MODES]
FORMS += [(n, A.ENGINE, mode) for n in ("many_blocks", "many_blocks_t") for mode in S.MODES]


@pytest.mark.parametrize("name,sc,mode", FORMS, ids=[f"{n}-{S.scoring_id(sc)}-{mode}" for n, sc, mode in FORMS])
def test_the_two_forms_agree_under_every_scoring(name, sc, mode):
    """fill + walk == the forward payload, field for field; the ops' sums are the record's counts; and with o == e no walk holds a gap
    state for two steps (fact 2 of align_affine_ref: the path is the linear path with gap o)"""
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    targets, reads, tor, rev = case
    m, x, o, e = sc
    for r, qa, t in S.submitted(case):
        rec, ops, visits, _ = S.full(qa, t, sc, mode)
        assert rec == S.ref(mode).forward(qa, t, sc), (name, r)
        if mode == "read":
            assert rec[0] == 0 and rec[2:4] == (0, len(qa))
        if rec[0] != 0:
            assert mode == "local" and ops == []
            continue
        n = CG.sums(ops)
        assert (n["="], n["X"], n["I"], n["D"]) == rec[6:10]
        opens = sum(1 for c, _ in ops if c in "ID")
        assert rec[1] == m * n["="] - x * n["X"] - o * opens - e * (n["I"] + n["D"] - opens)
        if o == e:
            assert not S.gap_held_two_steps(visits), (name, r)


@pytest.mark.parametrize("mode", S.MODES)
def test_the_walk_with_a_chosen_rule_is_the_references_walk_under_the_rule(mode):
    """the helper itself: order "dul" with open before extend gives the reference's path and visits"""
    for name in ("ties", "homopolymers", "overhangs", "strand", "zero_crossing"):
        for sc in (A.MM2, E.CHEAP_GAP):
            for r, qa, t in S.submitted(ALL[name]()):
                F = S.fill(qa, t, sc, mode)
                end = S.end_cell(F, mode)
                if end is None:
                    continue
                want = A.walk(qa, t, F, end[1], end[2], sc) if mode == "local" else E.walk(qa, t, F, end[2], sc)
                assert S.walk(qa, t, F, end[1], end[2], sc, mode) == want, (name, r)
    if mode == "local":                             # and open_wins=False is align_affine_ref's
        q, t = b"A" * 70 + b"ACGTTGCA", b"A" * 66 + b"ACGTTGCA"
        F = A.fill(q, t, A.MM2)
        _, i, j = R.end_cell(F[0])
        assert S.walk(q, t, F, i, j, A.MM2, mode, open_wins=False) == A.walk(q, t, F, i, j, A.MM2, open_wins=False)


# ---- end_order_case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", STANDARD, ids=S.scoring_id)
def test_the_end_cell_order_is_pinned_across_lanes_blocks_and_refills(sc):
    case = S.end_order_case()
    pairs = S.submitted(case)
    lower_lane = far = 0
    for r in S.END_ORDER_LOCAL:
        _, q, t = pairs[r]
        F = S.fill(q, t, sc, "local")
        top = max(max(row) for row in F[0])
        win, lose = S.end_cell(F, "local"), S.end_cell_ji(F, "local")
        assert win == (20 * sc[0], 20, len(t)) and lose == (20 * sc[0], len(q), 20) and top == win[0]       # two cells hold the maximum
        assert sum(row.count(top) for row in F[0]) == 2
        lower_lane += (lose[1] - 1) % 64 < (win[1] - 1) % 64
        # the loser two row blocks below the winner, and the two columns two refills apart
        far += (lose[1] - 1) // 64 >= (win[1] - 1) // 64 + 2 and abs((lose[2] - 1) // 64 - (win[2] - 1) // 64) >= 2
    assert lower_lane >= 1 and far >= 1
    # pair 3, |J1| = 30: the loser's row 70 is lane 5 of block 1, the winner's row 20 lane 19 of block 0 -- lane order is not row order
    assert len(pairs[3][1]) == 70 and ((70 - 1) % 64, (70 - 1) // 64) == (5, 1) and ((20 - 1) % 64, (20 - 1) // 64) == (19, 0)
    for r in S.END_ORDER_READ:
        _, q, t = pairs[r]
        assert case[3][r] == r - S.END_ORDER_READ[0] and len(q) == 20
        for mode in S.MODES:                        # one row: the local maximum is the last row's
            F = S.fill(q, t, sc, mode)
            last = F[0][-1]
            tied = tuple(j for j in range(1, len(last)) if last[j] == max(last[1:]))
            assert tied == S.END_ORDER_COLUMNS and sorted((j - 1) // 64 for j in tied) == [0, 1, 2]      # three refills
            assert S.end_cell(F, mode) == (20 * sc[0], 20, 20)
        assert S.end_cell_ji(F, "read") == (20 * sc[0], 20, 170)


# ---- shifted_tie_case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S.MODES)
def test_the_shifted_ties_pin_both_rules_beyond_the_first_block(mode):
    """under 2,4,4,2: extend-before-open changes at least 5 pairs beyond row 64 and H order "udl" at least 10 (measured: 9 and 25 locally,
    9 and 52 in read mode, of 108); the H ties on chosen paths beyond row 64 outnumber the 203 of the best case before"""
    pairs = gap_rule = gap_beyond = h_rule = h_beyond = h_ties = g_ties = 0
    cells = []
    for name in S.SHIFTED:
        case = ALL[name]()
        assert R.cells(case) <= 2_000_000
        pairs += len(case[1])
        changed, beyond, ties = S.wrong_rule(case, A.MM2, mode, open_wins=False)
        gap_rule, gap_beyond = gap_rule + changed, gap_beyond + beyond
        changed, beyond, _ = S.wrong_rule(case, A.MM2, mode, order="udl")
        h_rule, h_beyond = h_rule + changed, h_beyond + beyond
        h_ties += sum(S.count_ties(c, "h", row=64) for c in ties)
        g_ties += sum(S.count_ties(c, "g", row=64) for c in ties)
        cells += [c for cs in ties for c in cs]
    print(mode, "extend before open:", gap_rule, gap_beyond, "udl:", h_rule, h_beyond, "ties beyond row 64, H and gap:", h_ties, g_ties)
    assert pairs == 108 and gap_beyond >= 5 and h_beyond >= 10
    assert h_ties >= 800 and g_ties >= 5
    # and the ties lie on and around the edges: in rows and in columns 64, 65, 128 and 129 of some pair
    assert {64, 65, 128, 129} <= {i for i, _, _ in cells} and {64, 65, 128, 129} <= {j for _, j, _ in cells}


def test_the_shifts_are_the_edges():
    assert S.SHIFTS == (24, 57, 60, 63, 64, 88, 121, 127, 128) and sorted(n for part in S.SHIFT_PARTS for n in part) == list(S.SHIFTS)
    base = list(zip(R.tie_cases()[1], R.tie_cases()[0])) + list(zip(A.homopolymer_case()[1], A.homopolymer_case()[0]))
    for part, name in zip(S.SHIFT_PARTS, S.SHIFTED):
        targets, reads, tor, rev = ALL[name]()
        assert len(reads) == 12 * len(part) and not any(rev)
        for k, (q, x) in enumerate(zip(reads, tor)):
            n, (bq, bt) = part[k // 12], base[k % 12]
            assert q[n:] == bq and targets[x][n:] == bt and q[:n] == targets[x][:n] and len(q) == n + len(bq)


# ---- "up before left" -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", S.CHEAP_GAPS, ids=S.scoring_id)
@pytest.mark.parametrize("mode", S.MODES)
def test_up_before_left_decides_under_cheap_gaps(sc, mode):
    """a mismatch costs more than a gap in each sequence: H order "dlu" changes at least 20 pairs of edges + random, 5 beyond row 64
    (measured: 84 and 33 locally, 83 and 43 in read mode, of 109) -- against 1 to 4 pairs under 5,4,8,8, 5,4,8,6 and 5,4,12,1"""
    assert sc[1] > 2 * sc[2]
    changed = beyond = 0
    for name in ("edges", "random"):
        c, b, _ = S.wrong_rule(ALL[name](), sc, mode, order="dlu")
        changed, beyond = changed + c, beyond + b
    print(mode, sc, "dlu:", changed, beyond)
    assert changed >= 20 and beyond >= 5


def test_up_before_left_decided_little_before():
    """the same count on the same cases under 5,4,8,6: a handful"""
    changed = sum(S.wrong_rule(ALL[name](), A.ENGINE, "local", order="dlu")[0] for name in ("edges", "random"))
    assert changed <= 4


# ---- strand_edge_case -----------------------------------------------------------------------------------------------------------------
def test_the_strand_edges_sit_on_their_rows():
    case = S.strand_edge_case()
    targets, reads, tor, rev = case
    assert R.cells(case) <= 2_000_000 and all(s == 1 for s in rev) and all(b"T" not in q for q in reads) and any(b"U" in q for q in reads)
    spans = [n for n in S.STRAND_SPANS for _ in S.STRAND_FLANKS] + [n for n in S.STRAND_SPANS for _ in S.STRAND_FLANKS[1:]]
    after = [f[1] for _ in S.STRAND_SPANS for f in S.STRAND_FLANKS] + [f[1] for _ in S.STRAND_SPANS for f in S.STRAND_FLANKS[1:]]
    for sc in STANDARD:
        want = A.records(*case, sc)
        assert (want["status"] == 0).all()
        assert set((want["q_end"] - want["q_start"]).tolist()) == {1, 63, 64, 65, 127, 128, 129}
        starts = set(want["q_start"].tolist())
        assert 0 in starts and any(1 <= s <= 63 for s in starts) and any(s >= 64 for s in starts)
        # the alignment is the span exactly, without an indel: rows (|f2|, |f2| + n] of the read as given, columns (|g1|, |g1| + n]
        for r, (n, f2) in enumerate(zip(spans, after)):
            g1 = f2 if r < 21 else 0
            assert [int(want[f][r]) for f in ("q_start", "q_end", "t_start", "t_end", "q_gap", "t_gap")] == [f2, f2 + n, g1, g1 + n, 0, 0], r
            assert want["mismatches"][r] == len(range(10, n - 8, 20))
    # the transcript shorter than the read: in read mode both overhangs are I runs, on the reverse strand
    for r in range(21, 35):
        assert len(targets[tor[r]]) < len(reads[r])
        rec, ops = E.pair(reads[r], targets[tor[r]], 1, A.ENGINE)
        n1, n2 = len(reads[r]) - spans[r] - after[r], after[r]
        assert ops[0] == ("I", n1) and ("I", n2) in ops[-2:] and rec[4:6] == (0, spans[r]) and rec[8:10] == (n1 + n2, 0)


# ---- many_blocks_case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("many_blocks", "many_blocks_t"))
def test_the_long_pairs_align_across_sixteen_blocks(name):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000 and len(case[1]) == 1 and case[3] == [name == "many_blocks"]
    assert (len(case[1][0]) + 63) // 64 >= 17 and (len(case[0][0]) + 63) // 64 >= 17
    for sc in (A.LINEAR, A.ENGINE):
        rec = A.pair(case[1][0], case[0][0], case[3][0], sc)[0]
        assert rec[0] == 0 and rec[3] - rec[2] >= 1024 and rec[5] - rec[4] >= 1024
    # (the rectangle does not begin on a block edge of kernel E on the strand aligned: kernel F's blocks are not kernel E's)
    q, t, s = case[1][0], case[0][0], case[3][0]
    first_row = len(q) - rec[3] if s else rec[2]
    assert first_row % 64 != 0
