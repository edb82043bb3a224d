"""tests/pileup_ref.py, the plain-Python contract of `align_pileup`, held to hand-written tables, to the header's identities on every
case of the alignment models, and its constructed cases to the edges they are named after.  No device."""
import numpy as np
import pytest

import align_affine_ref as AF
import align_ends_ref as AE
import align_model as M
import align_ref as R
import pileup_ref as P


def rec(rows):
    """records from (status, q_start, q_end, t_start, t_end) per read; the other fields are not read by table()"""
    f = {"status": 0, "q_start": 1, "q_end": 2, "t_start": 3, "t_end": 4}
    return {k: np.array([r[i] for r in rows]) for k, i in f.items()}


def sparse(planes):
    """{field: {position: count}} of the counts that are not zero"""
    return {f: {j: v for j, v in enumerate(p) if v} for f, p in zip(P.FIELDS, planes) if any(p)}


def test_parse_refuses_what_is_no_cigar():
    assert P.parse(b"3I10=2I5=4I") == [(b"I", 3), (b"=", 10), (b"I", 2), (b"=", 5), (b"I", 4)]
    with pytest.raises(AssertionError):
        P.parse(b"3I10M")


def test_forward_read_with_every_op():
    #            0123456789
    t = b"ACGTACGTAC"
    q = b"CGAAATTA"
    got = P.table([t], [q], [0], [0], rec([(0, 0, 8, 1, 9)]), [b"2=1X2I1X2D2="])
    # i: C G | A | A A | T | - - | T A        j: 1 2 | 3 | . . | 4 | 5 6 | 7 8
    assert sparse(got) == {"c": {1: 1}, "g": {2: 1}, "a": {3: 1, 8: 1}, "t": {4: 1, 7: 1}, "del": {5: 1, 6: 1}, "ins": {4: 1},
                           "starts": {1: 1}, "ends": {8: 1}}
    assert P.depth(got) == [0, 1, 1, 1, 1, 1, 1, 1, 1, 0]


def test_reverse_strand_read_written_with_u():
    t = b"GGACGTTT"
    q = b"AACGU"               # as given; reverse-complemented: ACGTT, on t[2:7]
    got = P.table([t], [q], [0], [1], rec([(0, 0, 5, 2, 7)]), [b"5="])
    assert sparse(got) == {"a": {2: 1}, "c": {3: 1}, "g": {4: 1}, "t": {5: 1, 6: 1}, "starts": {2: 1}, "ends": {6: 1}}
    # clipped on the read as given: q_start 1, q_end 4 is rows 1 .. 3 of the aligned strand, CGT
    got = P.table([t], [q], [0], [1], rec([(0, 1, 4, 3, 6)]), [b"3="])
    assert sparse(got) == {"c": {3: 1}, "g": {4: 1}, "t": {5: 1}, "starts": {3: 1}, "ends": {5: 1}}


def test_read_mode_only_the_middle_insertion_counts():
    t = b"A" * 4 + b"C" * 10 + b"G" * 5 + b"T" * 3
    q = b"TTT" + b"C" * 10 + b"AA" + b"G" * 5 + b"TTTT"
    got = P.table([t], [q], [0], [0], rec([(0, 0, 24, 4, 19)]), [b"3I10=2I5=4I"])
    assert sparse(got) == {"c": {j: 1 for j in range(4, 14)}, "g": {j: 1 for j in range(14, 19)}, "ins": {14: 1},      # the 5='s first base
                           "starts": {4: 1}, "ends": {18: 1}}


def test_no_column_and_other_statuses_add_nothing():
    t = b"ACGT"
    rows = [(0, 0, 2, 3, 3), (1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (3, 0, 0, 0, 0)]
    got = P.table([t], [b"CC", b"AC", b"AC", b"AC"], [0, 0, 0, -1], [0, 0, 0, 0], rec(rows), [b"2I", b"", b"", b""])
    assert sparse(got) == {}


def test_second_target_begins_where_the_first_ends():
    got = P.table([b"ACG", b"TTAC"], [b"CG", b"TT"], [0, 1], [0, 0], rec([(0, 0, 2, 1, 3), (0, 0, 2, 0, 2)]), [b"2=", b"2="])
    assert sparse(got) == {"c": {1: 1}, "g": {2: 1}, "t": {3: 1, 4: 1}, "starts": {1: 1, 3: 1}, "ends": {2: 1, 4: 1}}


def _model_cases():
    out = []
    for mode, cases, ref in ((M.LOCAL, AF.all_cases(), AF), (M.READ, AE.all_cases(), AE)):
        for name in sorted(cases):
            scorings = ref.SCORINGS if name in ref.EDGE_CASES else (AF.LINEAR, AF.ENGINE)
            out += [(name, sc, mode) for sc in scorings]
    return out


@pytest.mark.parametrize("name,sc,mode", _model_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_identities_on_the_models_cases(name, sc, mode):
    case = (AE if mode == M.READ else AF).all_cases()[name]()
    records, _, planes = P.model(name, case, sc, mode)
    assert P.identities(planes, records) == []
    assert len(planes[0]) == sum(len(t) for t in case[0])


@pytest.mark.parametrize("name", sorted(P.op_count_pairs()))
def test_op_count_pairs_have_the_intended_number_of_ops(name):
    sc, mode, ops, q, t = P.op_count_pairs()[name]
    assert P.n_ops(q, t, sc, mode) == ops
    case = R.pairs_case([(q, t, 0)])
    records, _, planes = P.model("ops_" + name, case, sc, mode)
    assert P.identities(planes, records) == []


@pytest.mark.parametrize("name,mode", P.INS_FORMS)
def test_ins_pairs_hold_one_interior_i_op_at_the_index_they_are_named_for(name, mode):
    sc, ops, index, position, q, t = P.ins_pairs(name, mode)             # (asserts count, index and position through the model)
    named = name.split("_")
    if named[0] == "index":
        assert index == int(named[1]) and (len(named) == 2 or ops == int(named[3]))
    texts = M.cigars(*R.pairs_case([(q, t, 0)]), sc, mode)
    parsed = P.parse(texts[0])
    assert len(parsed) == ops and [k for k, (o, _) in enumerate(parsed) if o == b"I" and 0 < k < ops - 1] == [index]
    if name == "trailing_overhang":
        assert ops == 65 and parsed[64] == (b"I", 7) and index < 64      # the overhang is alone in the second round of 64 ops
    if name == "leading_overhang":
        assert ops > 64 and parsed[0] == (b"I", 3)
    # the table: that one count, at that position, and on both strands the same
    case = R.pairs_case([(q, t, 0)])
    records, _, planes = P.model("ins_" + name, case, sc, mode)
    assert sum(planes[P.INS]) == 1 and planes[P.INS][position] == 1 and P.identities(planes, records) == []
    back = P.reverse_given(q)
    rec2, texts2, planes2 = P.model("rev_ins_" + name, R.pairs_case([(back, t, 1)]), sc, mode)
    assert texts2 == texts and planes2 == planes and P.identities(planes2, rec2) == []
    assert int(rec2["q_start"][0]) == len(q) - int(records["q_end"][0]) and int(rec2["q_end"][0]) == len(q) - int(records["q_start"][0])


def test_ins_pairs_cover_the_indices_at_the_round_edges():
    have = {(forms[mode][1], forms[mode][0]) for _, forms in P.INS_PAIRS.values() for mode in forms}
    assert {i for i, _ in have} >= {1, 63, 64, 65, 127, 128} and {(63, 65), (64, 66), (127, 129), (131, 133)} <= have
    for mode in M.MODES:                                                 # ... each index under both forms (127 of 129 ops: read mode alone)
        mine = {forms[mode][1] for name, (_, forms) in P.INS_PAIRS.items() if mode in forms and name.startswith("index")}
        assert mine >= {1, 63, 64, 65, 127, 128, 131}


@pytest.mark.parametrize("name", sorted(P.op_count_pairs()))
def test_op_count_pairs_on_the_reverse_strand_give_the_forward_table(name):
    sc, mode, ops, q, t = P.op_count_pairs()[name]
    _, texts, planes = P.model("ops_" + name, R.pairs_case([(q, t, 0)]), sc, mode)
    rec2, texts2, planes2 = P.model("rev_ops_" + name, R.pairs_case([(P.reverse_given(q), t, 1)]), sc, mode)
    assert texts2 == texts and planes2 == planes and P.identities(planes2, rec2) == [] and b"T" not in P.reverse_given(q)


def test_gap_contention_case_spans_both_gaps_on_both_strands():
    q, t = P.gap_contention_pair()
    case = P.gap_contention_case()
    assert (len(q), len(t)) == (100, 101) and len(case[1]) == P.GAP_COPIES and sum(case[3]) == P.GAP_COPIES // 2
    assert set(case[1]) == {q, P.reverse_given(q)} and case[1][0] == q and case[3][:2] == [0, 1]
    for rev, given in ((0, q), (1, P.reverse_given(q))):
        assert M.pair(given, t, rev, P.ENGINE, M.LOCAL)[1] == [("=", 35), ("D", 3), ("=", 32), ("I", 2), ("=", 31)]
    small = [t], case[1][:2], [0, 0], [0, 1]
    records, texts, planes = P.model("gap_contention_2", small, P.ENGINE, M.LOCAL)
    assert texts == [P.GAP_CONTENTION_CIGAR] * 2 and P.identities(planes, records) == []
    assert sparse(planes)["del"] == {35: 2, 36: 2, 37: 2} and sparse(planes)["ins"] == {70: 2}
    assert sparse(planes)["starts"] == {0: 2} and sparse(planes)["ends"] == {100: 2} and set(P.depth(planes)) == {2}


def test_constructed_cases_sit_on_their_edges():
    # identical: one '=' run each, of the named lengths
    case = P.identical_case()
    assert M.cigars(*case, P.LINEAR, M.LOCAL) == [b"1=", b"63=", b"64=", b"65=", b"129="]
    # long gaps: one D run (the insert in the target) or one I run (in the read) of 63, 64, 65 between whole flanks
    case = P.long_gap_case()
    assert M.cigars(*case, P.ENGINE, M.LOCAL) == [b"120=%d%s120=" % (n, o) for n in (63, 64, 65) for o in (b"D", b"I")]
    _, _, planes = P.model("long_gaps", case, P.ENGINE, M.LOCAL)
    assert sum(planes[P.INS]) == 3 and sum(planes[P.DEL]) == 63 + 64 + 65
    # contention: every copy is the whole target, on either strand
    case = P.contention_case()
    assert len(case[1]) == P.CONTENTION_COPIES and sum(case[3]) == P.CONTENTION_COPIES // 2
    assert M.pair(case[1][0], case[0][0], 0, P.LINEAR, M.LOCAL)[1] == [("=", 70)] == M.pair(case[1][1], case[0][0], 1, P.LINEAR, M.LOCAL)[1]
    # neighbours: counts up to the last base of target 0 and from base 0 of target 1, none across, none on target 2
    case = P.neighbours_case()
    records, _, planes = P.model("neighbours", case, P.LINEAR, M.LOCAL, P.NEIGHBOURS_MAX_CELLS)
    assert list(records["status"]) == [0, 0, 0, 0, 3, 1, 2]
    assert planes[P.ENDS][79] == 2 and planes[P.STARTS][80] == 2 and P.depth(planes)[79] == 2 and P.depth(planes)[80] == 2
    assert not any(P.depth(planes)[170:]) and not any(planes[P.STARTS][170:]) and len(planes[0]) == 220
    assert sum(planes[P.STARTS]) == 4
    # read mode: every CIGAR has an I run at an end and one inside, and only the inner ones count
    case = P.read_mode_case()
    texts = M.cigars(*case, P.ENGINE, M.READ)
    inner = 0
    for text in texts:
        ops = P.parse(text)
        assert ops[0][0] == b"I" or ops[-1][0] == b"I"
        assert any(o == b"I" for o, _ in ops[1:-1])
        inner += sum(o == b"I" for o, _ in ops[1:-1])
    assert (ops[0][0], ops[-1][0]) == (b"I", b"I")               # the last pair overhangs on both sides
    _, _, planes = P.model("read_mode", case, P.ENGINE, M.READ)
    assert sum(planes[P.INS]) == inner
    # ... and a pair without a column
    none = R.pairs_case([(b"CC", b"AA", 0)])
    records, texts, planes = P.model("no_column", none, AE.CHEAP_GAP, M.READ)
    assert texts == [b"2I"] and int(records["t_end"][0]) == int(records["t_start"][0]) and not any(any(p) for p in planes)
