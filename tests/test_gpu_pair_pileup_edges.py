"""Kernel G (csrc/pair_pileup.hip) where tests/test_gpu_pair_pileup.py does not reach, through the same `expect`: records, CIGARs, the
table against the model and against the call's own CIGARs, the identities.  One interior I op at a chosen op index -- the last lane of
a round of 64 ops, the first lane of the next, the last op but one, op counts of 65, 66 and 129 -- where "not the last op" looks across
the round's edge; a read-mode overhang alone in its round, and one as op 0 of 134; all of these and the pairs of 63 to 129 ops handed
over on the reverse strand, where the rows run backwards and their offset accumulates over the rounds; 4096 reads with a D run and an I
run on the same positions.  Every pair is first held to the ops it is named for by the model (tests/pileup_ref.py)."""
import numpy as np
import pytest

import align_model as M
import align_ref as R
import cigar_ref as CR
import pileup_ref as P
from test_gpu_pair_pileup import expect, got_table, run, stacked

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,mode", P.INS_FORMS)
def test_one_interior_i_op_at_a_chosen_index(gpu_ctx, name, mode):
    sc, ops, index, position, q, t = P.ins_pairs(name, mode)             # (asserts the ops through the model)
    assert 0 < index < ops - 1
    rec, (offsets, _), table = expect(gpu_ctx, "ins_" + name, R.pairs_case([(q, t, 0)]), sc, mode)
    assert int(offsets[1]) == ops
    assert int(table["ins"].sum()) == 1 and int(table["ins"][position]) == 1, (name, mode, np.nonzero(table["ins"])[0])


def _strand_pairs():
    out = [("ins_" + name, mode) for name, mode in P.INS_FORMS]
    return out + [("ops_" + name, P.op_count_pairs()[name][1]) for name in sorted(P.op_count_pairs())]


@pytest.mark.parametrize("name,mode", _strand_pairs())
def test_the_same_pairs_on_the_reverse_strand(gpu_ctx, name, mode):
    """the read reverse-complemented and written with U, rev = 1: the same CIGAR, the same table"""
    if name.startswith("ins_"):
        sc, ops, _, _, q, t = P.ins_pairs(name[4:], mode)
    else:
        sc, _, ops, q, t = P.op_count_pairs()[name[4:]]
    back = P.reverse_given(q)
    assert back != q and b"T" not in back and R.revcomp(back) == q
    forward = P.model(name, R.pairs_case([(q, t, 0)]), sc, mode)
    assert len(P.parse(forward[1][0])) == ops
    rec, cg, table = expect(gpu_ctx, "rev_" + name, R.pairs_case([(back, t, 1)]), sc, mode)
    assert CR.split(*cg) == forward[1]
    assert (got_table(table) == stacked(forward[2])).all()


def test_contention_on_the_gap_planes(gpu_ctx):
    """4096 reads, both strands, each with 3 target bases missing and 2 bases more: del and ins under the contention the letters see"""
    q, t = P.gap_contention_pair()
    case = P.gap_contention_case()
    n = P.GAP_COPIES
    for rev, given in ((0, q), (1, P.reverse_given(q))):
        assert CR.text(M.pair(given, t, rev, P.ENGINE, M.LOCAL)[1]) == P.GAP_CONTENTION_CIGAR       # the model spans both gaps
    assert len(case[1]) == n and sum(case[3]) == n // 2 and (len(q), len(t)) == (100, 101)
    aligned = q[:67] + q[69:]                                            # the read's bases that stand in a column
    for cigars in (False, True):
        rec, cg, table = run(gpu_ctx, case, P.ENGINE, M.LOCAL, cigars=cigars)
        assert (rec["status"] == 0).all() and (rec["matches"] == 98).all() and (rec["t_gap"] == 3).all() and (rec["q_gap"] == 2).all()
        if cigars:
            assert set(CR.split(*cg)) == {P.GAP_CONTENTION_CIGAR}
        got = got_table(table)
        assert got.shape == (8, 101)
        for j in range(101):
            gone = 35 <= j < 38
            base = None if gone else aligned[j if j < 35 else j - 3]
            want = [n if b"ACGT"[k] == base else 0 for k in range(4)] + [n if gone else 0, n if j == 70 else 0, n if j == 0 else 0, n if j == 100 else 0]
            assert list(got[:, j]) == want, j
        assert P.identities(P.as_lists(table), rec) == []
