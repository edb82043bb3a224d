"""The packs of tests/constructed_alphabets.py sit where their names say -- on the CPU oracle alone, no GPU.  The oracle compares letters
as bytes, as the reference does.  What is proven here: the MSA of every `strands`, `late` and `alias` pack changes its gap pattern when
every byte is replaced by its table twin (so a kernel that scored such a pack from the (c >> 1) & 3 table, where it must compare, gives
other rows than the oracle); where U arrives in a `late` pack; that every constructed column of a `five` pack is one MSA column of five
letters; that `six` needs a sixth; that no other pack needs more than five; and the pack groups of the band packs and of the class 4 pack.
tests/test_gpu_poa_alphabet.py runs the same packs through kernel C."""
import numpy as np
import pytest

import constructed_alphabets as ca
from test_gpu_poa_variants import POA_BAND_SPREAD, _group_of

GAP = ord("-")


@pytest.fixture(scope="module")
def msa(oracle):
    """Oracle.poa_msa's rows as a matrix, with the AVX2 rows (exact where they run, 5 L + 64 < 32 000; the scalar loops elsewhere)"""
    def run(pack):
        oracle.set_poa_simd(True)
        try:
            rows, _ = oracle.poa_msa(list(pack))
        finally:
            oracle.set_poa_simd(False)
        return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
    return run


@pytest.fixture(scope="module")
def table_msa(oracle):
    """Oracle.poa_msa_table: the oracle with the table's scoring rule (letters of one (c >> 1) & 3 match), nodes still told apart by byte --
    what a kernel gives that takes the score table for a pack it must compare"""
    def run(pack):
        oracle.set_poa_simd(True)
        try:
            rows = oracle.poa_msa_table(list(pack))
        finally:
            oracle.set_poa_simd(False)
        return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
    return run


def letters_per_column(mat):
    """distinct non-gap letters of every column"""
    return np.array([len(set(col.tolist()) - {GAP}) for col in mat.T])


def same_gaps(a, b):
    return a.shape == b.shape and np.array_equal(a == GAP, b == GAP)


def test_twin_is_the_table_index():
    for c in range(256):
        t = ca.twin([bytes([c])])[0][0]
        assert t in b"ACGT" and (t >> 1) & 3 == (c >> 1) & 3
    assert ca.twin([b"ACGTU", b"@aBctFgN\x80"]) == [b"ACGTT", b"AACCTGGGA"]
    # every byte of ALIAS has the table index of its set's letter, and no two sets share one
    assert [{(c >> 1) & 3 for c in a} for a in ca.ALIAS] == [{0}, {1}, {2}, {3}]
    assert len(set(ca.ALIAS_ALL.tolist())) == len(ca.ALIAS_ALL) == 14


def test_simd_and_scalar_rows_agree_on_other_bytes(oracle, msa):
    """the AVX2 rows of the oracle compare bytes as the scalar loops do, also 0x80 and lower case"""
    for pack in (ca.alias(0), ca.strands(0, "interleaved")):
        rows, _ = oracle.poa_msa(pack)
        assert np.array_equal(msa(pack), np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1))


def test_table_oracle_on_hand_packs(oracle, msa, table_msa):
    """on one alphabet the table's rule is the true one; on T against U it is not, and the rows show it"""
    for pack in ([b"ACGTACGTTTGACA", b"ACGACGTTTGACA", b"GTTACGA"], ca.twin(ca.strands(0, "interleaved")), ca.twin(ca.alias(0))):
        assert np.array_equal(table_msa(pack), msa(pack))
    pack = [b"ACGGATTTTTTTTCAGGA", b"ACGGAUUUUUUUUCAGGA"]
    assert msa(pack).shape[1] > 18 and table_msa(pack).shape[1] == 18           # eight mismatches cost more than a flank brings (32 > 25); as matches they align
    assert table_msa(pack)[1].tobytes() == pack[1]


@pytest.mark.parametrize("name", sorted(ca.twin_packs()))
def test_twins_change_the_result(msa, table_msa, name):
    """the pack under the table's scoring rule (every byte its twin: T = U, A = @ = a ...) has another gap pattern than the pack itself,
    and so have the rows of an aligner that scores the pack itself by that rule"""
    pack = ca.twin_packs()[name]
    cls = int(name[-1])
    assert 6 <= len(pack) <= 8 and _group_of(pack) == cls and abs(max(map(len, pack)) - ca.LENGTHS[cls]) < 40
    real, table = msa(pack), msa(ca.twin(pack))
    assert not same_gaps(real, table), name
    assert not same_gaps(real, table_msa(pack)), name
    assert letters_per_column(real).max() <= 5, "the pack needs more than five letters in a column"
    kinds = {bytes(sorted(set(s) - set(b"ACG"))) for s in pack}
    if name.startswith(("strands", "late")):
        assert kinds == {b"T", b"U"}                                   # every read in one alphabet, the pack in two
        both = (real == ord("T")).any(0) & (real == ord("U")).any(0)
        assert both.sum() > ca.LENGTHS[cls] // 8                        # T and U share many columns
    else:
        assert set(b"".join(pack)) == set(ca.ALIAS_ALL.tolist())


@pytest.mark.parametrize("cls", range(4))
@pytest.mark.parametrize("order", ca.ORDERS)
def test_strands_orders(cls, order):
    pack = ca.strands(cls, order)
    u = "".join("U" if b"U" in s else "T" for s in pack)
    assert u == {"interleaved": "UTUTUTUT", "u_first": "UUUUTTTT", "t_first": "TTTTUUUU"}[order]


@pytest.mark.parametrize("cls", range(4))
@pytest.mark.parametrize("where", ca.WHERE)
def test_late_prefixes(cls, where):
    """the first m reads hold no byte outside ACGT, read m holds U"""
    pack = ca.late(cls, where)
    m = ca.late_m(where)
    assert m == {"second": 1, "middle": 4, "last": 7}[where] and len(pack) == 8
    assert all(set(s) <= set(b"ACGT") for s in pack[:m]) and b"U" in pack[m] and b"T" not in pack[m]


@pytest.mark.parametrize("cls", range(4))
def test_five_columns(msa, cls):
    """every constructed column is one MSA column of exactly five letters, no other column has more than one, and no read was shifted"""
    pack, cols = ca.five(cls)
    L = ca.LENGTHS[cls]
    assert len(pack) == 7 and all(len(s) == L for s in pack) and _group_of(pack) == cls
    assert cols[1] == cols[0] + 1 and 10 < min(cols) and max(cols) < L - 10
    assert all(sorted(o) == sorted(b"ACGTU") for o in ca.FIVE_ORDERS) and len({o.index(b"U") for o in ca.FIVE_ORDERS}) == 4
    mat = msa(pack)
    assert mat.shape == (7, L) and not (mat == GAP).any()
    n = letters_per_column(mat)
    assert [int(n[c]) for c in cols] == [5] * 4 and int((n > 1).sum()) == 4
    for c, order in zip(cols, ca.FIVE_ORDERS):
        assert mat[:5, c].tobytes() == order


def test_six_needs_a_sixth_letter(msa):
    """the oracle has no limit: six letters in that column, five in the other constructed ones"""
    pack, c = ca.six()
    mat = msa(pack)
    assert mat.shape == (6, ca.LENGTHS[0]) and mat[:, c].tobytes() == ca.FIVE_ORDERS[2] + b"N"
    n = letters_per_column(mat)
    assert int(n[c]) == 6 and sorted(n[n > 1].tolist()) == [5, 5, 5, 6]
    assert pack[:5] == ca.five(0)[0][:5]


@pytest.mark.parametrize("cls", range(4))
@pytest.mark.parametrize("shape", ca.NEAR_SHAPES)
def test_near_packs_are_band_packs(msa, cls, shape):
    pack = ca.near(cls, shape)
    assert ca.POA_BAND_SPREAD == POA_BAND_SPREAD and 3 <= len(pack) <= 5
    assert len(pack[0]) == ca.LENGTHS[cls] and len(pack[0]) - min(map(len, pack)) < 300 < POA_BAND_SPREAD
    assert _group_of(pack, band=True) == 16 + cls and _group_of(pack) == cls
    u = [b"U" in s for s in pack]
    assert not any(b"T" in s and b"U" in s for s in pack)
    if shape == "late":
        assert u == [False] * (len(pack) - 1) + [True]
    else:
        assert u == [k % 2 == 0 for k in range(len(pack))]
    assert letters_per_column(msa(pack)).max() <= 5


def test_class4_pack():
    pack = ca.class4()
    assert len(pack) == 2 and 2560 < max(map(len, pack)) <= 4096 and _group_of(pack) == 8
    assert b"U" in pack[0] and b"T" not in pack[0] and b"T" in pack[1] and b"U" not in pack[1]


def test_form_packs_are_distinct_and_in_their_classes():
    packs = ca.form_packs()
    assert len(packs) == 32 and len(set(map(tuple, packs.values()))) == 32
    for name, p in packs.items():
        assert _group_of(p) == int(name[-1]), name
        assert not any(0 in s or GAP in s for s in p), name
