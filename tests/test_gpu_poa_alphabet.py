"""Kernel C on packs that mix T and U, hold bytes that are no base, or need five letters in one column, byte for byte against the oracle.

The packed forms of the row loop score a pack of {A,C,G,T} or {A,C,G,U} from a table indexed by (c >> 1) & 3 and every other pack by
comparing bytes (poa.hip, S.plain, decided anew with every sequence of a pack).  The packs come from tests/constructed_alphabets.py;
tests/test_constructed_alphabets.py proves on the CPU that the MSA of each changes when the table's rule is applied to it, so a green
run here means the compare path ran and was right: in the barrier form and the team forms of all four column classes (with the teams'
own and with short rings), behind the fallback switches, in class 4, and for a band pack that loses the band when U arrives.  The sixth
letter in one column, which the aligned-group record cannot hold, is refused by name."""
import pytest

import constructed_alphabets as ca
from rattle_amd._lib import RattleError
from test_gpu_poa_variants import _band_edge_packs, _cheap_band_packs, _group_of, _run

pytestmark = pytest.mark.gpu

_FORM_PK = {"dense": 1, "mt4": 7, "mt2": 7, "mt1": 7}
_TEAMS = {"mt4": 4, "mt2": 2, "mt1": 1}


@pytest.mark.parametrize("mode,slots", [(None, None), ("dense", None), ("mt4", None), ("mt2", None), ("mt1", None), ("mt2", 6), ("mt1", 3)])
def test_mixed_alphabets_in_every_form(gpu_ctx, oracle, capfd, monkeypatch, mode, slots):
    """All `strands`, `late`, `alias` and `five` packs of the four packed classes in one call per form: the form the load picks, the
    barrier form (PK 1) and the teams (PK 7) on 4, 2 and 1 teams, the last two also with rings of 6 and 3 slots.  Under a forced form
    every group's timing line names the instance, so each of the sixteen <CPL, RING, 4, 1 | 7> variants has run its compare path."""
    packs = list(ca.form_packs().values())
    env = {}
    if mode:
        env["RATTLE_POA_MODE"] = mode
    if slots:
        env["RATTLE_POA_MT_SLOTS"] = str(slots)
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
    assert {d["group"] for d in lines} == {0, 1, 2, 3}
    if mode:
        for d in lines:
            assert d["pk"] == _FORM_PK[mode] and d["cpl"] == (4, 6, 8, 10)[d["group"]], d
            if mode in _TEAMS:
                assert d["ring"] == _TEAMS[mode], d
                if slots:
                    assert d["slots"] == slots, d
        assert {d["variant"] for d in lines if d["pass"] == 0} == {(cpl, r, 4, _FORM_PK[mode]) for cpl, r in
                                                                    zip((4, 6, 8, 10), (8, 4, 8, 8) if mode == "dense" else [_TEAMS[mode]] * 4)}


@pytest.mark.parametrize("form", ["rows", "strips"])
def test_a_band_pack_that_stops_being_plain(gpu_ctx, oracle, capfd, monkeypatch, form):
    """RATTLE_POA_BAND=1: near-identical packs of groups 16-19 that mix T and U (from the first alignment on, or with their last read)
    next to all-ACGT band packs of the same groups.  The band is tried only while a pack is plain: the mixed packs leave PK 8 and run
    again over the full rows, in a later pass, under a full-row instance; the plain ones keep their certified bands.  strips:
    RATTLE_POA_DEBUG=8 (an alignment without a band runs the full rows as strips; a pack that is not plain still leaves)."""
    mixed = [ca.near(cls, shape) for cls in range(4) for shape in ca.NEAR_SHAPES]
    plain = _cheap_band_packs(3) + _band_edge_packs(ca.LENGTHS)
    assert all(set(b"".join(p)) <= set(b"ACGT") for p in plain)
    packs = mixed + plain
    assert len(set(map(tuple, packs))) == len(packs)
    assert {_group_of(p, band=True) for p in mixed} == {_group_of(p, band=True) for p in plain} == {16, 17, 18, 19}
    env = {"RATTLE_POA_BAND": "1"}
    if form == "strips":
        env["RATTLE_POA_DEBUG"] = "8"
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
    print("alignments with a certified band:", int(counters[5]), "failed certificates:", int(counters[6]))
    assert int(counters[5]) >= 1, counters
    first = [d for d in lines if d["pass"] == 0]
    assert {d["group"] for d in first} == {16, 17, 18, 19} and all(d["pk"] == 8 for d in first), first
    for g in (16, 17, 18, 19):
        again = [d for d in lines if d["group"] == g and d["pass"] >= 1]
        assert again and all(d["pk"] != 8 for d in again) and max(d["packs"] for d in again) >= 2, (g, lines)


@pytest.mark.parametrize("debug", ["1", "2"])
def test_strands_behind_the_fallback_switches(gpu_ctx, oracle, capfd, monkeypatch, debug):
    """The full topological sort for ties (bit 0) and the plain traceback (bit 1, which compares letters itself) on the `strands` packs,
    in the barrier form."""
    packs = [ca.strands(cls, order) for cls in range(4) for order in ca.ORDERS]
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {"RATTLE_POA_DEBUG": debug, "RATTLE_POA_MODE": "dense"})
    assert {(d["group"], d["pk"]) for d in lines} == {(0, 1), (1, 1), (2, 1), (3, 1)}


def test_class_4_pack(gpu_ctx, oracle, capfd, monkeypatch):
    """the wide rows (one score path, compares only) on a U read against a T read"""
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, [ca.class4()])
    assert {(d["group"], d["pk"]) for d in lines} == {(8, 3)}, lines


def test_a_sixth_letter_in_one_column_is_refused_by_name(gpu_ctx, oracle, capfd, monkeypatch):
    """An aligned group holds five nodes.  The pack that needs a sixth ends the call with an argument error that names the pack and the
    limit, and the context goes on: the same five reads without the sixth give the oracle's rows."""
    pack, _ = ca.six()
    with pytest.raises(RattleError) as e:
        gpu_ctx.poa_msa([pack])
    assert "error -2:" in str(e.value) and "pack 0" in str(e.value) and "five distinct letters" in str(e.value), str(e.value)
    _run(gpu_ctx, oracle, capfd, monkeypatch, [ca.five(0)[0], pack[:5]])
