"""Kernel C on constructed graphs: the in-degree, ring and far-row edges of every form of the row loop, byte for byte against the oracle.

The packs come from tests/constructed_graphs.py; tests/test_constructed_graphs.py proves on the CPU which graph each of them gives (the
in-degree of the fan node at every alignment, the exact distances of a ladder, the rows whose every in-edge is far, the rows without
in-edge in the middle of the order) and that its rows change when the row loop overlooks one of those in-edges (the probes).  Here every pack runs in the barrier form, the team forms (with their own and with short rings), the band
(rows and strips, four wavefronts and one), the long-chain groups, the wide and segmented classes with and without a ring, and behind the
fallback switches.  Which path a row takes follows from its proved distance and from the ring (or the teams' reach) that the RATTLE_TIMING
line of its group prints: every case asserts that R and R + 1 are among the ladder's distances for every ring it met."""
import pytest

import constructed_graphs as cg
from test_gpu_poa_variants import POA_BAND_SPREAD, POA_CHAIN_SEQS, _band_slots, _cheap_band_packs, _device_cus, _group_of, _run

pytestmark = pytest.mark.gpu

_PACKS = {}


def _packed():
    """name -> pack for the packed classes: ladders (distances 2 .. 26) in classes 0-3; in classes 0 and 1 the far ladders (254 .. 257),
    the fans (in-degree 10, 17, 10 with every other in-edge beyond a ring of 4, 10 with three in-edges beyond the distance byte, the fan
    whose ninth in-edge is near and whose tenth is beyond every reach, and the bubbles of the far-first fan) and the branches (all in-edges
    far; mid-order starts); the 17-fan in 2 and 3"""
    if not _PACKS:
        for cls in range(4):
            _PACKS["ladder/%d" % cls] = cg.ladder(1, 25, cg.PACKED_L[cls])
        for cls in (0, 1):
            for D in cg.FAR_DS:
                _PACKS["far%d/%d" % (D, cls)] = cg.far_ladder(D, (1000, 1300)[cls])
            for m, s in cg.SMALL_FANS:
                _PACKS["fan%d,%d/%d" % (m, s, cls)] = cg.class_fan(m, s, cls)[0]
            _PACKS["fan-near-last/%d" % cls] = cg.class_fan(12, 2, cls, order=cg.NEAR_LAST)[0]
            _PACKS["fan-far-first/%d" % cls] = cg.class_fan(*cg.FAR_FIRST, cls, far_first=True)[0]
            _PACKS["branches/%d" % cls] = cg.branches((700, 1200)[cls])
        for cls in (2, 3):
            _PACKS["fan16,2/%d" % cls] = cg.class_fan(16, 2, cls)[0]
        for name, p in _PACKS.items():
            assert _group_of(p) == int(name[-1]), name
        assert len(set(map(tuple, _PACKS.values()))) == len(_PACKS)
    return _PACKS


def _assert_ring_edges(lines, distances=cg.LADDER_DISTANCES, band_packs=None):
    """R and R + 1 of every ring the call met are distances the ladder has: the barrier forms' ring, the teams' reach, the band's slots (from
    the LDS bytes of the group's first pass, whose longest read is known).  Fails where a device gives a ring the ladder does not cover."""
    seen = set()
    for d in lines:
        if d["pk"] == 7:
            R = d["reach"]
        elif d["pk"] == 8:
            if d["pass"] != 0:
                continue
            tl = max(len(s) for p in band_packs if _group_of(p, band=True) == d["group"] for s in p)
            R = _band_slots(d["band"], ((tl + 3) // 4 * 4 + 15) & ~15)
            assert R is not None, d
        else:
            R = d["ring"]
        if R == 0:
            continue                                            # a form without a ring: every predecessor row comes from the record
        assert R in distances and R + 1 in distances, ("the ladder does not cover this ring", R, d)
        seen.add((d["pk"], R))
    return seen


_FORM_PK = {"dense": 1, "mt4": 7, "mt2": 7, "mt1": 7}
_TEAMS = {"mt4": 4, "mt2": 2, "mt1": 1}


@pytest.mark.parametrize("mode,slots", [(None, None), ("dense", None), ("mt4", None), ("mt2", None), ("mt1", None), ("mt4", 11), ("mt2", 6), ("mt1", 3)])
def test_packed_classes_on_constructed_graphs(gpu_ctx, oracle, capfd, monkeypatch, mode, slots):
    """Every packed pack in one call per form: the form the load picks, the barrier form (rings of 8 rows, 4 in class 1), the teams with the
    ring the device gives them and with rings of 11 / 6 / 3 slots (reach 7 / 4 / 3: most of the ladder and of every fan then comes from the
    record)."""
    packs = list(_packed().values())
    env = {}
    if mode:
        env["RATTLE_POA_MODE"] = mode
    if slots:
        env["RATTLE_POA_MT_SLOTS"] = str(slots)
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
    assert {d["group"] for d in lines} == {0, 1, 2, 3}
    for d in (d for d in lines if d["pass"] == 0):
        if mode:
            assert d["pk"] == _FORM_PK[mode] and d["cpl"] == (4, 6, 8, 10)[d["group"]], d
        if mode in _TEAMS:
            assert d["ring"] == _TEAMS[mode], d
            if slots:
                assert d["slots"] == slots and d["reach"] == slots - (_TEAMS[mode] if _TEAMS[mode] > 1 else 0), d
        if mode == "dense":
            assert d["ring"] == (8, 4, 8, 8)[d["group"]], d
    seen = _assert_ring_edges(lines)
    print("rings met:", sorted(seen))
    assert seen


def _big_fans():
    packs = [cg.big_fan(*f)[0] for f in cg.BIG_FANS] + [cg.big_fan(*cg.BIG_FANS[-1], cls=1)[0]]
    assert [len(p) for p in packs] == [256, 256, 256, 257, 261, 263, 263]
    return packs


@pytest.mark.parametrize("mode", ["dense", "mt4", "mt2", "mt1"])
def test_in_degree_byte_and_long_chain_fans(gpu_ctx, oracle, capfd, monkeypatch, mode):
    """Fans of 256 .. 263 sequences: alignment k sees in-degree k, so each pack walks the row loop through every in-degree up to 253 .. 258,
    and the probes at the end need the last in-edges.  Three packs of exactly POA_CHAIN_SEQS sequences stay in group 0 (in-degree up to 253,
    254 and 255: the in-degree byte of the record reaches its cap in an ordinary group); those of 257, 261 and 263 sequences are long chains
    (groups 12 and, for the class-1 pack, 13) and go over the cap (in-degree 256 and 258)."""
    packs = _big_fans()
    assert POA_CHAIN_SEQS == 256 and [_group_of(p) for p in packs] == [0, 0, 0, 12, 12, 12, 13]
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {"RATTLE_POA_MODE": mode})
    first = [d for d in lines if d["pass"] == 0]
    assert {d["group"] for d in first} == {0, 12, 13}, first
    assert {d["group"]: d["packs"] for d in first} == {0: 3, 12: 3, 13: 1}, first
    for d in first:
        assert d["pk"] == _FORM_PK[mode], d
    _assert_ring_edges(lines)


def _band_packs():
    """band ladders of classes 0-3 (distances 2 .. 13) and fans whose lengths, probes included, spread by less than POA_BAND_SPREAD:
    in-degree 10, 17 and 191 (m = 190 is the largest such fan at s = 2) and the near-last fan; in-degree 10 and 17 in class 1"""
    packs = [cg.ladder(1, 12, cg.PACKED_L[c], probe_left=None) for c in range(4)]
    packs += [cg.fan(9, 2, probe_left=None)[0], cg.fan(16, 2, probe_left=None)[0], cg.fan(190, 2, probes=[8, 50], probe_left=None)[0],
              cg.fan(12, 2, order=cg.NEAR_LAST, probe_left=None)[0], cg.class_fan(9, 2, 1, probe_left=None)[0], cg.class_fan(16, 2, 1, probe_left=None)[0]]
    for q in packs:
        assert max(map(len, q)) - min(map(len, q)) < POA_BAND_SPREAD and 16 <= _group_of(q, band=True) < 20
    return packs


@pytest.mark.parametrize("load", ["few", "many"])
@pytest.mark.parametrize("form", ["rows", "strips"])
def test_band_on_constructed_graphs(gpu_ctx, oracle, capfd, monkeypatch, form, load):
    """RATTLE_POA_BAND=1: the ladders and the fans are band packs (groups 16-19).  few: the packs alone, four wavefronts per pack and a ring of
    8 slots; many: among more than four band packs per CU, one wavefront per pack, and with these lengths a ring of 4 slots.  strips:
    RATTLE_POA_DEBUG=8, an alignment that gets no band runs the full rows as strips on the band's row loop."""
    packs = _band_packs()
    if load == "many":
        packs = packs + _cheap_band_packs(-(-33 * _device_cus() // 8))
    env = {"RATTLE_POA_BAND": "1"}
    if form == "strips":
        env["RATTLE_POA_DEBUG"] = "8"
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
    print("alignments with a certified band:", int(counters[5]), "failed certificates:", int(counters[6]))
    assert int(counters[5]) >= 1, counters
    first = [d for d in lines if d["pass"] == 0]
    assert {d["group"] for d in first} == {16, 17, 18, 19}, first
    for d in first:
        assert d["variant"] == ((4, 8, 1, 8) if load == "many" else (4, 8, 4, 8)), d
    seen = _assert_ring_edges([d for d in lines if d["pk"] == 8], cg.BAND_LADDER_DISTANCES, band_packs=packs)
    print("rings met:", sorted(seen))
    assert (8, 4 if load == "many" else 8) in seen, seen


@pytest.mark.parametrize("noring", [False, True])
def test_wide_and_segmented_classes_on_constructed_graphs(gpu_ctx, oracle, capfd, monkeypatch, noring):
    """Backbones of 3000, 5000, 7000 and 9000 nt (the last: two segments), shallow (groups 8-11): in-degree 1 .. 10 at a node 400 columns
    before the end and distances 2 .. 6 -- R and R + 1 of the rings of 4 and 3 rows; and the same without a ring (RATTLE_POA_NORING=1)."""
    packs = [cg.wide_pack(L)[0] for L in cg.WIDE_L]
    assert [_group_of(p) for p in packs] == [8, 9, 10, 11]
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {"RATTLE_POA_NORING": "1"} if noring else None)
    assert {d["group"] for d in lines} == {8, 9, 10, 11}
    for d in lines:
        assert (d["ring"] == 0) == noring, d
    seen = _assert_ring_edges(lines, range(2, 7))
    assert noring or {R for _, R in seen} == {3, 4}, seen


@pytest.mark.parametrize("env", [{"RATTLE_POA_DEBUG": "1", "RATTLE_POA_MODE": "dense"}, {"RATTLE_POA_DEBUG": "2", "RATTLE_POA_MODE": "mt4"}])
def test_fans_behind_the_fallback_switches(gpu_ctx, oracle, capfd, monkeypatch, env):
    """The full topological sort (bit 0; the label sweep it replaces branches on the in-degree too) and the plain traceback (bit 1) on the fans,
    the branches and the fan of in-degree 258, in one form each."""
    p = _packed()
    packs = [v for k, v in p.items() if k.startswith(("fan", "branches"))] + [_big_fans()[5]]
    _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
