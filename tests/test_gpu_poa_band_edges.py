"""Kernel C's exact band (poa.hip step 3a, `dp_rows_band`) on the packs of tests/constructed_bands.py: every one sits ON a comparison of
the band's plan -- the certificate's bound and one below it, the window's outermost column on either side, the clamp t = L - 1, the skip
C < L - t, the ladder 2 -> 4 -> 8, the history rule, the strips a pack has or has not earned -- and tests/test_constructed_bands.py proves
on the CPU that it does.  Here the rows must be the oracle's byte for byte, and the band's counters must be what the plan model
(constructed_bands.plan_pack, written from DESIGN.md §4) says: a `>=` written as `>`, a window placed with the wrong sign or a rule the
document does not state shows as a counter that differs; a window or certificate that is too lax shows as rows that differ."""
import pytest

import constructed_bands as cb
from test_constructed_bands import CASES, facts_of, plan_of
from test_gpu_poa_variants import _cheap_band_packs, _device_cus, _group_of, _run

pytestmark = pytest.mark.gpu

BAND = {"RATTLE_POA_BAND": "1"}
# what has no band at some alignment: the failures at the widest window and the strips packs
NO_BAND = sorted(n for n in CASES if n.endswith("_8_off") or CASES[n]["family"] == "strips" or n == "clamp_63_junk")


def _figures(name, oracle, plan, counters, note=""):
    """one line per case for whoever measures (pytest -s): the model's attempts of the case's own alignment and the device's counters"""
    c = CASES[name]
    facts = facts_of(oracle, name)
    k = c.get("edge")
    att = ""
    if k is not None and k <= len(plan["alignments"]):
        f = facts[k - 1]
        att = " ".join("(cplb %d t %d s %d S %d threshold %d %s)" % (a[0], a[1], a[2], f["S"], cb.threshold(f["L"], a[1]), "certified" if a[3] else "failed")
                       for a in plan["alignments"][k - 1]["attempts"])
    print("BANDCASE %s%s: model ok %d fail %d strips %d cells %d back %s %s| device cells %d of %d, ok %d, fail %d" % (
        name, note, plan["ok"], plan["fail"], plan["strips"], plan["cells"], plan["back"], att + " " if att else "",
        int(counters[4]), int(counters[0]), int(counters[5]), int(counters[6])))


def _check(name, oracle, plan, counters, note=""):
    _figures(name, oracle, plan, counters, note)
    assert int(counters[5]) == plan["ok"], (name, counters)
    assert int(counters[6]) == plan["fail"], (name, counters)
    if plan["back"] is None:
        assert int(counters[4]) == plan["cells"], (name, counters)            # the band throughout: exactly the windows' (and the strips') cells
    else:
        assert int(counters[4]) >= int(counters[0]), (name, counters)         # handed back: the full rows ran the whole pack again


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_pack_alone(gpu_ctx, oracle, capfd, monkeypatch, name):
    """One pack per call: its own counters, on the four-wavefront instance (one pack is far below four per CU)."""
    pack = CASES[name]["pack"]
    assert _group_of(pack, band=True) == (19 if CASES[name]["family"] == "score" else 16)
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, [pack], BAND)
    first = [d for d in lines if d["pass"] == 0]
    assert [d["variant"] for d in first] == [(4, 8, 4, 8)], lines
    plan = plan_of(oracle, name)
    assert (len(lines) > 1) == (plan["back"] is not None), lines                # a second pass iff the pack was handed back
    _check(name, oracle, plan, counters)


def test_constructed_packs_on_one_wavefront(gpu_ctx, oracle, capfd, monkeypatch):
    """All of them in one call among enough cheap band packs that every band group takes k_band1 (more than four packs per CU): the same
    rows, and the totals of the certified and failed counts are the model's sums plus the filler's own (from a run of the filler alone)."""
    filler = _cheap_band_packs(-(-33 * _device_cus() // 8))
    names = sorted(CASES)
    packs = filler + [CASES[n]["pack"] for n in names]
    assert len(set(map(tuple, packs))) == len(packs)
    alone, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, filler, BAND)
    assert all(d["variant"] == (4, 8, 1, 8) for d in lines if d["pass"] == 0), lines
    assert int(alone[5]) >= 1
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, BAND)
    first = [d for d in lines if d["pass"] == 0]
    assert {d["group"] for d in first} == {16, 19}
    for d in first:
        assert d["variant"] == (4, 8, 1, 8), d
    plans = [plan_of(oracle, n) for n in names]
    print("BANDCASE together: model ok %d fail %d + filler ok %d fail %d | device ok %d fail %d" % (
        sum(p["ok"] for p in plans), sum(p["fail"] for p in plans), int(alone[5]), int(alone[6]), int(counters[5]), int(counters[6])))
    assert int(counters[5]) == int(alone[5]) + sum(p["ok"] for p in plans), (counters, alone)
    assert int(counters[6]) == int(alone[6]) + sum(p["fail"] for p in plans), (counters, alone)


@pytest.mark.parametrize("debug", [8, 16])
@pytest.mark.parametrize("name", NO_BAND)
def test_without_a_band_under_strips_and_without_attempts(gpu_ctx, oracle, capfd, monkeypatch, name, debug):
    """RATTLE_POA_DEBUG=8: every alignment without a band runs the full rows as strips in place, nothing is handed back.  16: no band is
    attempted at all.  The rows are the oracle's either way (checked by _run); the counters are the model's under the same switch."""
    env = dict(BAND, RATTLE_POA_DEBUG=str(debug))
    counters, lines = _run(gpu_ctx, oracle, capfd, monkeypatch, [CASES[name]["pack"]], env)
    plan = plan_of(oracle, name, debug=debug)
    if debug == 16:
        assert int(counters[5]) == 0 and plan["ok"] == 0
    else:
        assert plan["back"] is None and plan["strips"] >= 1 and len(lines) == 1, (plan, lines)
    _check(name, oracle, plan, counters, " debug %d" % debug)
