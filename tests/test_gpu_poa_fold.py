"""poa_run::fold_classes: a barrier-form class that fills the device with fewer workgroups per CU than the next wider one hands all its
packs to it (stage 1 of `correct`: the 1024-column packs ride the 1536-column instance, eight workgroups per CU instead of seven).

The rule is read from the RATTLE_TIMING lines (`group G pk K`, `N blocks/CU`, and `, N folded from the 1024 cols class` behind them on
the line of the group that took packs in); every run is compared with the oracle byte for byte and with the same call under
RATTLE_POA_FOLD=0.  RATTLE_POA_FOLD=1 folds whatever the numbers of packs; RATTLE_POA_MODE=dense keeps the instances independent of the
device's size."""
import re

import numpy as np
import pytest

from test_gpu_poa_variants import _device_cus, _edge_pack, _group_of, _lines, _noisy, _random_seq, _want

pytestmark = pytest.mark.gpu

_FOLDED = re.compile(r"(\d+) cols \([^\n]*?(\d+) blocks/CU, group (\d+) pk (\d+)[^\n,]*, (\d+) folded from the (\d+) cols class")
_BPC = re.compile(r"(\d+) blocks/CU, group (\d+) pk ")
_SWITCHES = ("RATTLE_POA_MODE", "RATTLE_POA_FOLD", "RATTLE_POA_NODE_CAP", "RATTLE_POA_BUDGET_MB")


def _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env):
    """one call of the MSA entry under exactly the switches of `env`; every pack == the oracle; -> rows, widths, timing lines, folds"""
    monkeypatch.setenv("RATTLE_TIMING", "1")
    for k in _SWITCHES:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    capfd.readouterr()
    rows, width, counters = gpu_ctx.poa_msa(packs)
    err = capfd.readouterr().err
    cells = 0
    for p, pack in enumerate(packs):
        want, c = _want(oracle, pack)
        cells += c
        assert width[p] == len(want[0]), p
        assert rows[p] == want, p
    assert int(counters[0]) == cells
    lines = _lines(err)
    assert lines, err[-2000:]
    # (cols of the group that took packs in, its blocks/CU, group, packs folded, cols of the class they came from)
    folds = [(int(m[1]), int(m[2]), int(m[3]), int(m[5]), int(m[6])) for m in _FOLDED.finditer(err)]
    bpc = {int(m[2]): int(m[1]) for m in _BPC.finditer(err)}
    return rows, list(width), lines, folds, bpc


def _noisy_pack(L, depth=6, err=0.10, seed=0):
    """`depth` reads at `err` total error of one random template, the longest exactly L nt (the template itself, first)"""
    rng = np.random.default_rng(L * 13 + seed)
    base = _random_seq(rng, L)
    return [base.tobytes()] + [_noisy(rng, base, err)[:L].tobytes() for _ in range(depth - 1)]


def _small_packs():
    """longest reads of about 300 and 700, exactly 1024 (the narrow class's last column) and 1025 nt, and one pack near 1400"""
    packs = [_noisy_pack(L) for L in (300, 700, 1024, 1025, 1400)]
    assert [_group_of(p) for p in packs] == [0, 0, 0, 1, 1]
    assert [max(map(len, p)) for p in packs] == [300, 700, 1024, 1025, 1400]
    return packs


def test_forced_fold_small(gpu_ctx, oracle, capfd, monkeypatch):
    """RATTLE_POA_FOLD=1: three packs of the 1024-column class (one at its last column) run in the 1536-column instance beside two of its
    own: one group, no 1024-column line, the folded count on the line, and the MSA of the oracle and of the unfolded run"""
    packs = _small_packs()
    rows0, width0, lines0, folds0, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {"RATTLE_POA_MODE": "dense", "RATTLE_POA_FOLD": "0"})
    assert [(d["group"], d["cols"], d["packs"]) for d in lines0] == [(0, 1024, 3), (1, 1536, 2)] and not folds0, lines0
    rows1, width1, lines1, folds1, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {"RATTLE_POA_MODE": "dense", "RATTLE_POA_FOLD": "1"})
    assert rows1 == rows0 and width1 == width0
    assert [(d["group"], d["cols"], d["packs"], d["variant"]) for d in lines1] == [(1, 1536, 5, (6, 4, 4, 1))], lines1
    assert [(f[0], f[2], f[3], f[4]) for f in folds1] == [(1536, 1, 3, 1024)], folds1


def _tiny_pack(L, i):
    rng = np.random.default_rng(1000 * L + i)
    a = _random_seq(rng, L)
    b = a.copy()
    b[L // 2] = a[L // 2] ^ 6 if a[L // 2] in (65, 71) else a[L // 2]      # (A <-> G; C and T stay: some packs are two equal reads)
    return [a.tobytes(), b.tobytes()]


def test_rule_fires_at_its_edge(gpu_ctx, oracle, capfd, monkeypatch):
    """Nothing forced but the form: places + 1 packs in each of the two classes (two reads of 64 nt; two reads of 1030 nt) fold, with
    exactly `places` packs in the narrow class they do not.  places = CUs x blocks/CU of each instance in the unfolded run."""
    n_cu = _device_cus()
    narrow = [_tiny_pack(64, i) for i in range(4)]
    wide = [_tiny_pack(1030, i) for i in range(4)]
    env = {"RATTLE_POA_MODE": "dense"}
    probe = [narrow[0], wide[0]]
    *_, bpc = _run(gpu_ctx, oracle, capfd, monkeypatch, probe, dict(env, RATTLE_POA_FOLD="0"))
    p0, p1 = n_cu * bpc[0], n_cu * bpc[1]
    assert bpc[0] < bpc[1], bpc                  # (seven against eight: the premise of the rule on this device)

    def packs_of(n0, n1):
        return [narrow[i % 4] for i in range(n0)] + [wide[i % 4] for i in range(n1)]

    packs = packs_of(p0 + 1, p1 + 1)
    rows0, width0, lines0, folds0, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, dict(env, RATTLE_POA_FOLD="0"))
    assert [(d["group"], d["packs"], d["n_slots"]) for d in lines0] == [(0, p0 + 1, p0), (1, p1 + 1, p1)] and not folds0, lines0
    rows1, width1, lines1, folds1, bpc1 = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
    assert rows1 == rows0 and width1 == width0
    assert [(d["group"], d["packs"], d["n_slots"]) for d in lines1] == [(1, p0 + p1 + 2, p1)], lines1
    assert folds1 == [(1536, bpc[1], 1, p0 + 1, 1024)] and bpc1 == {1: bpc[1]}, (folds1, bpc1)
    # one pack fewer in the narrow class: it has a place for every pack, and keeps them
    packs = packs_of(p0, p1 + 1)
    _, _, lines2, folds2, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, env)
    assert [(d["group"], d["packs"], d["n_slots"]) for d in lines2] == [(0, p0, p0), (1, p1 + 1, p1)] and not folds2, lines2


def test_rule_stays_out_of_small_jobs(gpu_ctx, oracle, capfd, monkeypatch):
    """default environment, two dozen packs across both classes: the groups and instances of RATTLE_POA_FOLD=0"""
    packs = [_edge_pack(500 + 40 * i, 3, seed=i) for i in range(12)] + [_edge_pack(1050 + 40 * i, 3, seed=i) for i in range(12)]
    assert [_group_of(p) for p in packs] == [0] * 12 + [1] * 12
    rows0, width0, lines0, folds0, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {"RATTLE_POA_FOLD": "0"})
    rows1, width1, lines1, folds1, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, {})
    key = lambda lines: [(d["group"], d["variant"], d["pass"], d["packs"], d["n_slots"]) for d in lines]
    assert key(lines1) == key(lines0) and {d["group"] for d in lines1} == {0, 1} and not folds0 and not folds1, (lines0, lines1)
    assert rows1 == rows0 and width1 == width0


def test_retry_inside_a_folded_group(gpu_ctx, oracle, capfd, monkeypatch):
    """forced fold with a first-pass node capacity below the MSA width of the folded 700- and 1024-nt packs: they outgrow their slots in
    the wide group and run again there with four times the nodes; the result is the oracle's and the unfolded run's"""
    packs = _small_packs()
    cap = 640
    must_retry = [p for p, pack in enumerate(packs) if len(_want(oracle, pack)[0][0]) > cap]      # (a graph has a node per MSA column at least)
    assert {1, 2} <= set(must_retry) and len(_want(oracle, packs[0])[0][0]) < cap
    env = {"RATTLE_POA_MODE": "dense", "RATTLE_POA_NODE_CAP": str(cap)}
    rows0, width0, lines0, _, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, dict(env, RATTLE_POA_FOLD="0"))
    assert {d["group"] for d in lines0} == {0, 1}
    rows1, width1, lines1, folds1, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, dict(env, RATTLE_POA_FOLD="1"))
    assert rows1 == rows0 and width1 == width0
    assert {d["group"] for d in lines1} == {1}, lines1
    assert [(f[2], f[3]) for f in folds1] == [(1, 3)], folds1          # said once, on the pass that took them in
    by_pass = {d["pass"]: d["packs"] for d in lines1}
    assert by_pass[0] == 5 and by_pass.get(1, 0) >= len(must_retry), lines1


def test_budget_guard(gpu_ctx, oracle, capfd, monkeypatch):
    """forced fold under an arena budget that holds a slot per pack as the groups stand but not five slots of the wide group: no fold"""
    packs = _small_packs()
    env = {"RATTLE_POA_MODE": "dense"}
    rows0, width0, lines0, _, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, dict(env, RATTLE_POA_FOLD="0"))
    assert [(d["group"], d["pass"], d["n_slots"]) for d in lines0] == [(0, 0, 3), (1, 0, 2)], lines0
    mb = {d["group"]: d["mb"] for d in lines0}
    eps = 0.05e6                                                   # what %.1f MB may hide of one slot
    unfolded = 3 * (mb[0] * 1e6 + eps) + 2 * (mb[1] * 1e6 + eps)
    budget_mb = (int(unfolded) >> 20) + 1
    assert unfolded <= budget_mb << 20 < 5 * (mb[1] * 1e6 - eps), (budget_mb, mb)
    env["RATTLE_POA_BUDGET_MB"] = str(budget_mb)
    rows1, width1, lines1, folds1, _ = _run(gpu_ctx, oracle, capfd, monkeypatch, packs, dict(env, RATTLE_POA_FOLD="1"))
    assert rows1 == rows0 and width1 == width0
    key = lambda lines: [(d["group"], d["pass"], d["packs"], d["n_slots"], d["mb"]) for d in lines]
    assert key(lines1) == key(lines0) and not folds1, (lines1, folds1)
