"""The abundance rule without a device: its two statements in tests/abundance_ref.py (plain Python ints; numpy on uint64) agree bit for
bit, and the rule does what its description says -- the worked example, the exact mass after every iteration, the symmetry of targets
that always come together, the compatibility edge, the stop rule."""
import numpy as np
import pytest

import abundance_ref as ref

ONE = ref.ONE


def hand(rows, k):
    """rows: per read a list of (target, score), best first"""
    n = len(rows)
    c = {"count": np.array([len(r) for r in rows], np.uint32), "target": np.full((n, k), -1, np.int32), "score": np.full((n, k), -1.0)}
    for i, r in enumerate(rows):
        for j, (t, s) in enumerate(r):
            c["target"][i, j] = t
            c["score"][i, j] = s
    return c


def example():
    """3 reads unique to A, 1 unique to B, 4 on {A, B}: the fixed point is 6 / 2"""
    return hand([[(0, 0.8)]] * 3 + [[(1, 0.8)]] + [[(0, 0.8), (1, 0.8)]] * 4, 2)


@pytest.mark.parametrize("n,k,nt,seed", [(1, 1, 1, 0), (40, 2, 9, 1), (200, 8, 40, 2), (150, 3, 17, 3), (64, 8, 8, 4)])
def test_the_two_forms_agree_bit_for_bit(n, k, nt, seed):
    rng = np.random.default_rng(seed)
    cands = ref.lists(n, k, nt, rng, empty=0.1)
    for tol, iters in ((1e-3, 60), (0.0, 7), (0.5, 1000)):
        a, b = ref.scalar(cands, nt, 0.95, tol, iters), ref.vector(cands, nt, 0.95, tol, iters)
        assert ref.same(a, b) is None, ref.same(a, b)


def test_the_two_forms_agree_on_lists_no_assignment_would_make():
    """unsorted scores, a target twice in one read, a negative best score, reads without a candidate, and none at all"""
    rng = np.random.default_rng(9)
    n, k, nt = 90, 4, 6
    cands = {"count": rng.integers(0, k + 1, n).astype(np.uint32), "target": rng.integers(0, nt, (n, k)).astype(np.int32),
             "score": rng.uniform(-0.2, 1.0, (n, k))}
    a, b = ref.scalar(cands, nt, 0.9, 1e-3, 50), ref.vector(cands, nt, 0.9, 1e-3, 50)
    assert ref.same(a, b) is None, ref.same(a, b)
    assert a["compatible_reads"].max() <= n
    none = {"count": np.zeros(5, np.uint32), "target": np.full((5, 2), -1, np.int32), "score": np.full((5, 2), -1.0)}
    a, b = ref.scalar(none, 3), ref.vector(none, 3)
    assert ref.same(a, b) is None and a["n_placed"] == 0 and a["iterations"] == 1 and a["converged"] == 1 and not a["units"].any() and not a["cpm"].any()
    for f in (ref.scalar, ref.vector):
        e = f(hand([], 3), 4)
        assert e["iterations"] == 0 and e["converged"] == 1 and e["units"].tolist() == [0] * 4 and e["posterior"].shape == (0, 3)
        e = f(none, 0)
        assert e["iterations"] == 0 and e["converged"] == 1 and len(e["units"]) == 0


def agree(cands, nt, label, **kw):
    a, b = ref.scalar(cands, nt, **kw), ref.vector(cands, nt, **kw)
    assert ref.same(a, b) is None, (label, ref.same(a, b))
    assert int(a["units"].sum()) == a["n_placed"] * ONE, label
    return a


@pytest.mark.parametrize("nt,empties,unnamed",
                         [(nt, e, None) for nt in ref.SCAN_NT for e in (False, True)] + [(nt, True, u) for nt, u in ref.SCAN_UNNAMED])
def test_scan_rounds_case_names_targets_on_both_sides_of_every_round_edge(nt, empties, unnamed):
    cands = ref.scan_rounds_case(nt, empties, unnamed)
    assert ref.scan_rounds_holds(cands, nt, empties, unnamed)
    assert not ref.scan_rounds_holds(cands, nt, not empties, unnamed)
    t0 = ref.slot0(cands)
    assert 600 < len(t0) <= 700 == len(cands["count"]) and cands["target"].shape == (700, 4) and t0.max() == nt - 1
    for first in range(0, nt, ref.SCAN):                                 # every round the scan takes over the targets holds reads
        assert ((t0 >= first) & (t0 < first + ref.SCAN)).any()
    if unnamed is not None:
        assert ref.scan_rounds_holds(ref.scan_rounds_case(nt, empties), nt, empties) and (ref.scan_rounds_case(nt, empties)["target"] == unnamed).any()
    r = agree(cands, nt, "scan rounds", max_iters=12)
    assert r["n_placed"] == len(t0) and (unnamed is None or r["units"][unnamed] == 0)


def test_leftover_and_spread_cases_hold_more_than_eight_distinct_targets_where_they_say():
    for distinct in (9, 8):
        cands = ref.leftover_case(distinct)
        assert ref.leftover_holds(cands, distinct) and not ref.leftover_holds(cands, 17 - distinct)
        assert np.bincount(cands["target"][:64, 1][cands["target"][:64, 1] >= 0]).tolist()[1:] == ([7] * 9 if distinct == 9 else [8] * 7 + [7])
        r = agree(cands, ref.LEFTOVER_NT, "leftover")
        assert r["converged"] == 1 and r["n_placed"] == 94
    for alone_every in (0, 5):
        cands = ref.spread_case(alone_every)
        assert ref.spread_holds(cands, alone_every) and not ref.spread_holds(cands, 5 - alone_every)
        target = cands["target"]
        for j in range(1, 8):
            assert np.bincount(target[:, j][target[:, j] >= 0]).max() <= 7
        assert all(len(set(row[row >= 0])) == (row >= 0).sum() for row in target)         # a read names a target once
        assert (target[::5, 1:] < 0).all() == bool(alone_every) and target.max() == 300
        agree(cands, ref.SPREAD_NT, "spread", max_iters=60)


def test_the_cases_of_whole_empty_wavefronts():
    cands, nt = ref.empty_wavefront_case()
    assert ref.empty_wavefronts(cands) == 2 and (cands["count"] > 0).sum() == 100 and len(cands["count"]) == 300
    r = agree(cands, nt, "empties", max_iters=60)
    assert r["iterations"] > 3 and r["n_placed"] == 100
    cands, nt = ref.run_to_the_edge_case()
    t0 = ref.slot0(cands)
    assert ref.empty_wavefronts(cands) == 1 and np.bincount(t0).tolist() == [62, 130] and (62 + 130) % ref.WAVE == 0
    r = agree(cands, nt, "run to the edge", max_iters=60)
    assert r["iterations"] > 3 and r["n_placed"] == 192


def test_the_odd_lists_hold_a_target_twice_a_hole_and_a_negative_best_score():
    for k in (4, 8):
        cands = ref.odd_lists(k)
        assert ref.odd_holds(cands) == (True, True, True)
        agree(cands, ref.ODD_NT, "odd lists", ratio=ref.ODD_RATIO, max_iters=50)
    assert ref.odd_holds(ref.lists(200, 8, 40, np.random.default_rng(2))) == (False, False, False)
    cands = ref.odd_hand()
    assert ref.odd_holds(cands) == (True, True, False)
    r = agree(cands, ref.ODD_NT, "odd lists by hand", ratio=ref.ODD_RATIO, max_iters=50)
    assert r["compatible_reads"].tolist() == ref.ODD_HAND_COMPATIBLE == [1, 1, 1, 1, 0, 1]
    assert r["units"].tolist()[2] == ONE and r["units"][1] + r["units"][3] == ONE and r["units"][0] + r["units"][5] == ONE


def test_beyond_2_53_case_is_what_it_says_without_running_it():
    """(the run itself takes the vector form two seconds: tests/test_gpu_abundance_edges.py makes it, once per variant)"""
    for handing_over in (0, 10):
        cands = ref.beyond_2_53_case(handing_over)
        assert len(cands["count"]) == ref.BEYOND_N + handing_over and ref.BEYOND_N * ONE > 2 ** 53 >= (1 << 21) * ONE
        assert (cands["count"] == 2).sum() == 3000 + handing_over and (cands["target"][:ref.BEYOND_N, 0] == 0).all()
        assert cands["target"][ref.BEYOND_N:].tolist() == [[1, 0]] * handing_over


def test_the_worked_example_converges_to_six_and_two():
    r = ref.scalar(example(), 2)
    assert r["converged"] == 1 and r["iterations"] == 10 and r["n_placed"] == 8
    assert abs(r["est_reads"][0] - 6.0) <= 1e-3 and abs(r["est_reads"][1] - 2.0) <= 1e-3          # within tol
    assert int(r["units"].sum()) == 8 * ONE
    assert r["compatible_reads"].tolist() == [7, 5]
    assert r["cpm"].tolist() == [float(u) / float(8 * ONE) * 1e6 for u in r["units"].tolist()]
    # a shared read's posterior is the share of its two targets, a unique read's is 1
    assert r["posterior"][0].tolist() == [1.0, 0.0] and r["posterior"][3].tolist() == [1.0, 0.0]
    p = r["posterior"][4]
    assert p[0] + p[1] == 1.0 and abs(p[0] - 0.75) < 1e-3


def test_the_mass_is_exact_after_every_iteration():
    rng = np.random.default_rng(5)
    cands = ref.lists(300, 8, 40, rng, empty=0.05)
    states = []
    r = ref.scalar(cands, 40, 0.95, 0.0, 40, states)
    assert len(states) == r["iterations"] == 40 and r["converged"] == 0
    for A in states:
        assert sum(A) == r["n_placed"] * ONE
    assert int(r["units"].sum()) == r["n_placed"] * ONE
    assert np.allclose(r["posterior"].sum(1)[cands["count"] > 0], 1.0, rtol=0, atol=2 ** -31)


def test_two_targets_that_always_come_together_stay_equal():
    """targets 1 and 2 occur only side by side, in slots 1 and 2 behind target 0: equal at the start and after every iteration"""
    rows = [[(0, 0.9), (1, 0.9), (2, 0.9)]] * 5 + [[(0, 0.9)]] * 2 + [[(3, 0.9), (1, 0.9), (2, 0.9)]] * 3
    states = []
    r = ref.scalar(hand(rows, 3), 4, 0.95, 0.0, 25, states)
    assert all(A[1] == A[2] for A in states) and r["units"][1] == r["units"][2] > 0


def test_a_slot_at_exactly_the_ratio_is_in_and_one_ulp_below_is_out():
    top, ratio = 0.7, 0.95
    edge = ratio * top
    below = np.nextafter(edge, 0.0)
    inside = hand([[(0, top), (1, edge)]], 2)
    outside = hand([[(0, top), (1, below)]], 2)
    assert ref.compatible(inside, ratio).tolist() == [[True, True]] and ref.compatible(outside, ratio).tolist() == [[True, False]]
    for f in (ref.scalar, ref.vector):
        assert f(inside, 2, ratio)["compatible_reads"].tolist() == [1, 1] and f(inside, 2, ratio)["units"].tolist() == [ONE // 2, ONE // 2]
        assert f(outside, 2, ratio)["compatible_reads"].tolist() == [1, 0] and f(outside, 2, ratio)["units"].tolist() == [ONE, 0]


def test_the_stop_rule():
    c = example()
    full = ref.scalar(c, 2, 0.95, 1e-3, 1000)
    lim = ref.tol_units(1e-3)
    assert lim == int(1e-3 * 4294967296.0) == 4294967
    d = full["delta"].tolist()
    assert len(d) == full["iterations"] and d[-1] <= lim and all(x > lim for x in d[:-1])
    # delta is the largest move of the iteration: recomputed from the states
    states = []
    ref.scalar(c, 2, 0.95, 1e-3, 1000, states)
    start = [3 * ONE + 4 * (ONE - ONE // 2), ONE + 4 * (ONE // 2)]
    for i, A in enumerate(states):
        before = start if i == 0 else states[i - 1]
        assert d[i] == max(abs(x - y) for x, y in zip(A, before))
    # tol 0 with a small max_iters: not converged, max_iters iterations, and a prefix of the longer run
    short = ref.scalar(c, 2, 0.95, 0.0, 5)
    assert short["converged"] == 0 and short["iterations"] == 5 and short["delta"].tolist() == d[:5]
    assert ref.same(short, ref.vector(c, 2, 0.95, 0.0, 5)) is None
    # a looser tolerance stops earlier on the same path
    loose = ref.scalar(c, 2, 0.95, 0.1, 1000)
    assert loose["converged"] == 1 and loose["delta"].tolist() == d[:loose["iterations"]] and loose["iterations"] < full["iterations"]
