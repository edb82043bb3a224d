"""Every pack of tests/constructed_bands.py sits on the comparison of the band's plan it is named after (no GPU: the oracle's graph,
columns and best score through Oracle.poa_band, and the plan model of constructed_bands).  tests/test_gpu_poa_band_edges.py runs the same
packs through kernel C; what is proved here is what makes its counter comparisons mean something: a pack moved one base off its edge
fails in here."""
import numpy as np
import pytest

import constructed_bands as cb
from test_band_lemma import best_cells, dag_dp

CASES = cb.cases()
_FACTS = {}


def facts_of(oracle, name):
    if name not in _FACTS:
        _FACTS[name] = oracle.poa_band(CASES[name]["pack"])
    return _FACTS[name]


def plan_of(oracle, name, debug=0):
    return cb.plan_pack(facts_of(oracle, name), debug)


def test_every_pack_is_a_band_pack():
    """3 - 12 sequences, and lengths that put the pack into a band group: at most 2560 nt, spread at most 400"""
    assert len(CASES) == 46
    for name, c in CASES.items():
        lens = [len(s) for s in c["pack"]]
        assert 3 <= len(lens) <= 12, name
        assert max(lens) - min(lens) <= 400, name
        assert max(lens) <= (2560 if c["family"] == "score" else 1024), name
        if c["family"] in ("right", "diag", "left", "history", "strips"):
            assert 300 <= min(lens) and max(lens) <= 700, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_columns_order_the_edges(oracle, name):
    facts = facts_of(oracle, name)
    assert len(facts) == len(CASES[name]["pack"]) - 1
    for k, f in enumerate(facts, 1):
        assert f["ordered"], (name, k)
        assert f["L"] == len(CASES[name]["pack"][k]) and len(f["cols"]) == f["n"] and f["C"] == int(f["cols"].max(initial=0)), (name, k)


EDGE = sorted(n for n, c in CASES.items() if c["family"] in ("right", "diag", "left"))


@pytest.mark.parametrize("name", EDGE)
def test_edge_alignment_has_the_constructed_score_and_diagonal(oracle, name):
    """S is exactly what the junk and the substitution leave; with that score the constructed run IS the optimal path, and it lies
    `offset` columns from the rows' columns: + t (the window's last column) for right / on, - s (its first) for left / on, one column
    inside for sub, one outside for off"""
    c = CASES[name]
    facts = facts_of(oracle, name)
    f = facts[c["edge"] - 1]
    N = len(c["base"])
    assert facts[0]["S"] == cb.MATCH * N and facts[0]["C"] == N
    assert (f["n"], f["C"], f["L"]) == (N, N, len(c["pack"][2]))
    assert list(f["cols"]) == list(range(1, N + 1))                     # a chain: row i lies in column i
    assert f["S"] == c["S"], (name, f["S"], c["S"])
    assert cb.width(f["C"], f["L"], c["cplb"]) == (c["t"], c["s"])
    # the constructed run: read column j faces graph column j - offset, and matches there (but for the one substitution)
    read, base, off = c["pack"][2], c["base"], c["offset"]
    run = [j for j in range(1, f["L"] + 1) if 1 <= j - off <= N and read[j - 1] == base[j - off - 1]]
    longest = max(len(list(g)) for g in np.split(np.array(run), np.nonzero(np.diff(run) != 1)[0] + 1))
    variant = name.rsplit("_", 1)[1]
    assert len(run) >= f["L"] - c["m"] - (variant == "sub")
    assert longest >= (f["L"] - c["m"]) // 2
    assert cb.MATCH * len(run) - (4 if variant == "sub" else 0) >= c["S"]          # nothing but this run can pay for S
    want = {"on": 0, "sub": -1, "off": 1}[variant]
    if c["family"] == "right":
        assert off - c["t"] == want
    if c["family"] == "left":
        assert -off - c["s"] == want
    # on the certificate's edge
    assert c["S"] - cb.threshold(f["L"], c["t"]) == {"on": 4, "sub": 0, "off": -1}[variant]


@pytest.mark.parametrize("name", EDGE)
def test_model_certifies_on_the_edge_and_fails_one_beyond(oracle, name):
    c = CASES[name]
    plan = plan_of(oracle, name)
    att = plan["alignments"][c["edge"] - 1]["attempts"]
    named = [a for a in att if a[0] == c["cplb"]]
    assert named == [(c["cplb"], c["t"], c["s"], c["certified_here"])], (name, att)
    assert [a[0] for a in att] == [x for x in cb.LADDER if x <= c["cplb"]] + ([2 * c["cplb"]] if not c["certified_here"] and c["cplb"] < 8 else [])
    assert [a[3] for a in att[:-1]] == [False] * (len(att) - 1)
    if c["certified_here"] or c["cplb"] < 8:
        assert att[-1][3] and plan["back"] is None and plan["ok"] == 2 and plan["fail"] == len(att) - 1
    else:
        assert plan["back"] == 2 and (plan["ok"], plan["fail"]) == (1, 3)          # nothing wider than 8 columns per lane
        strips = plan_of(oracle, name, debug=8)
        assert strips["back"] is None and (strips["ok"], strips["fail"], strips["strips"]) == (1, 3, 1)
    assert plan["cells"] == 2 * len(c["base"]) * 64 + sum(len(c["base"]) * 64 * a[0] for a in att)


def test_clamp_cases(oracle):
    for name, c in CASES.items():
        if c["family"] != "clamp":
            continue
        f = facts_of(oracle, name)[1]
        assert f["S"] == c["S"], name
        att = plan_of(oracle, name)["alignments"][1]["attempts"]
        last = att[-1]
        assert (last[1] == f["L"] - 1 and last[0] == 8) == c["clamped"], (name, att)
        if c["clamped"]:
            assert cb.threshold(f["L"], last[1]) == 1 and last[3] == (c["S"] > 0), (name, att)
            assert (63 * 8 - 1 - (f["C"] - f["L"])) >> 1 > f["L"] - 1               # the clamp binds
    assert [a[:2] for a in plan_of(oracle, "clamp_20")["alignments"][1]["attempts"]] == [(8, 19)]
    assert [a[:2] for a in plan_of(oracle, "clamp_62")["alignments"][1]["attempts"]] == [(8, 61)]
    assert [a[:2] for a in plan_of(oracle, "clamp_63")["alignments"][1]["attempts"]] == [(8, 62)]
    assert plan_of(oracle, "clamp_wide_62")["alignments"][1]["attempts"] == [(4, 6, 244, True)]
    assert plan_of(oracle, "clamp_wide_63")["alignments"][1]["attempts"] == [(4, 7, 244, True)]
    assert plan_of(oracle, "clamp_63_part")["alignments"][1]["attempts"] == [(4, 7, 244, False), (8, 62, 299, True)]
    junk = plan_of(oracle, "clamp_63_junk")
    assert junk["alignments"][1]["attempts"] == [(4, 7, 244, False), (8, 62, 299, False)] and junk["back"] == 2


def test_skip_cases(oracle):
    """e = 125 / 126 at two columns per lane, 251 / 252 at four: tau = L - t is C, then C + 1"""
    assert (cb.skip_edge(2), cb.skip_edge(4)) == (125, 251)
    for name, c in CASES.items():
        if c["family"] != "skip":
            continue
        f = facts_of(oracle, name)[0]
        assert (f["C"], f["L"], f["S"]) == (cb.SKIP_N, cb.SKIP_N + c["e"], c["S"]), name
        att = plan_of(oracle, name)["alignments"][0]["attempts"]
        assert len(att) == 1 and att[0][3], (name, att)
        assert att[0][0] == (c["cplb"] if c["tried"] else 2 * c["cplb"]), (name, att)
        if c["tried"]:
            assert f["L"] - att[0][1] == f["C"] and att[0][2] == 0          # tau == C: the window starts in the row's own column
        else:
            room = 63 * c["cplb"] - 1 - (f["C"] - f["L"])
            assert room >= 0 and f["L"] - (room >> 1) == f["C"] + 1         # skipped by C < L - t alone, one column short


def test_history_twins_differ_in_the_third_alignments_first_attempt(oracle):
    p29, p30 = plan_of(oracle, "history_29"), plan_of(oracle, "history_30")
    for h, p in ((29, p29), (30, p30)):
        facts = facts_of(oracle, "history_%d" % h)
        assert [f["S"] for f in facts] == CASES["history_%d" % h]["S"]
        assert (facts[2]["C"], facts[2]["L"]) == (cb.HIST_N, cb.HIST_N)
        assert (cb.MATCH * facts[1]["L"] - facts[1]["S"]) // cb.MATCH == h          # t_hist of the second alignment
        assert p["back"] is None and p["ok"] == 3 and p["fail"] == 0
    for k in (0, 1):
        a, b = p29["alignments"][k]["attempts"], p30["alignments"][k]["attempts"]
        assert [(x[0], x[1], x[3]) for x in a] == [(x[0], x[1], x[3]) for x in b] and len(a) == 1 and a[0][0] == 2
    assert p29["alignments"][2]["attempts"] == [(2, 62, 62, True)]                 # t_want = 62 <= t
    assert p30["alignments"][2]["attempts"] == [(4, 125, 125, True)]               # t_want = 64 > 62: the 2-column form is skipped
    assert p30["cells"] - p29["cells"] == facts_of(oracle, "history_30")[2]["n"] * 64 * 4 - facts_of(oracle, "history_29")[2]["n"] * 64 * 2 \
        + 64 * 2 * sum(facts_of(oracle, "history_30")[k]["n"] - facts_of(oracle, "history_29")[k]["n"] for k in (0, 1))


def test_strips_cases_land_on_the_predicted_side(oracle):
    for name, c in CASES.items():
        if c["family"] != "strips":
            continue
        p = plan_of(oracle, name)
        assert (p["back"], p["strips"]) == (c["back"], c["strips"]), (name, p["back"], p["strips"])
        hows = [a["how"] for a in p["alignments"]]
        assert hows[:7] == ["band"] * 7, name
        assert p_ok_before_first_failure(p) == (7 if name == "strips_8th" else 8), name
        under8 = plan_of(oracle, name, debug=8)
        assert under8["back"] is None and under8["strips"] == sum(len(s) == 300 for s in c["pack"])
        under16 = plan_of(oracle, name, debug=16)
        assert under16["ok"] == 0 and under16["fail"] == 0 and under16["back"] == 1
    # the three-quarters rule, on both sides: 8 certified, the 10th alignment keeps it, the 11th does not
    assert 4 * 8 >= 3 * 10 and 4 * 8 < 3 * 11


def p_ok_before_first_failure(plan):
    n = 0
    for a in plan["alignments"]:
        if a["how"] != "band":
            break
        n += 1
    return n


def test_score_cases(oracle):
    for name in ("score_12800", "score_last_column"):
        facts = facts_of(oracle, name)
        assert [f["S"] for f in facts] == CASES[name]["S"]
        p = plan_of(oracle, name)
        assert [a["attempts"] for a in p["alignments"]] == [[(2, 62, 62, True)]] * 2


def _chain(base):
    return [{"letter": int(x), "preds": [i] if i else [], "col": i + 1} for i, x in enumerate(base)]


@pytest.mark.parametrize("family", ["right", "left"])
def test_a_window_one_column_short_loses_the_small_edge_case(family):
    """The right / left `on` cases in small (64 columns, t = 8), in plain Python matrices as in test_band_lemma.py: the window as planned
    gives the full matrices' best score and best cells; one column narrower on the side the path touches, the best score is lower -- a
    kernel whose window is one column short there would change these packs' rows."""
    base, read, C, L, t, s = cb.small_edge(family)
    rows, b = _chain(base), [int(x) for x in read]
    full = best_cells(dag_dp(rows, b)[0])
    assert full[0] == cb.MATCH * (L - t) >= cb.threshold(L, t)
    band = lambda lo_cut, hi_cut: (lambda i: (max(1, rows[i - 1]["col"] - s + lo_cut), min(L, rows[i - 1]["col"] + t - hi_cut)))
    assert best_cells(dag_dp(rows, b, band(0, 0))[0]) == full
    short = best_cells(dag_dp(rows, b, band(0, 1) if family == "right" else band(1, 0))[0])
    assert short[0] < full[0]
    other = best_cells(dag_dp(rows, b, band(1, 0) if family == "right" else band(0, 1))[0])
    assert other == full                                   # (the side the path does not touch may lose a column)
