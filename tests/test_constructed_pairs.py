"""The constructed pairs of tests/constructed.py are what they claim to be -- on the CPU oracle alone, no GPU.  The GPU tests of
kernel B (tests/test_gpu_pair_score_edges.py) run the same pairs; what is proven here is that each of them sits on the edge of
pair_score.hip it is named after: the exact match count at PS_MCAP = 400 and at bcap = 2048, the length of the LIS, the number of
kept chain elements, the NaN variance of a single distance, which walk runs."""
import bisect
import math

import numpy as np
import pytest

import constructed as cs


def match_list(oracle, c, k):
    """get_common_kmers from the oracle's own lists: the (pos1, pos2) pairs in the reference's order"""
    fh, fp, _, _, _, _ = oracle.extract_kmers(c.a, k, False)
    ex = oracle.extract_kmers(c.b, k, True)
    bh, bp = (ex[2], ex[3]) if c.strand else (ex[0], ex[1])
    lo, hi = np.searchsorted(bh, fh, "left"), np.searchsorted(bh, fh, "right")
    return sorted((int(fp[i]), int(bp[j])) for i in range(len(fh)) for j in range(lo[i], hi[i]))


def lis_length(pos2):
    """strictly increasing, as similarity.cpp:10-31"""
    tails = []
    for x in pos2:
        at = bisect.bisect_left(tails, x)
        tails[at:at + 1] = [x]
    return len(tails)


def check_claims(oracle, c, k):
    bases, hc, nd, var, nm, _ = oracle.pair_score(c.a, c.b, k, c.strand, dist_cap=1)
    cl = c.claims
    ml = match_list(oracle, c, k)
    assert len(ml) == nm, c
    lis = lis_length([m[1] for m in ml])
    if "n_matches" in cl:
        assert nm == cl["n_matches"], (c, nm)
    if "min_matches" in cl:
        assert nm >= cl["min_matches"], (c, nm)
    if "lis" in cl:
        assert lis == cl["lis"], (c, lis)
        if cl["lis"] == 1:
            assert (bases, nd) == (k, 0), c                 # `reversed`: one chain element, no distance
    if "nd" in cl:
        assert nd == cl["nd"], (c, nd)
    if cl.get("nd_below_lis"):
        assert nd + 1 < lis, (c, nd, lis)                   # a chain element that is not kept
    if cl.get("searched_beyond_chain"):
        assert nd + 1 < nm, (c, nd, nm)
    if cl.get("nan_var"):
        assert nd == 1 and math.isnan(var), (c, nd, var)
    if cl.get("hc_below_bases"):
        assert 0 < hc < bases and var > 25.0, (c, hc, bases, var)
    if "swapped" in cl:
        assert cs.is_swapped(c.a, c.b, k) == cl["swapped"], c
    n_a, n_b = len(c.a) - k, len(c.b) - k
    if "n_searched" in cl:
        assert (n_a if cl.get("swapped") else n_b) == cl["n_searched"], c
    if "n_walked" in cl:
        assert (n_b if cl.get("swapped") else n_a) == cl["n_walked"], c
    return nm, lis, nd


@pytest.mark.parametrize("k", [10, 11, 16])
def test_every_case_is_what_it_claims(oracle, k):
    names = set()
    stats = {}
    for c in cs.cases(k):
        assert c.name not in names
        names.add(c.name)
        stats[c.name] = check_claims(oracle, c, k)
    # the edges every k must reach (kernel B, pair_score.hip): 400 / 401 matches in the plain and in the swapped shape, on both
    # strands; the searched list on both sides of 2048; the walked list on every side of 512 and 1024; the swap threshold
    for la in (700, 3000):
        for rc in ("", "-rc"):
            assert [stats[f"k{k}-fragment-{la}-{m}{rc}"][0] for m in (399, 400, 401)] == [399, 400, 401]
    assert {c.claims["n_searched"] for c in cs.cases(k) if "searched-" in c.name} == {2047, 2048, 2049}
    assert {c.claims["n_walked"] for c in cs.cases(k) if "walked-" in c.name} == {511, 512, 513, 1023, 1024, 1025}
    for c in cs.cases(k):
        if c.name.endswith("-200") or "walked-" in c.name:
            assert stats[c.name][0] <= 400, c               # the full pass in LDS runs on them, not the oversize relaunch
    at, above = (next(c for c in cs.cases(k) if c.name == f"k{k}-swap-threshold-{w}") for w in ("at", "above"))
    assert len(at.a) - k == 4 * (len(at.b) - k) + 256 and len(above.a) - k == 4 * (len(above.b) - k) + 257


def test_exact_core_cases_at_k16(oracle):
    """the figures the generators were designed to: one match per core, LIS 1 / n / about 2 sqrt(n), the tail search of two_track
    running past 64 and 128 tails"""
    by_name = {c.name: c for c in cs.cases(16)}
    for n in cs.CORE_N:
        for order, lis in (("reversed", 1), ("identity", n)):
            nm, got, nd = check_claims(oracle, by_name[f"k16-{order}-{n}"], 16)
            assert (nm, got, nd) == (n, lis, lis - 1)
        nm, got, nd = check_claims(oracle, by_name[f"k16-random-{n}"], 16)
        assert nm == n and (n < 63 or math.sqrt(n) < got < 3 * math.sqrt(n)), (n, got)
    assert check_claims(oracle, by_name["k16-two-track-300"], 16) == (300, 150, 149)
    for r in (63, 64, 65):
        assert check_claims(oracle, by_name[f"k16-sawtooth-{r}"], 16) == (4 * r, r, r - 1)
    for n in cs.CHAIN_N:
        c = by_name[f"k16-chain-{n}"]
        d = oracle.pair_score(c.a, c.b, 16, 0, dist_cap=1024)[5]
        assert np.array_equal(d, cs.walk_gaps(n)[1:] - 1)     # the walk's distances are the gap-length differences
    for at in cs.SPLIT_AT:
        c = by_name[f"k16-split-{at}"]
        ml = match_list(oracle, c, 16)
        assert ml[at][0] - ml[at - 1][0] == 1 and ml[at][1] - ml[at - 1][1] >= 16      # chain element `at`: d1 < k, d2 >= k


def test_k5_core_cases_have_matches_everywhere(oracle):
    """below k = 6 the 6-mer prefilter of the walk is off and 5-nt cores match all over: no claim but that, and that the big
    ones go past the LDS capacity"""
    big = 0
    for c in cs.cases(5):
        assert not c.claims
        nm = oracle.pair_score(c.a, c.b, 5, c.strand, dist_cap=1)[4]
        big += nm > 400
    assert big >= 10 and not [c for c in cs.cases(5) if "fragment" in c.name]


def test_count_cases_and_the_folded_count(oracle):
    """The pairs that go through the count form.  The per-pair search counts |common| itself.  The seed-major pass (pair_count.hip)
    counts over hashes folded to 20 bits for k > 10: an upper bound of |common| by design, equal to it when no two different k-mers of
    the pair fold together.  The fragment pairs are generated free of such collisions; the `reversed` pairs (6 800 k-mers a read: some
    40 collisions expected) cannot be, so their seed-major count is held to the folded count.  The fold of constructed.n_common is
    checked here on the oracle's own hashes."""
    cc = cs.count_cases()
    assert sorted(c.claims["n_matches"] for c in cc) == [399] * 3 + [400] * 3 + [401] * 3
    for c in cc:
        fa = oracle.extract_kmers(c.a, 16, False)[0].astype(np.int64)
        fb = oracle.extract_kmers(c.b, 16, False)[0].astype(np.int64)
        va, ca = np.unique(cs.fold20(fa), return_counts=True)
        assert len(fa) - len(va) <= 2048                    # PC_REP: the repeat list of the seed does not overflow
        vb, cb = np.unique(cs.fold20(fb), return_counts=True)
        _, ia, ib = np.intersect1d(va, vb, return_indices=True)
        folded = int((ca[ia] * cb[ib]).sum())
        nm = oracle.pair_score(c.a, c.b, 16, 0, dist_cap=1)[4]
        assert folded == cs.n_common(c.a, c.b, 16, 0, True) and nm == cs.n_common(c.a, c.b, 16) == c.claims["n_matches"], c
        assert folded == nm if "fragment" in c.name else folded >= nm, (c, folded, nm)
