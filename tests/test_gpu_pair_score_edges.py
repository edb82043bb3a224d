"""Kernel B (pair_score.hip) on pairs constructed to sit on its edges, against the oracle through rattle_hip_pair_score and, for the
count form, rattle_hip_debug_evaluate.  Everything in the kernel advances 64 elements per ballot and lives in arrays of a fixed
capacity; the pairs of tests/constructed.py pin one case to each side of every such edge (tests/test_constructed_pairs.py proves on
the CPU that they do).  Bit-exact: integers, and the double variance by bits with NaN equal to NaN."""
import numpy as np
import pytest

import constructed as cs

pytestmark = pytest.mark.gpu


def _same_float(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


_scored = {}


def _score_all(gpu_ctx, oracle, k, want):
    """All cases of one k in ONE load (both strands) and ONE pair_score call, each as (a, b, strand) as built, on the other strand,
    and with the two reads exchanged; made once per k and shared.  The cases selected by `want` are compared with the oracle here;
    returns per such case the oracle's answer of the pair as built."""
    if k not in _scored:
        reads, ii, jj, ss = [], [], [], []
        for c in cs.cases(k):
            ia = len(reads)
            reads += [c.a, c.b]
            ii += [ia, ia, ia + 1]; jj += [ia + 1, ia + 1, ia]; ss += [c.strand, 1 - c.strand, c.strand]
        gpu_ctx.load_reads(reads, k, True)
        _scored[k] = (reads, ii, jj, ss, gpu_ctx.pair_score(ii, jj, ss))
    reads, ii, jj, ss, (bases, hc, nd, var, nm) = _scored[k]
    out = {}
    for t in range(len(ii)):
        c = cs.cases(k)[t // 3]
        if not want(c):
            continue
        b, h, n, v, m, _ = oracle.pair_score(reads[ii[t]], reads[jj[t]], k, int(ss[t]), dist_cap=1)
        label = (c.name, ("as built", "other strand", "exchanged")[t % 3])
        assert (bases[t], nd[t], nm[t]) == (b, n, m), (label, (bases[t], nd[t], nm[t]), (b, n, m))
        if m > 0:
            assert hc[t] == h, (label, hc[t], h)
        assert _same_float(var[t], v), (label, var[t], v)
        if t % 3 == 0:
            out[c.name] = (b, h, n, v, m)
    return out


@pytest.mark.parametrize("k", [5, 10, 11, 16])
def test_core_pairs_lis_and_walk_edges(gpu_ctx, oracle, k):
    """Stage 2 of pair_score_kernel on core / separator pairs, whose match list is one match per core in a chosen order.
    The LIS loop (`while (t0 < nb)`: an extending run found with one ballot, anything else searched): `reversed` -- every element
    after the first takes the search and replaces tv[1]; `identity` -- one run per 64 elements, `!searched` takes the chain
    from the list itself; `sawtooth(63 | 64 | 65)` -- a run that ends one before, on and one after the 64-element step;
    `two_track` -- the tail search `for (b2 = 0; b2 < l; b2 += 64)` with l past 64 and 128, replacing below and at the last tail;
    n = 1, 2, 63 .. 65, 128, 129, 399 .. 401 around the ballot width and PS_MCAP = 400 (401: the oversize relaunch with 32-bit
    indices in global scratch).  The co-linearity walk (`for (base = 1; base < l; base += 64)`): chains of 2, 64, 65, 66, 129,
    130 elements, distances on both sides of `dist < 10`, a chain element that is not kept at chain index 63, 64, 65, and the
    single distance whose variance divides by nd - 1 = 0.  k = 5: the 6-mer prefilter of the walk is off (`pre`), 5-nt cores
    match everywhere and most pairs are oversize; only the oracle's answer is asserted there."""
    got = _score_all(gpu_ctx, oracle, k, lambda c: "swapped" not in c.claims)
    assert len(got) == len(cs.cases(k, fragments=False))
    if k == 16:
        assert got["k16-nd1-nan"][2] == 1 and np.isnan(got["k16-nd1-nan"][3])
        assert [got[f"k16-reversed-{n}"][4] for n in (399, 400, 401)] == [399, 400, 401]
    assert sum(g[4] > 400 for g in got.values()) >= 4          # the oversize relaunch ran


@pytest.mark.parametrize("k", [10, 11, 16])
def test_fragment_pairs_capacity_edges(gpu_ctx, oracle, k):
    """Stage 1 of pair_score_kernel and its capacities on fragment pairs (B = a stretch of A) with an exact match count.
    399 / 400 / 401 matches against `total + tot <= cap` and `if (total > cap)` with cap = PS_MCAP = 400, in the plain shape and
    in the swapped one (nA > 4 nB + 256: the first pass walks B and sorts the matches back, the oversize relaunch of 401 runs
    not swapped), on both strands.  The searched list at 2047 / 2048 / 2049 k-mers against `b_lds = nS <= bcap`: staged in LDS
    or searched in global memory, with 200 matches (the full pass) and with all of them (the relaunch).  The walked list at
    511 .. 513 and 1023 .. 1025 k-mers against `fetch_walk`'s batches of 64 * WB = 512, with the matches in the last batch.
    Both sides of `nA > 4 * nB + 256` with nB = 100."""
    got = _score_all(gpu_ctx, oracle, k, lambda c: "swapped" in c.claims)
    by_name = {c.name: c for c in cs.cases(k)}
    for swapped in (False, True):
        assert sorted(g[4] for n, g in got.items() if "-fragment-" in n and by_name[n].claims["swapped"] == swapped) == [399, 399, 400, 400, 401, 401]


@pytest.mark.parametrize("mode", ["search", "seed"])
def test_count_form_has_no_capacity(gpu_ctx, oracle, mode):
    """The count form of kernel B through one evaluation of one seed against one candidate (thr = 0.0: kernel A lets the pair
    through): the `reversed` and fragment pairs of k = 16 with 399, 400 and 401 matches.  pair_score_kernel<COUNT> keeps no match
    arrays (`cap = 0`, `if (!COUNT && total + tot <= cap)`), so 400 and 401 must look alike: the per-pair search counts the
    oracle's n_matches.  The seed-major pass (pair_count.hip) counts over hashes folded to 20 bits for k > 10, an upper bound of
    n_matches by design: it is held to exactly that folded count, which IS n_matches for the fragment pairs (generated without a
    folded collision) and lies above it for the `reversed` ones (some 40 collisions among 2 x 6 800 k-mers: 435 for 399)."""
    cases = cs.count_cases()
    reads = [r for c in cases for r in (c.a, c.b)]
    gpu_ctx.load_reads(reads, 16, True)
    rects = [([2 * i], [2 * i + 1], 0.0) for i in range(len(cases))]
    got = gpu_ctx.debug_evaluate(rects, 0.3, count_pass=mode)
    assert got["count_pass"] == {mode}
    S = got["survivors"]
    assert sorted(zip(S["rect"].tolist(), S["strand"].tolist())) == [(r, s) for r in range(len(cases)) for s in (0, 1)]
    assert (S["seed"] == 0).all() and (S["cand"] == 0).all()
    for r, s, cnt in zip(S["rect"], S["strand"], S["count"]):
        c = cases[r]
        nm = oracle.pair_score(c.a, c.b, 16, int(s), dist_cap=1)[4]
        want = nm if mode == "search" else cs.n_common(c.a, c.b, 16, int(s), folded=True)
        assert cnt == want >= nm, (c, mode, int(s), int(cnt), want, nm)
        if s == 0:
            assert nm == c.claims["n_matches"]
            if "fragment" in c.name:
                assert cnt == nm, (c, mode, int(cnt), nm)
