"""The lemma behind the exact rejection of the cluster evaluation (cluster_driver.hip, count_bound_kernel): a pair whose
double(k * |common|) / min_len is below t_s cannot pass cluster_together's score test (cluster.cpp:23-27), because

    hc_bases <= bases <= k * |LIS| <= k * |common|

calc_similarity (similarity.cpp:52-85) adds at most k bases per KEPT element of the longest chain, the kept elements are some of the
chain's, the chain is a subsequence of the common k-mer list, and hc_bases adds a subset of the same terms.  Checked here on the
oracle for k = 1 .. 16 over random, rearranged, repeat-rich and reverse-strand pairs; a counterexample would make the device's
rejection unsound.  |common| is recomputed from the oracle's k-mer lists (sum over shared hashes of the product of their
multiplicities) and |LIS| by a plain patience sort, strictly increasing in the second position as the reference's search is."""
import bisect

import numpy as np
import pytest

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def mutate(rng, s: bytes, rate: float) -> bytes:
    a = np.frombuffer(s, np.uint8)
    r = rng.random(len(a))
    out = a.copy()
    sub = r < rate * 0.5
    out[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    out = out[r >= rate * 0.25]
    return out.tobytes()


def pairs_for(k):
    """(a, b, strand): b's forward list if strand == 0, else its reverse-complement list"""
    rng = np.random.default_rng(4000 + k)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    out = []
    for _ in range(6):                                                # unrelated reads
        out.append((rnd(int(rng.integers(40, 300))), rnd(int(rng.integers(40, 300))), int(rng.integers(0, 2))))
    for _ in range(6):                                                # the same transcript with errors, both strands
        t = rnd(int(rng.integers(80, 400)))
        b = mutate(rng, t, float(rng.choice([0.0, 0.03, 0.1])))
        out.append((mutate(rng, t, 0.05), b, 0))
        out.append((t, revcomp(b), 1))
    for _ in range(4):                                                # rearranged segments: chains far shorter than |common|
        seg = [rnd(int(rng.integers(20, 90))) for _ in range(5)]
        order = rng.permutation(5)
        out.append((b"".join(seg), b"".join(seg[i] for i in order) + seg[0], int(rng.integers(0, 2))))
    for unit in (b"A", b"AC", b"ACG", b"AACGT", b"ACGTTGCA"):      # repeat-rich: large cross products of equal hashes
        n = int(rng.integers(60, 200))
        a = (unit * (n // len(unit) + 1))[:n]
        out.append((a, mutate(rng, a, 0.02), 0))
        out.append((a + rnd(50) + a, revcomp(a[5:]), 1))
        out.append((rnd(40) + a[: n // 2], a, 0))
    out.append((b"", rnd(50), 0))                                     # empty and short reads
    out.append((rnd(k), rnd(k + 1), 0))
    return out


def common_and_lis(oracle, a, b, k, strand):
    fh, fp, _, _, _, _ = oracle.extract_kmers(a, k, False)
    gh, gp, rh, rp, _, _ = oracle.extract_kmers(b, k, True)
    bh, bp = (rh, rp) if strand else (gh, gp)
    matches = []
    for h in np.intersect1d(fh, bh):
        p1 = fp[fh == h]; p2 = bp[bh == h]
        matches += [(int(x), int(y)) for x in p1 for y in p2]
    matches.sort()
    tails = []
    for _, y in matches:                                             # strictly increasing in the second position
        i = bisect.bisect_left(tails, y)
        if i == len(tails):
            tails.append(y)
        else:
            tails[i] = y
    return len(matches), len(tails)


@pytest.mark.parametrize("k", list(range(1, 17)))
def test_bases_never_exceed_k_times_common(oracle, k):
    related = repeats = 0
    for a, b, strand in pairs_for(k):
        bases, hc, nd, var, nm, _ = oracle.pair_score(a, b, k, strand, dist_cap=1)
        common, lis = common_and_lis(oracle, a, b, k, strand)
        assert nm == common, (a, b, strand)
        assert 0 <= hc <= bases <= k * lis <= k * common, (k, a, b, strand, hc, bases, lis, common)
        if common:
            mn = float(min(len(a), len(b)))
            # the device's test itself: a pair rejected on its count is rejected by the reference too, at every threshold
            # up to the one the count allows
            t_s = float(k * common) / mn
            assert float(bases) / mn <= t_s and float(hc) / mn <= t_s
        related += common > 0
        repeats += common > lis
    assert related >= 20 and repeats >= 5        # the pairs did share k-mers, and chains shorter than |common| were there
