"""Read pairs built so that kernel B's match list (pair_score.hip) lands on a chosen edge, and the claims each pair makes about
itself.  No GPU and no oracle in here: tests/test_constructed_pairs.py proves every claim on the oracle alone, and
tests/test_gpu_pair_score_edges.py then runs the same pairs through the kernel, so a GPU case cannot go vacuous.

Core / separator pairs.  Read A is n random cores of k nt, one separator base from {A, C} before each and k + 1 separator bases
after the last (extract_kmers_from_read drops the last k-mer of a read: the last core must lie inside L - k).  Read B holds the same
cores in another order with separators from {G, T}, `gap[t]` of them before block t.  A k-mer that touches a separator has an A / C
where the other read can only have G / T or a core base, so (for k = 16: at k = 10, 11 a few chance matches come on top) the match list
is one match per core; in pos1 order the pos2 ranks are the chosen `rank`, and with rank = identity the walk's distance list is gap[t] - 1.

Fragment pairs.  A is random and B = A[a : a + m + k]: m matches when A has no repeated k-mer.  The seed of the generator is advanced
until the plain count below says so."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
CODE = np.zeros(256, np.int64)
for _c, _v in zip(b"ACTG", range(4)):
    CODE[_c] = _v


def revcomp(s):
    return s.translate(COMP)[::-1]


def rnd(rng, n, alphabet=ACGT):
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


def kmer_values(s, k, folded=False):
    """the hashes (kmer.hpp:25-40) of positions 0 .. L - k - 1, the list of extract_kmers_from_read, in position order"""
    c = CODE[np.frombuffer(s, np.uint8)]
    nk = max(len(s) - k, 0)
    h = np.zeros(nk, np.int64)
    for i in range(k):
        h = h * 4 + c[i:i + nk]
    return fold20(h) if folded else h


def fold20(h):
    """the 20-bit fold of the seed-major count pass (pair_count.hip) for k > 10"""
    return (h ^ (h >> 20)) & 0xFFFFF


def n_common(a, b, k, strand=0, folded=False):
    """|common| of get_common_kmers: the sum over shared k-mers of the product of their multiplicities.  folded: over the hashes as
    the seed-major count pass sees them for k > 10 (an upper bound of |common|, equal to it when no two k-mers fold together)."""
    ha, hb = kmer_values(a, k, folded and k > 10), kmer_values(revcomp(b) if strand else b, k, folded and k > 10)
    va, ca = np.unique(ha, return_counts=True)
    vb, cb = np.unique(hb, return_counts=True)
    _, ia, ib = np.intersect1d(va, vb, return_indices=True)
    return int((ca[ia] * cb[ib]).sum())


class Case:
    """One pair: reads a (the seed, walked unless the swap runs) and b, the strand of b, and `claims`: what the oracle must say of it
    (keys: n_matches, min_matches, lis, nd, nd_below_lis, nan_var, hc_below_bases, searched_beyond_chain, swapped, n_searched,
    n_walked)."""

    def __init__(self, name, a, b, strand=0, **claims):
        self.name, self.a, self.b, self.strand, self.claims = name, a, b, strand, claims

    def __repr__(self):
        return self.name


# ---- pos2 ranks in pos1 order -------------------------------------------------------------------------------------------------
def reversed_rank(n):
    return np.arange(n)[::-1].copy()


def identity_rank(n):
    return np.arange(n)


def random_rank(n, seed=0):
    return np.random.default_rng(1000 + seed + n).permutation(n)


def sawtooth_rank(r, groups=4):
    """`groups` ascending groups of r, each group below the one before: an extending run of exactly r elements, then a search"""
    return np.concatenate([np.arange(g * r, (g + 1) * r) for g in range(groups - 1, -1, -1)])


def two_track_rank(n):
    """pos2 alternates between a high ascending track and a low one: LIS n / 2, every other element searches the tails"""
    r = np.zeros(n, np.int64)
    r[0::2] = n // 2 + np.arange((n + 1) // 2)
    r[1::2] = np.arange(n // 2)
    return r


def walk_gaps(n):
    """separator lengths of B that give the distances 0 .. 24 in identity order: both sides of `dist < 10` (similarity.cpp:73)"""
    return 1 + (7 * np.arange(n)) % 25


def core_pair(k, rank, gaps=None, split_at=None, seed=0):
    """(A, B) of the core / separator construction.  rank[c]: the rank of core c's block in B.  gaps[t]: separators before block t
    of B (default 1 each).  split_at = c: core c is k + 1 nt -- two overlapping k-mers in A -- and B carries the two as separate blocks
    (so B has one block more, and every later rank moves up by one)."""
    rng = np.random.default_rng([k, len(rank), seed, 77])
    n = len(rank)
    cores = [rnd(rng, k + 1 if c == split_at else k) for c in range(n)]
    if split_at is not None:
        # its two k-mers share k - 1 bases: the end bases from {A, C}, or B's separator next to one block completes the other k-mer
        cores[split_at] = rnd(rng, 1, ACGT[:2]) + cores[split_at][1:k] + rnd(rng, 1, ACGT[:2])
    a = b"".join(rnd(rng, 1, ACGT[:2]) + c for c in cores) + rnd(rng, k + 1, ACGT[:2])
    blocks = [None] * n
    for c in range(n):
        blocks[rank[c]] = [cores[c]] if c != split_at else [cores[c][:k], cores[c][1:]]
    blocks = [x for bl in blocks for x in bl]
    gaps = np.ones(len(blocks), np.int64) if gaps is None else np.asarray(gaps)
    assert len(gaps) == len(blocks) and gaps.min() >= 1
    gt = ACGT[2:]                                          # {G, T}
    b = b"".join(rnd(rng, int(g), gt) + x for g, x in zip(gaps, blocks)) + rnd(rng, k + 1, gt)
    return a, b


CORE_N = (1, 2, 63, 64, 65, 128, 129, 399, 400, 401)
CHAIN_N = (2, 64, 65, 66, 129, 130)
SPLIT_AT = (63, 64, 65)                                    # chain index of the element that is in the chain and NOT kept


def core_cases(k):
    """Every core / separator case for one k.  `exact` claims (n_matches == n, LIS) are made at k = 16 only; below that the claims
    are the weaker ones that hold with chance matches too."""
    exact = k == 16
    out = []

    def add(name, rank, gaps=None, split_at=None, strand=0, **claims):
        a, b = core_pair(k, rank, gaps, split_at)
        n = len(rank) + (split_at is not None)
        if exact:
            claims["n_matches"] = n
        elif k >= 10:
            claims["min_matches"] = n
        if k < 10:
            claims = {}                                    # k = 5: cores match everywhere; only the oracle's answer counts
        if strand:
            b = revcomp(b)
        out.append(Case(f"k{k}-{name}" + ("-rc" if strand else ""), a, b, strand, **claims))

    for n in CORE_N:
        # every element after the first is below the only tail: searched, l stays 1, bases = k, no distance
        add(f"reversed-{n}", reversed_rank(n), **({"lis": 1, "nd": 0} if exact else {"searched_beyond_chain": n > 1}))
        # never searched: the chain is the list
        add(f"identity-{n}", identity_rank(n), **({"lis": n, "nd": n - 1} if exact else {}))
        add(f"random-{n}", random_rank(n), **({} if exact else {"searched_beyond_chain": n > 2}))
    for n in (401,):                                        # the other strand: B reverse-complemented, strand = 1
        add(f"reversed-{n}", reversed_rank(n), strand=1, **({"lis": 1, "nd": 0} if exact else {}))
        add(f"identity-{n}", identity_rank(n), strand=1, **({"lis": n, "nd": n - 1} if exact else {}))
        add(f"random-{n}", random_rank(n), strand=1)
    for r in (63, 64, 65):
        add(f"sawtooth-{r}", sawtooth_rank(r), **({"lis": r, "nd": r - 1} if exact else {}))
    add("sawtooth-64", sawtooth_rank(64), strand=1, **({"lis": 64, "nd": 63} if exact else {}))
    add("two-track-300", two_track_rank(300), **({"lis": 150, "nd": 149} if exact else {}))
    add("two-track-300", two_track_rank(300), strand=1, **({"lis": 150, "nd": 149} if exact else {}))
    add("two-track-131", two_track_rank(131))
    # the walk, identity order: distances on both sides of 10, chains that end on every side of a 64-element step
    add("walk-130", identity_rank(130), walk_gaps(130), hc_below_bases=True, **({"nd": 129, "lis": 130} if exact else {}))
    for n in CHAIN_N:
        add(f"chain-{n}", identity_rank(n), walk_gaps(n), **({"nd": n - 1, "lis": n} if exact else {}))
    add("nd1-nan", identity_rank(2), [1, 40], **({"nd": 1, "lis": 2} if exact else {}), nan_var=True)
    for at in SPLIT_AT:
        # the second k-mer of core at - 1 is chain element `at`: d1 = 1 < k, d2 >= k, not kept
        add(f"split-{at}", identity_rank(130), 1 + (3 * np.arange(131)) % 4, split_at=at - 1, nd_below_lis=True,
            **({"lis": 131, "nd": 129} if exact else {}))
    return out


def fragment_pair(k, la, m, strand=0, prefix=0, exact=True, at_most=None):
    """A of `la` nt and B = `prefix` random nt + A[a : a + m + k] (reverse-complemented for strand 1): (A, B, |common|).  exact: the
    seed moves on until |common| == m (A has no second copy of a k-mer of B) and the seed-major count pass, which folds the hashes of
    k > 10 to 20 bits, counts m as well; otherwise until |common| <= at_most."""
    for s in range(400):
        rng = np.random.default_rng([k, la, m, s, prefix, 78])
        a = rnd(rng, la)
        at = int(rng.integers(0, la - m - k + 1))
        b = rnd(rng, prefix) + a[at:at + m + k]
        if strand:
            b = revcomp(b)
        c = n_common(a, b, k, strand)
        if (c == m and n_common(a, b, k, strand, True) == m) or (not exact and (at_most is None or c <= at_most)):
            return a, b, c
    raise AssertionError("no seed gives the wanted match count")


def is_swapped(a, b, k):
    """pair_score.hip: the short list is walked when nA > 4 nB + 256"""
    return max(len(a) - k, 0) > 4 * max(len(b) - k, 0) + 256


def fragment_cases(k):
    out = []
    for la in (700, 3000):                                 # 3000: nA > 4 nB + 256, the swapped walk (and its sort) runs
        for m in (399, 400, 401):                          # PS_MCAP = 400: 401 takes the oversize relaunch
            for strand in (0, 1):
                a, b, _ = fragment_pair(k, la, m, strand)
                out.append(Case(f"k{k}-fragment-{la}-{m}" + ("-rc" if strand else ""), a, b, strand, n_matches=m, nd=m - 1,
                                swapped=la == 3000))
    # the searched list at the LDS capacity bcap = 2048: a fragment of the seed (>= nS matches: oversize, searched from global memory
    # past 2048) and a mostly unrelated candidate of the same length (<= 400 matches: the full pass itself on either side of bcap)
    for ns in (2047, 2048, 2049):
        a, b, c = fragment_pair(k, ns + k + 300, ns, exact=False)
        out.append(Case(f"k{k}-searched-{ns}-all", a, b, 0, n_matches=c, min_matches=ns, swapped=False, n_searched=ns))
        a, b, c = fragment_pair(k, ns + k + 300, 200, prefix=ns - 200, exact=False, at_most=400)
        out.append(Case(f"k{k}-searched-{ns}-200", a, b, 0, n_matches=c, min_matches=200, swapped=False, n_searched=ns))
    # the walked list is fetched 512 k-mers per batch (WB = 8 steps of 64): lists that end before, on and after a batch edge, with the
    # matches at the END of the walk; not swapped (A walked) and swapped (B walked, 300 of its k-mers in A)
    for nw in (511, 512, 513, 1023, 1024, 1025):
        rng = np.random.default_rng([k, nw, 79])
        for s in range(400):
            a = rnd(rng, nw + k)
            b = rnd(rng, 40) + a[-(300 + k):]              # a's last k-mers, the neighbours of the dropped one included
            c = n_common(a, b, k)
            if c <= 400:
                break
        else:
            raise AssertionError("no seed gives the wanted match count")
        out.append(Case(f"k{k}-walked-{nw}-tail", a, b, 0, n_matches=c, min_matches=300, swapped=False, n_walked=nw))
        a, b, c = fragment_pair(k, 4 * nw + 257 + k + 100, 300, prefix=nw - 300, exact=False, at_most=400)
        out.append(Case(f"k{k}-walked-{nw}-swapped", a, b, 0, n_matches=c, min_matches=300, swapped=True, n_walked=nw))
    # both sides of the swap threshold nA > 4 nB + 256, nB = 100
    for extra, swapped in ((0, False), (1, True)):
        a, b, _ = fragment_pair(k, 4 * 100 + 256 + extra + k, 100)
        out.append(Case(f"k{k}-swap-threshold-{'above' if swapped else 'at'}", a, b, 0, n_matches=100, nd=99, swapped=swapped,
                        n_searched=4 * 100 + 256 + extra if swapped else 100))
    return out


def count_cases():
    """the k = 16 pairs that also go through the count form (debug_evaluate): it has no capacity, 400 and 401 must look alike"""
    names = [f"k16-reversed-{n}" for n in (399, 400, 401)] + [f"k16-fragment-{la}-{m}" for la in (700, 3000) for m in (399, 400, 401)]
    return [c for c in cases(16) if c.name in names]


_cache = {}


def cases(k, fragments=True):
    """all cases of one k (built once)"""
    if k not in _cache:
        _cache[k] = (core_cases(k), fragment_cases(k) if k >= 10 else [])
    core, frag = _cache[k]
    return core + (frag if fragments else [])
