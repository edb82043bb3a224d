"""Packs built so that the graph kernel C (poa.hip) aligns against lands on a chosen edge of its row loops: how many in-edges a row has,
how many rows back its predecessors lie, whether the byte fields of the compact plan record saturate.  No GPU and no oracle in here:
tests/test_constructed_graphs.py proves through Oracle.poa_graph that every pack has the shape it is named after, and
tests/test_gpu_poa_graph_edges.py then runs the same packs through the kernel in every form of the row loop, so a GPU case cannot go vacuous.

Every pack is made of exact pieces of one random backbone B, without noise: the graph is B's chain plus the edges the constructor wants.
B itself comes first, and a plain copy of B comes last, so that one alignment sees the finished graph.  The alignment is local (kSW, match 5,
gap open -8, extend -6): a deletion of D graph nodes is bridged only if each flank scores more than the gap costs, 5 flank > 8 + 6 (D - 1)
(`min_flank`); what is not bridged becomes a fresh branch, which is what `branches` is after.

Probes.  A read that CREATES an in-edge does not depend on it, and neither does a read that could cross the same gap at a price: a
deletion adds no node, so the rows come out the same whether the row loop saw the edge or paid for the gap.  So behind the reads that build
a shape come probes, one per in-edge under test: the bases before the edge and, behind it, a flank too short to pay for any way round
(`max_flank`).  Through the edge the flank aligns; a row loop that misses the edge leaves it unaligned, which adds nodes and columns.
tests/test_constructed_graphs.py proves that too, with Oracle.poa_msa_blind (the oracle with a row loop that overlooks chosen in-edges)."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
AGT = np.frombuffer(b"AGT", np.uint8)
PROBE_LEFT = 40          # bases of a probe before its edge (200 points: the probe's alignment is anchored there)


def backbone(seed, L):
    return ACGT[np.random.default_rng(seed).integers(0, 4, L)].copy()


def gap_cost(D):
    return 8 + 6 * (D - 1)


def min_flank(D):
    """the fewest matching bases on each side of a deletion of D graph nodes that the local alignment still bridges"""
    return gap_cost(D) // 5 + 1


def max_flank(D):
    """the most matching bases behind a gap of D nodes (or bases) that do NOT pay for it"""
    return (gap_cost(D) - 1) // 5


def _other(rng, x):
    return [c for c in ACGT if c != x][int(rng.integers(0, 3))]


def ladder_sites(Ds, first=PROBE_LEFT):
    """(a, D) for every D, in the order given: the deletions side by side, every flank long enough for both its neighbours (and a few
    bases more); returns (sites, L)"""
    sites, a = [], max(first, min_flank(Ds[0]) + 4)
    for i, D in enumerate(Ds):
        sites.append((a, D))
        a += D + min_flank(max(Ds[i:i + 2])) + 4
    return sites, a + first


def deletion_ladder(L, sites, seed=0, probe_left=PROBE_LEFT):
    """B, then one read per site (a, D) with B[a : a + D] removed, then one probe per site, then B.  The node after the gap gets a second
    in-edge exactly D + 1 rows back (wherever the gap slides to among equal letters: both ends move together).  The non-chain distances of
    the finished graph are {D + 1}.  The probe of a site is B[a - probe_left : a] (None: B[:a]) + the max_flank(D) bases behind the gap; the
    first base behind the gap differs from the first one in it, so that the flank has no other place to go."""
    rng = np.random.default_rng(1000 * L + seed)
    B = ACGT[rng.integers(0, 4, L)].copy()
    for a, D in sites:
        assert a >= min_flank(D) and L - a - D >= min_flank(D), (a, D, L)
        if B[a + D] == B[a]:
            B[a + D] = _other(rng, B[a])
    reads = [np.concatenate([B[:a], B[a + D:]]).tobytes() for a, D in sites]
    probes = [np.concatenate([B[0 if probe_left is None else a - probe_left:a], B[a + D:a + D + max_flank(D)]]).tobytes() for a, D in sites]
    return [B.tobytes()] + reads + probes + [B.tobytes()]


def ladder(lo, hi, L=None, seed=0, probe_left=PROBE_LEFT):
    """deletion_ladder with D = lo .. hi side by side: distances lo + 1 .. hi + 1; L: the backbone padded in front to this length (a column
    class: the deletions lie in its last columns)"""
    Ds = list(range(lo, hi + 1))
    sites, need = ladder_sites(Ds)
    if L is not None:
        assert L >= need, (L, need)
        sites, need = ladder_sites(Ds, first=PROBE_LEFT + L - need)[0], L
    return deletion_ladder(need, sites, seed, probe_left)


def far_ladder(D, L=1000, seed=0):
    """one deletion of D nodes in the middle of B: a distance of D + 1.  D = 253 .. 256 lie on both sides of the record's distance byte
    (saturated at 255).  One deletion per pack: a second one next to it would be aligned through the first one's edge."""
    return deletion_ladder(L, [((L - D) // 2, D)], seed + D)


def fan(m, s, far_first=False, head=120, tail=200, seed=0, piece=None, order=None, probes=None, probe_left=PROBE_LEFT, last=True):
    """In-degree m + 1 at node c = m s + head of a backbone of c + tail bases, the predecessors 1 + s i rows back (i = 0 .. m): read i is
    B[:c - s i] + B[c:].  The letter rules keep a gap from sliding (runs of equal letters would merge in-edges): B[c] = C, the base
    before every gap G / T in turn, the first base of every gap not C.  Reads in increasing i, so alignment k of the pack sees in-degree
    k at the node and the in-edge order is by distance.
    order: the reads' i in another order (and m = the largest of them).  A read is aligned through an edge that is already there plus an
    insertion, and adds nodes instead of an in-edge, when that is cheaper than its own deletion: keep to `no i < j <= 2 i among the reads
    before read i`.  far_first (reads in decreasing i) breaks that rule: its graph is not a fan (see FAR_FIRST).
    head: pads the backbone in front (a column class; the node lies `tail` columns before the end).  piece: the reads are only the `piece`
    bases on either side of the node, B[c - s m - piece : c - s i] + B[c : c + piece] (long backbones: the oracle's work is rows x columns).
    probes: the i whose in-edge gets a probe behind the reads (default: all, none for far_first), B[c - s i - probe_left : c - s i]
    (None: B[:c - s i]) + B[c : c + 2]: two bases, 10 points, less than any way round costs (a gap of s >= 2).
    last=False: without the copy of B at the end (packs that count their sequences; the probes see the finished graph).
    Returns (pack, c)."""
    if order is None:
        order = list(range(m, 0, -1) if far_first else range(1, m + 1))
    else:
        assert not far_first and m == max(order)
        for k, i in enumerate(order):
            assert not any(i < j <= 2 * i for j in order[:k]), (i, order[:k])
    if probes is None:
        probes = [] if far_first else sorted(order)
    c = m * s + head
    L = c + tail
    rng = np.random.default_rng(7919 * m + 31 * s + seed)
    B = ACGT[rng.integers(0, 4, L)].copy()
    B[c] = ord("C")
    for i in range(1, m + 1):
        if B[c - s * i] == ord("C"):
            B[c - s * i] = AGT[rng.integers(0, 3)]
    for i in range(m + 1):
        B[c - 1 - s * i] = b"GT"[i % 2]
    lo, hi = (0, L) if piece is None else (c - s * m - piece, c + piece)
    assert 0 <= lo and hi <= L and s >= 2
    reads = [np.concatenate([B[lo:c - s * i], B[c:hi]]).tobytes() for i in order]
    pr = [np.concatenate([B[0 if probe_left is None else c - s * i - probe_left:c - s * i], B[c:c + 2]]).tobytes() for i in probes]
    return [B.tobytes()] + reads + pr + ([B.tobytes()] if last else []), c


def fan_distances(m, s, far_first=False, order=None):
    """the in-edge order of the fan node in the finished graph: the chain edge first, then the reads' edges in pack order"""
    if order is None:
        order = range(m, 0, -1) if far_first else range(1, m + 1)
    return [1] + [1 + s * i for i in order]


# near in-edges LAST: in-edge order 1, 7, 9 .. 19, 3, 25 -- the ninth in-edge 3 rows back, inside every ring, the tenth beyond every ring and reach
NEAR_LAST = [3, 4, 5, 6, 7, 8, 9, 1, 12]

# far-first fans: later reads are aligned through the earlier reads' edges plus a short insertion, so the graph is not the plain fan's.  What
# Oracle.poa_graph shows for fan(12, 2, far_first=True) (proved in tests/test_constructed_graphs.py): the in-edges of the row with the most
# in-edges, in in-edge order -- the ninth, tenth and eleventh lie 5, 3 and 1 rows back, inside every ring, the twelfth 23 rows back.  It has
# no probes: a graph of bubbles next to the fans, not a claim.
FAR_FIRST = (12, 2)
FAR_FIRST_DISTANCES = [21, 19, 17, 15, 13, 11, 9, 7, 5, 3, 1, 23]


def wide_pack(L, seed=0):
    """one pack for the wide and segmented classes: the backbone of L nt; nine reads of 600 nt around a fan node 400 columns before the
    backbone's end (in-degree 10: m = 9, s = 2) and their probes; ONE read of 700 nt from the middle of the backbone with deletions of
    1 .. 5 nodes, 100 nt apart (distances 2 .. 6), and a probe for each; the backbone again: the last alignment computes every column of
    the finished graph.  The reads are short because the oracle fills these classes with its scalar loops.  Returns (pack, c)."""
    fpack, c = fan(9, 2, head=L - 418, tail=400, seed=seed, piece=300)
    B = np.frombuffer(fpack[0], np.uint8).copy()
    a0 = L // 2
    keep = np.ones(700, bool)
    sites = [(a0 + 100 + 100 * i, D) for i, D in enumerate(range(1, 6))]
    for a, D in sites:
        keep[a - a0:a - a0 + D] = False
        if B[a + D] == B[a]:
            B[a + D] = _other(np.random.default_rng(a), B[a])
    probes = [np.concatenate([B[a - PROBE_LEFT:a], B[a + D:a + D + max_flank(D)]]).tobytes() for a, D in sites]
    return [B.tobytes()] + fpack[1:-1] + [B[a0:a0 + 700][keep].tobytes()] + probes + [B.tobytes()], c


# branches(): per backbone length the seed whose pack has the rows named below.  A random head or tail aligns somewhere by chance in most
# packs, which moves the rows: these were found by running the proof of tests/test_constructed_graphs.py over seeds 0, 1, ...
BRANCH_SEED = {700: 26, 1200: 13}


def branches(L=700, seed=None):
    """Reads that the local alignment does NOT bridge, so that fresh branches hang on B's chain:
    - heads: random bases + B[t:] -- the random head becomes a chain that enters B[t]; the sort puts it right before B[t], so its first node is
      a row without in-edge in the middle of the order (a mid-order start).  Probes: B[t - 40 : t] + the head's first ten bases -- a row loop
      that gives such a row the row before it as predecessor aligns them, the true one adds ten nodes;
    - tails: B[:t] + X for t = L - 100, L - 200, L - 300 and one random X of 300 nt -- X becomes a chain that the sort puts behind the whole
      of B, and its first node has three in-edges, 101, 201 and 301 rows back and no near one (every in-edge beyond every ring, one
      beyond the distance byte); a fourth tail B[:L - 12] + Y becomes a chain behind X: one in-edge, more than 255 rows back.  X and Y start
      with a letter that is not the backbone's at the place they leave it.  Probes: B[t - 40 : t] + the tail's first ten bases."""
    seed = BRANCH_SEED[L] if seed is None else seed
    rng = np.random.default_rng(4099 + seed)
    B = ACGT[rng.integers(0, 4, L)].copy()
    X = ACGT[rng.integers(0, 4, 300)].copy()
    Y = ACGT[rng.integers(0, 4, 40)].copy()
    X[0] = [x for x in ACGT if x not in (B[L - 100], B[L - 200], B[L - 300])][0]
    Y[0] = [x for x in ACGT if x != B[L - 12]][0]
    H1 = ACGT[rng.integers(0, 4, 60)]
    H2 = ACGT[rng.integers(0, 4, 9)]
    reads = [np.concatenate([H1, B[300:]]), np.concatenate([H2, B[150:]]),
             np.concatenate([B[:L - 100], X]), np.concatenate([B[:L - 200], X]), np.concatenate([B[:L - 300], X]), np.concatenate([B[:L - 12], Y])]
    probes = [np.concatenate([B[L - t - PROBE_LEFT:L - t], X[:10]]) for t in (100, 200, 300)] + [np.concatenate([B[L - 12 - PROBE_LEFT:L - 12], Y[:10]])]
    probes += [np.concatenate([B[300 - PROBE_LEFT:300], H1[:10]]), np.concatenate([B[150 - PROBE_LEFT:150], H2])]
    return [B.tobytes()] + [r.tobytes() for r in reads + probes] + [B.tobytes()]


def old_far_pack():
    """the pack of test_gpu_poa.py::test_predecessors_hundreds_of_rows_back_and_many_in_edges as it has always been (noisy reads, `exon skips`
    that the local alignment does not bridge, prefixes glued to a common tail), sorted by length"""
    rng = np.random.default_rng(77)
    acgt = ACGT
    tx = acgt[rng.integers(0, 4, 1400)]

    def noisy(a, err=0.06):
        r = rng.random(len(a))
        b = a.copy()
        sub = r < err * 0.4
        b[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
        return b[(r >= err * 0.7) | (r < err * 0.4)]          # a few deletions too

    pack = [noisy(tx).tobytes() for _ in range(10)]
    for a, n in ((200, 300), (450, 620), (800, 410), (150, 505)):
        pack.append(noisy(np.concatenate([tx[:a], tx[a + n:]])).tobytes())
    for cut in range(300, 960, 55):
        pack.append(noisy(np.concatenate([tx[:cut], tx[1000:]]), 0.03).tobytes())
    pack.sort(key=lambda s: -len(s))
    return pack


# ---- what a graph of Oracle.poa_graph says ----
def shape(graph):
    """of one (indeg, off, dist): the largest in-degree and its rank, the sorted distances other than 1, and the ranks > 0 without in-edge"""
    indeg, off, dist = graph
    return {"max_in": int(indeg.max()), "max_in_rank": int(indeg.argmax()),
            "non_chain": sorted(int(d) for d in dist[dist != 1]),
            "starts": [int(r) for r in np.nonzero(indeg == 0)[0] if r > 0]}


def in_edges(graph, rank):
    indeg, off, dist = graph
    return [int(d) for d in dist[off[rank]:off[rank + 1]]]


def all_far_rows(graph, far):
    """ranks with in-edges, all of them more than `far` rows back -> [(rank, [distances])]"""
    indeg, off, dist = graph
    out = []
    for r in np.nonzero(indeg > 0)[0]:
        d = dist[off[r]:off[r + 1]]
        if d.min() > far:
            out.append((int(r), [int(x) for x in d]))
    return out


# ---- the packs of tests/test_gpu_poa_graph_edges.py, by name; tests/test_constructed_graphs.py proves each one's claim ----
PACKED_L = (None, 1300, 1800, 2300)          # backbone lengths of the ladder in column classes 0 .. 3 (None: as short as the flanks allow, 949)
LADDER_DISTANCES = range(2, 27)              # of ladder(1, 25)
BAND_LADDER_DISTANCES = range(2, 14)         # of ladder(1, 12)
FAN_L = (None, 1400, 1900, 2400)             # the fans' backbones in classes 0 .. 3 (None: head = 120); the fan node lies 200 columns before the end
SMALL_FANS = ((9, 2), (16, 2), (9, 3), (9, 40))
# the big fans (s = 2): (m, the probes' i, whether B comes again at the end) -- three packs of exactly POA_CHAIN_SEQS = 256 sequences with
# in-degree up to 253, 254 and 255, one of 257 sequences, and in-degree up to 256 and 258 (261 and 263 sequences)
BIG_FANS = ((252, (8, 252), True), (253, (8, 253), False), (254, (254,), False), (253, (8, 253), True), (255, (8, 253, 254, 255), True), (257, (8, 255, 256, 257), True))
FAR_DS = (253, 254, 255, 256)
WIDE_L = (3000, 5000, 7000, 9000)


def class_head(m, s, cls):
    return 120 if FAN_L[cls] is None else FAN_L[cls] - 200 - m * s


def class_fan(m, s, cls=0, **kw):
    """fan(m, s) on a backbone of FAN_L[cls] bases"""
    return fan(m, s, head=class_head(m, s, cls), **kw)


def big_fan(m, probes, last=True, cls=0):
    """fan(m, 2) with probes for a few in-edges only"""
    return class_fan(m, 2, cls, probes=list(probes), last=last)
