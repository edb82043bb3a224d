"""The constructed packs of tests/constructed_graphs.py have the graph shape they are named after -- on the CPU oracle alone, no GPU.
Oracle.poa_graph gives, for every alignment of a pack, the graph it is computed against (in-degree per rank, distance rank - predecessor's
rank per in-edge, in in-edge order); tests/test_gpu_poa_graph_edges.py runs the same packs through kernel C.  What is proven here is which
edge of poa.hip's row loops each pack sits on: the in-degree the fan node has at every alignment (4 / 5: the second batch of fetches; 8 / 9:
the edge-list walk; 254 / 255 / 256: the in-degree byte of the compact plan record), the exact distances of a ladder (R and R + 1 for every
ring and reach; 254 .. 257 around the distance byte), a row whose every in-edge is far, a row without in-edge in the middle of the order."""
import numpy as np
import pytest

import constructed_graphs as cg


@pytest.fixture(scope="module")
def graphs(oracle):
    """Oracle.poa_graph with the AVX2 rows (exact where they run, 5 L + 64 < 32 000; the scalar loops elsewhere)"""
    def run(pack):
        oracle.set_poa_simd(True)
        try:
            return oracle.poa_graph(list(pack))
        finally:
            oracle.set_poa_simd(False)
    return run


def test_hook_on_a_hand_graph(oracle):
    """ACGTACGT, then ACGACGT (T deleted: a second in-edge two rows back at the second A), then the first again"""
    g = oracle.poa_graph([b"ACGTACGTTTGACA", b"ACGACGTTTGACA", b"ACGTACGTTTGACA"])
    assert len(g) == 2
    indeg, off, dist = g[0]
    assert indeg.tolist() == [0] + [1] * 13 and dist.tolist() == [1] * 13 and off.tolist() == [0] + list(range(14))
    indeg, off, dist = g[1]
    assert indeg.tolist() == [0, 1, 1, 1, 2] + [1] * 9
    assert cg.in_edges(g[1], 4) == [1, 2] and cg.shape(g[1]) == {"max_in": 2, "max_in_rank": 4, "non_chain": [2], "starts": []}
    assert oracle.poa_graph([b"ACGT"]) == [] and oracle.poa_graph([]) == []


def test_hook_agrees_with_the_msa_loop(oracle):
    """the hook runs poa_msa's own loop: as many rows per alignment as the cell count of poa_msa says"""
    pack = cg.branches(700)
    g = oracle.poa_graph(pack)
    _, cells = oracle.poa_msa(pack)
    assert cells == sum(len(x[0]) * len(s) for x, s in zip(g, pack[1:]))


@pytest.fixture(scope="module")
def notices(oracle):
    """the pack's rows change under each of the given wrong row loops (Oracle.poa_msa_blind)"""
    def run(pack, wrong):
        oracle.set_poa_simd(True)
        try:
            want, _ = oracle.poa_msa(list(pack))
            missed = [w for w in wrong if oracle.poa_msa_blind(list(pack), *w) == want]
        finally:
            oracle.set_poa_simd(False)
        assert not missed, missed
    return run


def test_blind_oracle_on_a_hand_graph(oracle):
    """hiding nothing gives poa_msa's rows; hiding the shortcut of the hand graph changes how its probe aligns"""
    pack = [b"ACGTACGTTTGACA", b"ACGACGTTTGACA", b"GTTACGA", b"ACGTACGTTTGACA"]
    want, _ = oracle.poa_msa(pack)
    assert want[2] == b"GTTACG-A---------"                                # ACG, then the A behind the deleted T through the shortcut
    assert oracle.poa_msa_blind(pack, "from", 9) == want and oracle.poa_msa_blind(pack, "at", 7) == want
    assert oracle.poa_msa_blind(pack, "from", 1) != want and oracle.poa_msa_blind(pack, "at", 2) != want


_CLASS_MAX = (1024, 1536, 2048, 2560)


def _in_class(pack, cls):
    return (0, 1024, 1536, 2048)[cls] < max(map(len, pack)) <= _CLASS_MAX[cls]


@pytest.mark.parametrize("cls", range(4))
def test_ladder_distances(graphs, notices, cls):
    """distances 2 .. 26, each once, and nothing else: R and R + 1 for the rings of 3, 4 and 8 rows and every team reach up to 24.  A row
    loop that overlooks the in-edges of one distance changes the rows, whichever distance it is (class 1: R and R + 1 of the barrier form's ring of 4)"""
    pack = cg.ladder(1, 25, cg.PACKED_L[cls])
    assert len(pack) == 52 and _in_class(pack, cls)
    sh = cg.shape(graphs(pack)[-1])
    assert sh["non_chain"] == list(cg.LADDER_DISTANCES) and sh["max_in"] == 2 and sh["starts"] == []
    if cls < 2:                                                           # (classes 2 and 3: the same sites behind a longer pad)
        notices(pack, [("at", d) for d in (cg.LADDER_DISTANCES, (4, 5))[cls]])


@pytest.mark.parametrize("cls", range(4))
def test_band_ladder_distances(graphs, notices, cls):
    """the band's ladder: distances 2 .. 13 (its rings have 8 or 4 slots), the probes as long as the band's spread of lengths wants them"""
    pack = cg.ladder(1, 12, cg.PACKED_L[cls], probe_left=None)
    assert max(map(len, pack)) - min(map(len, pack)) < 400 and _in_class(pack, cls)
    assert cg.shape(graphs(pack)[-1])["non_chain"] == list(cg.BAND_LADDER_DISTANCES)
    if cls < 2:
        notices(pack, [("at", d) for d in (4, 5, 8, 9)])


@pytest.mark.parametrize("L", [1000, 1300])
@pytest.mark.parametrize("D", cg.FAR_DS)
def test_far_ladder_distance(graphs, notices, D, L):
    """one in-edge exactly D + 1 = 254 .. 257 rows back; overlooked, the rows change"""
    pack = cg.far_ladder(D, L)
    g = graphs(pack)
    assert cg.shape(g[-1])["non_chain"] == [D + 1] and cg.shape(g[0])["non_chain"] == []
    notices(pack, [("at", D + 1), ("beyond", min(D + 1, 255))])


def test_unbridged_deletion_is_a_branch(graphs):
    """the rule the ladders keep to: a deletion of 400 nodes at L = 1000 has flanks of 300 < 481 and is not bridged"""
    assert cg.min_flank(400) == 481 and cg.max_flank(1) == 1 and cg.max_flank(2) == 2 and cg.max_flank(25) == 30
    B = cg.backbone(5, 1000)
    sh = cg.shape(graphs([B.tobytes(), np.concatenate([B[:300], B[700:]]).tobytes(), B.tobytes()])[-1])
    assert 401 not in sh["non_chain"] and sh["starts"]


def _fan_claim(graphs, pack, c, m, s, order=None):
    """alignment k sees in-degree k at the node (m + 1 from the first probe on) and no row has more; the in-edge order"""
    g = graphs(pack)
    want = list(range(1, m + 2)) if order is None else list(range(1, len(order) + 2))
    want += [want[-1]] * (len(g) - len(want))
    assert [int(x[0][c]) for x in g] == want
    assert [int(x[0].max()) for x in g[1:]] == want[1:]
    assert cg.in_edges(g[-1], c) == cg.fan_distances(m, s, order=order)
    assert len(g[-1][0]) == len(pack[0])                                  # the probes add no node
    return g


# (m, s, class): the GPU tests' fans in classes 0 and 1, the (16, 2) fan in classes 2 and 3; and the in-degrees the issue probed one by one
_FAN_CASES = [(m, s, c) for c in (0, 1) for m, s in cg.SMALL_FANS] + [(16, 2, 2), (16, 2, 3)] + [(m, s, 0) for m, s in ((3, 2), (4, 2), (7, 2), (8, 2), (8, 3), (8, 40))]


@pytest.mark.parametrize("m,s,cls", _FAN_CASES)
def test_fan_in_degree(graphs, notices, m, s, cls):
    """... and a row loop that stops after the fourth, the eighth or the next-to-last in-edge, or overlooks any one of them, changes the rows"""
    pack, c = cg.class_fan(m, s, cls)
    assert _in_class(pack, cls) and c == len(pack[0]) - 200
    g = _fan_claim(graphs, pack, c, m, s)
    if s == 40:
        assert sum(d >= 255 for d in cg.in_edges(g[-1], c)) == (2 if m == 8 else 3)
    wrong = [("from", k) for k in (4, 8, m) if k <= m and cls < 2]
    if cls == 0:
        wrong += [("at", d) for d in cg.fan_distances(m, s)[1:]] + ([("beyond", 255)] if s == 40 else [])
    notices(pack, wrong)


def test_fan_breaks_without_its_letter_rules(graphs):
    """what the rules are for: with the bases before the gaps all equal to the one before the node, gaps slide and in-edges merge"""
    pack, c = cg.fan(9, 2)
    B = np.frombuffer(pack[0], np.uint8).copy()
    B[c - 19:c] = ord("G")
    broken = [B.tobytes()] + [np.concatenate([B[:c - 2 * i], B[c:]]).tobytes() for i in range(1, 10)] + [B.tobytes()]
    assert int(graphs(broken)[-1][0].max()) < 10


@pytest.mark.parametrize("m,probes,last", cg.BIG_FANS, ids=["%d-%dseq" % (m, m + 1 + len(p) + l) for m, p, l in cg.BIG_FANS])
def test_big_fan_in_degree(graphs, notices, m, probes, last):
    """256, 256, 256, 257, 261 and 263 sequences (on both sides of POA_CHAIN_SEQS = 256), in-degree k at alignment k up to m + 1 = 253 .. 258;
    a row loop that overlooks the last in-edge changes the rows -- for m = 257 also one that stops at the in-degree byte's 255, one before
    or one after, or after the eighth in-edge"""
    pack, c = cg.big_fan(m, probes, last)
    assert len(pack) == m + 1 + len(probes) + last and max(map(len, pack)) == 2 * m + 320 <= 1024
    assert len(pack) == {252: 256, 254: 256, 255: 261, 257: 263}.get(m, 257 if last else 256)
    _fan_claim(graphs, pack, c, m, 2)
    notices(pack, [("from", m)] + ([("from", k) for k in (8, 254, 255, 256)] if m == 257 else []))


def test_big_fan_in_class_1(graphs):
    pack, c = cg.big_fan(257, (8, 255, 256, 257), cls=1)
    assert len(pack) == 263 and _in_class(pack, 1)
    _fan_claim(graphs, pack, c, 257, 2)


def test_band_fans(graphs, notices):
    """fans whose lengths spread by less than POA_BAND_SPREAD = 400, probes included: in-degree 10 and 17, and the largest at s = 2, 191"""
    for m, probes in ((9, None), (16, None), (190, [8, 50])):
        pack, c = cg.fan(m, 2, probes=probes, probe_left=None)
        assert max(map(len, pack)) - min(map(len, pack)) < 400
        _fan_claim(graphs, pack, c, m, 2)
        notices(pack, [("from", 8)])
    assert max(map(len, pack)) - min(map(len, pack)) == 380


@pytest.mark.parametrize("cls", [0, 1])
def test_near_last_fan(graphs, notices, cls):
    """near in-edges last: in-edge order 1, 7 .. 19, 3, 25 -- the ninth in-edge 3 rows back (inside every ring), the tenth beyond every reach;
    overlooking either changes the rows"""
    pack, c = cg.class_fan(12, 2, cls, order=cg.NEAR_LAST)
    assert _in_class(pack, cls)
    g = _fan_claim(graphs, pack, c, 12, 2, cg.NEAR_LAST)
    assert cg.in_edges(g[-1], c) == [1, 7, 9, 11, 13, 15, 17, 19, 3, 25]
    notices(pack, [("from", 8), ("from", 9), ("at", 3), ("at", 25)])


@pytest.mark.parametrize("cls", [0, 1])
def test_far_first_fan(graphs, cls):
    """reads in decreasing i do not give a fan: what they give instead (a row of twelve in-edges, the near ones last, among bubbles)"""
    m, s = cg.FAR_FIRST
    pack, c = cg.class_fan(m, s, cls, far_first=True)
    g = graphs(pack)
    sh = cg.shape(g[-1])
    assert sh["max_in"] == 12 and cg.in_edges(g[-1], sh["max_in_rank"]) == cg.FAR_FIRST_DISTANCES
    assert [int(x[0].max()) for x in g][-4:] == [9, 10, 11, 12]
    assert len(g[-1][0]) > len(pack[0])


@pytest.mark.parametrize("L", sorted(cg.BRANCH_SEED))
def test_branches_rows(graphs, notices, L):
    """two rows without in-edge in the middle of the order; a row with three in-edges 101, 201 and 301 rows back and none nearer; rows whose
    only in-edge is more than 255 rows back.  The rows change under a row loop that overlooks one of the three, or everything beyond the
    distance byte or beyond the longest ring, or that gives a row without in-edge the row before it as predecessor"""
    pack = cg.branches(L)
    assert max(map(len, pack)) == L + 200
    g = graphs(pack)
    n = len(g[-1][0])
    starts = cg.shape(g[-1])["starts"]
    assert len(starts) == 2 and all(100 < r < n - 100 for r in starts)
    far = [d for _, d in cg.all_far_rows(g[-1], 24)]
    assert far[:2] == [[101, 201, 301], [313]] and all(len(d) == 1 and d[0] >= 255 for d in far[2:])
    notices(pack, [("at", 101), ("at", 201), ("at", 301), ("beyond", 255), ("beyond", 25), ("start", 0)])


@pytest.mark.parametrize("L", cg.WIDE_L)
def test_wide_pack(graphs, notices, L):
    """in-degree 1 .. 10 at the fan node (400 columns before the end), then distances 2 .. 6 from one read; probes for all of them"""
    pack, c = cg.wide_pack(L)
    assert len(pack) == 26 and len(pack[0]) == L and c == L - 400 and max(map(len, pack[1:-1])) <= 700
    g = graphs(pack)
    assert [int(x[0][c]) for x in g] == list(range(1, 11)) + [10] * 15
    assert cg.in_edges(g[-1], c) == cg.fan_distances(9, 2)
    assert cg.shape(g[-1])["non_chain"] == sorted([2, 3, 4, 5, 6] + cg.fan_distances(9, 2)[1:]) and len(g[-1][0]) == L
    if L < 6000:
        notices(pack, [("from", 8), ("at", 4)])


def test_reach_of_the_old_far_pack(graphs):
    """test_gpu_poa.py::test_predecessors_hundreds_of_rows_back_and_many_in_edges: what its noisy pack reaches, sorted and reversed"""
    pack = cg.old_far_pack()
    for p, max_in, n_far, mid_starts, all_far in ((pack, 8, 6, 0, 2), (pack[::-1], 5, 5, 1, 6)):
        gr = graphs(p)[-1]
        sh = cg.shape(gr)
        assert sh["max_in"] == max_in                                     # never more than eight in-edges
        assert sum(d >= 255 for d in sh["non_chain"]) == n_far            # predecessors 255 or more rows back
        assert sum(10 < r < len(gr[0]) - 10 for r in sh["starts"]) == mid_starts
        assert len(cg.all_far_rows(gr, 8)) == all_far
