"""The report form of the verdict kernel alone, through the test hook rattle_hip_debug_evaluate on a context with the cluster
report on: the evidence record it writes beside every accepted pair -- bases, hc_bases and the 64 bits of the variance -- is what
oracle.pair_score gives for that pair, whichever launch accepted it (the first verdict launch, or the second one after the
oversize full pass, whose hits are appended behind the first launch's), for both use_hc values and every selectable count pass;
and the hits themselves are the hits of the plain kernel.

One evaluation holds more than 8192 hits (more than travel with the counters: the evidence is fetched in two parts like the
hits) from 11 000 full comparisons, 43 blocks with a partial last wavefront; an isoform family on both strands, accepted and
rejected side by side in a wavefront; and the four repeat reads whose pairs exceed the LDS match capacity (400 matches)."""
import numpy as np
import pytest

from rattle_amd import synth

pytestmark = pytest.mark.gpu

MODES = ("seed", "search", "index")
K, T_S, T_V, MCAP = 10, 0.5, 1000000.0, 400
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def build_scene(oracle):
    """the reads, the rectangles of the one evaluation, and the oracle's pair_score behind a cache"""
    rng = np.random.default_rng(11)
    same = synth.reads(110, 1, 1, False, seed=12, exon=(30, 40), sub=0.01, ins=0.005, dele=0.005)[0]      # one transcript, one strand
    iso = synth.reads(200, 6, 3, True, seed=13, exon=(20, 45))[0]                                       # isoforms, both strands
    rep = [b"AC" * 640, b"CA" * 640 + b"GGT", b"AC" * 400 + rnd(rng, 400), b"AC" * 250 + rnd(rng, 2000)]
    reads = same + iso + rep
    S = np.arange(len(same), dtype=np.uint32)
    I = np.arange(len(same), len(same) + len(iso), dtype=np.uint32)
    R = np.arange(I[-1] + 1, I[-1] + 1 + len(rep), dtype=np.uint32)
    rects = [(S[:100], S, 0.0), (R, R[::-1].copy(), 0.0), (R[:2], None, 0.0), (I[:60], I[60:], 0.2), (I[:30], None, 0.1)]
    cache = {}

    def score(i, j, strand):
        key = (int(i), int(j), int(strand))
        if key not in cache:
            cache[key] = oracle.pair_score(reads[key[0]], reads[key[1]], K, key[2], dist_cap=1)[:5]
        return cache[key]

    return reads, rects, score


@pytest.fixture(scope="module")
def scene(oracle):
    return build_scene(oracle)


def hit_keys(H):
    return (H["rect"].astype(np.int64) << 42) | (H["seed"].astype(np.int64) << 21) | (H["cand"].astype(np.int64) << 1) | H["strand"]


@pytest.mark.parametrize("use_hc", [False, True], ids=["bases", "hc"])
def test_evidence_of_every_hit_is_the_oracles_pair_score(gpu_ctx, scene, use_hc):
    """Every count pass with more than 8192 hits and both strands; the repeat reads' rectangles (1.8 s of oversize full pass per
    evaluation, whatever the count pass) ride along in one count pass per use_hc value: "seed" without, "search" with use_hc."""
    reads, all_rects, score = scene
    gpu_ctx.load_reads(reads, K, True)
    for mode in MODES:
        with_rep = mode == MODES[int(use_hc)]
        rects = all_rects if with_rep else [all_rects[0]] + all_rects[3:]
        plain = gpu_ctx.debug_evaluate(rects, T_S, T_V, use_hc, False, mode)
        assert "evidence" not in plain
        gpu_ctx.set_cluster_report(True)
        try:
            got = gpu_ctx.debug_evaluate(rects, T_S, T_V, use_hc, False, mode)
        finally:
            gpu_ctx.set_cluster_report(False)
        H, E = got["hits"], got["evidence"]
        n = len(H["seed"])
        assert got["count_pass"] == {mode}
        assert n > 8192 and len(E["bases"]) == len(E["hc_bases"]) == len(E["variance"]) == n
        # the switch changes no verdict
        assert np.array_equal(np.sort(hit_keys(H)), np.sort(hit_keys(plain["hits"]))) and len(np.unique(hit_keys(H))) == n
        assert got["oversize_pairs"] == plain["oversize_pairs"] and (got["oversize_pairs"] > 0) == with_rep
        want = np.zeros((n, 2), np.int64)
        want_var = np.zeros(n, np.float64)
        oversize_hits = 0
        per_rect = np.zeros(len(rects), np.int64)
        for q in range(n):
            seeds, cands, _ = rects[int(H["rect"][q])]
            i, j = seeds[H["seed"][q]], (seeds if cands is None else cands)[H["cand"][q]]
            bases, hc, nd, var, nm = score(i, j, H["strand"][q])
            want[q] = (bases, hc)
            want_var[q] = var
            oversize_hits += nm > MCAP
            per_rect[H["rect"][q]] += 1
            mn = float(min(len(reads[i]), len(reads[j])))
            assert float(hc if use_hc else bases) / mn >= T_S and var < T_V, (mode, q)
        print(f"[report eval use_hc={int(use_hc)} {mode}] {n} hits per rectangle {per_rect.tolist()}, {oversize_hits} of them oversize pairs, "
              f"{got['oversize_pairs']} oversize pairs")
        bad = np.nonzero((E["bases"] != want[:, 0]) | (E["hc_bases"] != want[:, 1]) | (E["variance"].view(np.uint64) != want_var.view(np.uint64)))[0]
        assert len(bad) == 0, (mode, len(bad), [(int(H["rect"][b]), int(H["seed"][b]), int(H["cand"][b]), int(H["strand"][b]), int(E["bases"][b]),
                                                 int(E["hc_bases"][b]), float(E["variance"][b]), want[b].tolist(), float(want_var[b])) for b in bad[:5]])
        assert not np.isnan(E["variance"]).any()
        # every rectangle has hits, the isoform family on both strands; with the repeat reads the second verdict launch contributed
        assert (per_rect > 0).all() and (oversize_hits >= 1) == with_rep
        assert set(H["strand"][H["rect"] >= len(rects) - 2].tolist()) == {0, 1}
