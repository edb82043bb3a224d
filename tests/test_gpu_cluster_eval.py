"""One evaluation of the greedy clustering (cluster_driver.hip: the steps of evaluator::run_local) pair by pair against a plain reference, through
the test hook rattle_hip_debug_evaluate: kernel A's survivor list over many rectangles (and its capacity retry), the survivor sort,
both count passes for |common| (the seed-major LDS bit set of pair_count.hip and the per-pair search of pair_score.hip), the exact
rejection of count_bound_kernel with its per-rectangle statistics, the full pass with its oversize relaunch, and the verdicts.

The reference follows cluster_together (oracle/orc_cluster.hpp): bit vectors and k-mer lists from oracle.extract_kmers, |common| = the
sum over shared hashes of the product of their multiplicities, the score and variance of every kept pair from oracle.pair_score.  The
seed-major pass is held to its documented semantics exactly: with f = fold(h) ((h ^ h >> 20) & 0xFFFFF for k > 10, else h) and
nrep = nA - |distinct f of the seed|, a candidate k-mer contributes the seed's multiplicity of f, or 1 + nrep for every f in the seed
when nrep > 2048.  Every scenario runs with the count pass forced to "seed", to "search", and as the driver picks it."""
import numpy as np
import pytest
import scipy.sparse as sp

from rattle_amd import synth
from rattle_amd.api import Context

pytestmark = pytest.mark.gpu

MODES = ("seed", "search", "auto")
PC_REP = 2048
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def family(n, genes, seed, exon=(20, 45), both=True, isoforms=1, **kw):
    return synth.reads(n, genes, isoforms, both, seed=seed, exon=exon, **kw)[0]


class Ref:
    """The oracle's side of one loaded read set: k-mer lists, bit vectors, and per rectangle the tables of survival, |common| and
    the seed-major pass's count for every (seed, candidate, strand)."""

    def __init__(self, oracle, reads, k, both):
        self.oracle, self.reads, self.k, self.both = oracle, reads, k, both
        ex = [oracle.extract_kmers(s, k, both) for s in reads]
        self.n = len(reads)
        self.fh = [x[0].astype(np.int64) for x in ex]
        self.rh = [x[2].astype(np.int64) for x in ex] if both else None
        self.bf = np.array([x[4] for x in ex], np.uint64).reshape(self.n, 64)
        self.br = np.array([x[5] for x in ex], np.uint64).reshape(self.n, 64)
        self.pcf = np.bitwise_count(self.bf).sum(1).astype(np.int64)
        self.len = np.array([len(s) for s in reads], np.int64)
        self.fold = (lambda h: (h ^ (h >> 20)) & 0xFFFFF) if k > 10 else (lambda h: h)
        self.nrep = np.array([len(h) - len(np.unique(self.fold(h))) for h in self.fh], np.int64)
        self.raw = self._matrices(lambda h: h)
        self.folded = self._matrices(self.fold)
        self.verdicts = {}

    def _matrices(self, f):
        """sparse multiplicity matrices (read x value): forward lists, and the candidates' lists per strand"""
        lists = [f(h) for h in self.fh] + ([f(h) for h in self.rh] if self.both else [])
        allv = np.concatenate(lists + [np.zeros(1, np.int64)])
        _, inv = np.unique(allv, return_inverse=True)
        inv = inv[:-1]
        rows = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
        M = sp.csr_matrix((np.ones(len(rows), np.int64), (rows, inv)), shape=(len(lists), int(inv.max(initial=0)) + 1))
        return M[:self.n], (M[self.n:] if self.both else None)

    def tables(self, seeds, cands, thr, triangular):
        """(survives, common, seed-pass count) per strand, each [len(seeds), len(cands)]"""
        seeds = np.asarray(seeds, np.int64); cands = np.asarray(cands, np.int64)
        strands = (0, 1) if self.both else (0,)
        mmax = np.maximum(self.pcf[seeds][:, None], self.pcf[cands][None, :]).astype(np.float64)
        surv = []
        for st in strands:
            if thr == 0.0 and st == 0:
                ok = np.ones(mmax.shape, bool)                        # cluster.cpp:19: bv_threshold == 0 passes
            else:
                bvc = self.bf if st == 0 else self.br
                common = np.zeros(mmax.shape, np.int64)
                for a in range(0, len(seeds), 64):
                    common[a:a + 64] = np.bitwise_count(self.bf[seeds[a:a + 64]][:, None, :] & bvc[cands][None, :, :]).sum(2)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ok = common.astype(np.float64) / mmax >= thr
            if triangular:
                ok &= np.arange(len(cands))[None, :] > np.arange(len(seeds))[:, None]
            surv.append(ok)
        A = self.raw[0][seeds]
        Af = self.folded[0][seeds]
        ind = Af.copy(); ind.data[:] = 1
        over = self.nrep[seeds] > PC_REP
        common, seedc = [], []
        for st in strands:
            C = (self.raw[0] if st == 0 else self.raw[1])[cands]
            Cf = (self.folded[0] if st == 0 else self.folded[1])[cands]
            common.append((A @ C.T).toarray())
            s = (Af @ Cf.T).toarray()
            if over.any():
                s[over] = (ind[over] @ Cf.T).toarray() * (1 + self.nrep[seeds][over])[:, None]
            seedc.append(s)
        return surv, common, seedc

    def verdict(self, i, j, strand, t_s, t_v, use_hc):
        """cluster_together's score and variance test on one pair (cluster.cpp:20-34 / :44-58), and the oracle's |common|"""
        key = (int(i), int(j), int(strand))
        if key not in self.verdicts:
            self.verdicts[key] = self.oracle.pair_score(self.reads[i], self.reads[j], self.k, int(strand), dist_cap=1)[:5]
        bases, hc, nd, var, nm = self.verdicts[key]
        mn = float(min(len(self.reads[i]), len(self.reads[j])))
        score = float(hc if use_hc else bases) / mn
        return bool(score >= t_s and var < t_v), nm, nd


def keys(rect, seed, cand, strand):
    return ((np.asarray(rect, np.int64) << 42) | (np.asarray(seed, np.int64) << 21) | (np.asarray(cand, np.int64) << 1)
            | np.asarray(strand, np.int64))


def expected(ref, rects):
    """every survivor of the rectangle list: key, seed read, candidate read, |common|, seed-pass count"""
    out = {f: [] for f in ("key", "i", "j", "rect", "common", "seedc")}
    for r, (seeds, cands, thr) in enumerate(rects):
        tri = cands is None
        cl = seeds if tri else cands
        if len(seeds) == 0 or len(cl) == 0:
            continue
        surv, common, seedc = ref.tables(seeds, cl, thr, tri)
        for st in range(len(surv)):
            s, c = np.nonzero(surv[st])
            out["key"].append(keys(np.full(len(s), r), s, c, np.full(len(s), st)))
            out["i"].append(np.asarray(seeds, np.int64)[s]); out["j"].append(np.asarray(cl, np.int64)[c])
            out["rect"].append(np.full(len(s), r))
            out["common"].append(common[st][s, c]); out["seedc"].append(seedc[st][s, c])
    E = {f: (np.concatenate(v) if v else np.zeros(0, np.int64)) for f, v in out.items()}
    o = np.argsort(E["key"])
    return {f: v[o] for f, v in E.items()}


def n_pairs(seeds, cands):
    s = len(seeds)
    return s * (s - 1) // 2 if cands is None else s * len(cands)


def check(ctx, ref, rects, mode, t_s, t_v=1000000.0, use_hc=False, exp=None, label=""):
    """One evaluation against the reference; returns (what the hook reported, statistics of what the reference saw)."""
    k = ref.k
    if exp is None:
        exp = expected(ref, rects)
    got = ctx.debug_evaluate(rects, t_s, t_v, use_hc, not ref.both, mode)
    S = got["survivors"]
    gk = keys(S["rect"], S["seed"], S["cand"], S["strand"])
    o = np.argsort(gk)
    gk, cnt = gk[o], S["count"][o].astype(np.int64)
    # kernel A: exactly the expected survivors, each once
    assert len(gk) == len(exp["key"]) and np.array_equal(gk, exp["key"]), (label, mode, len(gk), len(exp["key"]))
    ran = got["count_pass"]
    if len(gk):
        assert len(ran) == 1 and (mode == "auto" or ran == {mode}), (label, mode, ran)
    # the count pass: never below |common| (what the rejection relies on), and exactly what the pass that ran is documented to give
    assert (cnt >= exp["common"]).all(), (label, mode, np.nonzero(cnt < exp["common"])[0][:5])
    want = exp["seedc"] if ran == {"seed"} else exp["common"]
    bad = np.nonzero(cnt != want)[0]
    assert len(bad) == 0, (label, mode, ran, [(int(exp["i"][b]), int(exp["j"][b]), int(exp["key"][b] & 1), int(cnt[b]), int(want[b]),
                                               int(exp["common"][b])) for b in bad[:5]])
    # count_bound_kernel: the kept pairs are the survivors with double(k * count) / min_len >= t_s, from the device's own count
    mn = np.minimum(ref.len[exp["i"]], ref.len[exp["j"]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (cnt * k).astype(np.float64) / mn
    keep = v >= t_s
    K = got["kept"]
    kk = np.sort(keys(K["rect"], K["seed"], K["cand"], K["strand"]))
    assert np.array_equal(kk, exp["key"][keep]), (label, mode, len(kk), int(keep.sum()))
    # the full pass and the verdicts: the hits are the kept pairs cluster_together accepts (a rejected count cannot be accepted:
    # tests/test_count_bound_lemma.py), whatever the count pass
    want_hits, nd1, big = [], 0, 0
    for q in np.nonzero(keep)[0]:
        ok, nm, nd = ref.verdict(exp["i"][q], exp["j"][q], exp["key"][q] & 1, t_s, t_v, use_hc)
        assert nm == exp["common"][q], (label, q, nm, exp["common"][q])
        if ok:
            want_hits.append(exp["key"][q])
        nd1 += nd == 1
        big += nm > 400
    H = got["hits"]
    hk = np.sort(keys(H["rect"], H["seed"], H["cand"], H["strand"]))
    assert len(np.unique(hk)) == len(hk)
    assert np.array_equal(hk, np.sort(np.array(want_hits, np.int64))), (label, mode, len(hk), len(want_hits))
    # per-rectangle counters: [0] pairs, [1] survivors, [2] summed counts, [5] kept
    for r, (seeds, cands, thr) in enumerate(rects):
        m = exp["rect"] == r
        want_c = (n_pairs(seeds, cands) if len(seeds) and (cands is None or len(cands)) else 0, int(m.sum()), int(cnt[m].sum()),
                  int((keep & m).sum()))
        c = got["counters"][r]
        assert (int(c[0]), int(c[1]), int(c[2]), int(c[5])) == want_c, (label, mode, r, c, want_c)
    at_bar = int((v[keep] == t_s).sum())
    stats = {"survivors": len(gk), "kept": int(keep.sum()), "hits": len(hk), "pass": sorted(ran), "at_t_s": at_bar,
             "nd1_kept": nd1, "big_kept": big, "filter_launches": got["filter_launches"], "oversize": got["oversize_pairs"],
             "over_count": int((cnt > exp["common"]).sum())}
    print(f"[{label}] count pass {mode:6s} -> {stats}")
    return got, stats


def boundary_t_s(ref, exp, lo):
    """the smallest double(k * |common|) / min_len >= lo of a survivor that both count passes count exactly: t_s on the exact bar
    of a pair"""
    mn = np.minimum(ref.len[exp["i"]], ref.len[exp["j"]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (exp["common"] * ref.k).astype(np.float64) / mn
    v = v[np.isfinite(v) & (v >= lo) & (exp["seedc"] == exp["common"])]
    return float(v.min()) if len(v) else lo


# ---- rectangle lists ------------------------------------------------------------------------------------------------------------
def rectangle_list(rng, n):
    """dozens of rectangles: the shapes around kernel A's 32 x 256 tile, triangular ones, empty ones in between, several thresholds"""
    thr = [0.0, 0.35000000000000003, 0.2, 0.4, 0.1, 0.20000000000000007]
    ids = lambda m: rng.choice(n, m, replace=m > n).astype(np.uint32)
    shapes = [(1, 1), (1, 257), (33, 1), (31, 255), (32, 256), (33, 257), (2, 3), (5, 7), (1, 2), (3, 1), (64, 65), (17, 130),
              (1, 1), (2, 2), (7, 1), (1, 64), (9, 9)]
    rects = []
    for t, (a, b) in enumerate(shapes):
        rects.append((ids(a), ids(b), thr[t % len(thr)]))
        if t % 4 == 1:
            rects.append((ids(0), ids(5), thr[(t + 1) % len(thr)]))                     # empty: no seeds
            rects.append((ids(3), ids(0), thr[(t + 2) % len(thr)]))                     # empty: no candidates
        if t % 4 == 3:
            rects.append((np.sort(ids(2 + t)), None, thr[(t + 3) % len(thr)]))
    for m in (1, 2, 33, 65):                                                            # triangular (level 1 of a greedy round)
        rects.append((np.sort(ids(m)), None, thr[m % len(thr)]))
    rects.append((ids(0), None, 0.0))
    return rects


@pytest.mark.parametrize("both", [True, False], ids=["cdna", "rna"])
@pytest.mark.parametrize("k", [3, 6, 10, 11, 16])
def test_rectangle_lists(gpu_ctx, oracle, k, both):
    """k < 6 (no 6-mer prefilter), k <= 10 (exact bit set), k > 10 (folded hash); both strands and one (bv_filter_kernel<false>).
    Small rectangles put rectangle boundaries inside one wavefront of count_bound_kernel; t_s sits on the exact bar of a pair."""
    rng = np.random.default_rng(70 + k + 100 * both)
    reads = family(240, 30, 500 + k, both=both) + [b"", rnd(rng, k - 1), rnd(rng, k), rnd(rng, k + 1), rnd(rng, 40)]
    ref = Ref(oracle, reads, k, both)
    gpu_ctx.load_reads(reads, k, both)
    rects = rectangle_list(rng, len(reads))
    exp = expected(ref, rects)
    # t_s on the exact bar of a pair; for k < 10 every related pair's bar is far above any score, so there a plain 0.3
    t_s = boundary_t_s(ref, exp, 0.3) if k >= 10 else 0.3
    seen = set()
    for mode in MODES:
        _, st = check(gpu_ctx, ref, rects, mode, t_s, exp=exp, label=f"rects k={k} {'cdna' if both else 'rna'}")
        assert st["hits"] > 0
        if k >= 10:
            assert st["at_t_s"] >= 1 and 0 < st["kept"] < st["survivors"]
        seen |= set(st["pass"])
    assert seen == {"seed", "search"}


# ---- the seed-major kernel ------------------------------------------------------------------------------------------------------
def fold_twin(kmer: bytes, k):
    """a k-mer whose hash differs from kmer's and whose 20-bit fold is the same (k > 10), or None"""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    h = 0
    for b in kmer:
        h = (h << 2) | code[b]
    f = (h ^ (h >> 20)) & 0xFFFFF
    for i in range(k):
        for j in range(k):
            for x in range(1, 4):
                for y in range(4):
                    g = h ^ (x << (2 * (k - 1 - i)))
                    g = (g & ~(3 << (2 * (k - 1 - j)))) | (y << (2 * (k - 1 - j))) if j != i else g
                    if g != h and ((g ^ (g >> 20)) & 0xFFFFF) == f:
                        return bytes(b"ACGT"[(g >> (2 * (k - 1 - t))) & 3] for t in range(k))
    return None


@pytest.mark.parametrize("k,both", [(10, True), (11, True), (16, False)])
def test_seed_major_edges(gpu_ctx, oracle, k, both):
    """Homopolymer seeds of k + 2048 .. k + 2050 bases (nrep = 2047 / 2048 / 2049: 2048 is the last exact repeat list), a periodic
    seed far past it, candidates of 0, 1, 63 .. 513 k-mers (every loop of the streaming code), reads of length <= k on both sides, a
    seed whose survivors span several 512-pair workgroups, many one-survivor seeds, and for k > 10 candidates whose k-mers fold onto
    the seed's with other hashes."""
    rng = np.random.default_rng(300 + k)
    fam = family(700, 40, 900 + k, both=both)
    n_list = (0, 1, 63, 64, 65, 192, 193, 448, 449, 512, 513)
    homo = [b"C" * (k + 2048), b"C" * (k + 2049), b"C" * (k + 2050)]     # (C: a hash that is not 0, what stale LDS may hold)
    # the same repeat counts beside distinct k-mers, where an overflowing list (1 + nrep per hit) and the exact count differ
    uniq = rnd(rng, 400)
    h0 = oracle.extract_kmers(uniq + b"C" * (k + 1), k, False)[0]
    base_nrep = len(h0) - len(np.unique(h0))
    homo += [uniq + b"C" * (k + 1 + want - base_nrep) for want in (2047, 2048, 2049)]
    periodic = [b"ACGGT" * 2000]
    homo_c = [b"C" * (k + m) for m in n_list] + [b"C" * 30 + rnd(rng, k + m) for m in n_list] + [uniq[50:300], uniq[:k + 5] + b"C" * 40]
    mixed_c = [fam[m % len(fam)][: k + m] if len(fam[m % len(fam)]) >= k + m else (fam[0] * 3)[: k + m] for m in n_list]
    mixed_c += [(b"ACGGT" * 120)[: k + m] for m in n_list]
    short = [b"", rnd(rng, k - 3), rnd(rng, k), b"A" * k, b"A" * (k + 1)]
    twins = []
    if k > 10:                                                          # folded collisions with the first family reads
        for s in fam[:20]:
            parts = []
            for p in range(0, min(len(s) - k, 200), 17):
                t = fold_twin(s[p:p + k], k)
                if t:
                    parts.append(t + rnd(rng, 3))
            twins.append(b"".join(parts))
    reads = fam + homo + periodic + homo_c + mixed_c + short + twins
    F = np.arange(len(fam), dtype=np.uint32)
    H = np.arange(len(fam), len(fam) + 6, dtype=np.uint32)
    P = np.array([len(fam) + 6], np.uint32)
    b0 = len(fam) + 7
    HC = np.arange(b0, b0 + len(homo_c), dtype=np.uint32)
    MC = np.arange(b0 + len(homo_c), b0 + len(homo_c) + len(mixed_c), dtype=np.uint32)
    SH = np.arange(MC[-1] + 1, MC[-1] + 1 + len(short), dtype=np.uint32)
    TW = np.arange(SH[-1] + 1, SH[-1] + 1 + len(twins), dtype=np.uint32)
    rects = [
        (H, HC, 0.0),                                                   # the repeat-list limit, every candidate length
        (np.concatenate([H, P]), MC, 0.0),
        (P, np.concatenate([HC, MC]), 0.0),
        (F[:1], F[1:], 0.0),                                            # one seed, > 512 survivors: several workgroups
        (F[:400], F[400:401], 0.0),                                     # one survivor (per strand) for each of many seeds
        (np.concatenate([SH, F[:3]]), np.concatenate([SH, F[3:40], MC]), 0.0),     # reads of length <= k on both sides
        (F[:40], F[40:300], 0.2),
    ]
    if k > 10:
        rects.append((F[:20], TW, 0.0))
    ref = Ref(oracle, reads, k, both)
    gpu_ctx.load_reads(reads, k, both)
    exp = expected(ref, rects)
    # no kept pairs: the homopolymer pairs would each cost the oracle millions of matches; kept pairs and verdicts are tested elsewhere
    t_s = 1e9
    nrep = ref.nrep[H]
    assert list(nrep) == [2047, 2048, 2049] * 2 and ref.nrep[P[0]] > 4 * PC_REP
    assert [len(ref.fh[c]) for c in HC[:len(n_list)]] == list(n_list)
    over = exp["seedc"] > exp["common"]
    collide = 0
    if k > 10:
        m = np.isin(exp["j"], TW) & over
        collide = int(m.sum())
        assert collide >= 10, collide                                  # the folded collisions are there
    for mode in MODES:
        _, st = check(gpu_ctx, ref, rects, mode, t_s, exp=exp, label=f"seed-major edges k={k}")
        if mode == "seed":
            assert st["over_count"] == int(over.sum()) and st["over_count"] > 0
    print(f"[seed-major edges k={k}] nrep of the homopolymer (and mixed) seeds {[int(x) for x in nrep]}, periodic seed {int(ref.nrep[P[0]])}; "
          f"pairs the seed pass overcounts: {int(over.sum())} (folded collisions with other hashes: {collide})")


# ---- the survivor sort ----------------------------------------------------------------------------------------------------------
def test_survivor_sort_paths(gpu_ctx, oracle):
    """More than 16 384 survivors (several sort blocks) of 1 025 .. 8 192 seeds (a multi-block scan), and more than 8 192 seeds (the
    global-atomic histogram); short reads keep the oracle cheap."""
    reads = family(9400, 300, 41, exon=(15, 22))
    ref = Ref(oracle, reads, 10, True)
    gpu_ctx.load_reads(reads, 10, True)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(reads)).astype(np.uint32)
    cases = [("2000 seeds", [(perm[:2000], perm[2000:2012], 0.0)]),
             ("9000 seeds", [(perm[:4500], perm[9000:9002], 0.0), (perm[4500:9000], perm[9002:9004], 0.0)])]
    for label, rects in cases:
        exp = expected(ref, rects)
        ns = sum(len(r[0]) for r in rects)
        assert len(exp["key"]) > 16384 and ns > 1024
        t_s = boundary_t_s(ref, exp, 0.3)
        for mode in MODES:
            _, st = check(gpu_ctx, ref, rects, mode, t_s, exp=exp, label=f"survivor sort, {label}")
            assert st["hits"] > 0


# ---- the per-pair search --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 11])
def test_search_pass_swap_and_long_lists(gpu_ctx, oracle, k):
    """The count pass walks the shorter list: a long seed against short candidates swaps (nA > nB), a short seed against long
    candidates does not; the long side's list has more than 2 048 entries (searched in global memory, not LDS)."""
    rng = np.random.default_rng(600 + k)
    longs = [rnd(rng, int(rng.integers(2600, 3900))) for _ in range(5)]
    frags = []
    for L in longs:
        for flen in (150, 300, 450):
            a = int(rng.integers(0, len(L) - flen))
            f = L[a:a + flen]
            frags.append(f if len(frags) % 2 else revcomp(f))
            frags.append(f[:80] + f[40:])                               # an internal repeat: cross products
    others = family(40, 5, 77 + k)
    reads = longs + frags + others
    nl, nf = len(longs), len(frags)
    Lg = np.arange(nl, dtype=np.uint32); Fr = np.arange(nl, nl + nf, dtype=np.uint32)
    Ot = np.arange(nl + nf, len(reads), dtype=np.uint32)
    rects = [(Lg, np.concatenate([Fr, Ot]), 0.0), (Fr, Lg, 0.0), (Lg, None, 0.0), (Fr, Lg, 0.1), (Ot, Lg, 0.0)]
    ref = Ref(oracle, reads, k, True)
    gpu_ctx.load_reads(reads, k, True)
    exp = expected(ref, rects)
    nA = np.array([len(ref.fh[i]) for i in exp["i"]]); nB = np.array([len(ref.fh[j]) for j in exp["j"]])
    assert ((nA > nB) & (nA > 2048)).sum() > 50 and ((nA < nB) & (nB > 2048)).sum() > 50
    for mode in MODES:
        _, st = check(gpu_ctx, ref, rects, mode, 0.3, exp=exp, label=f"search k={k}")
        assert st["hits"] > 0


# ---- the full pass and the verdicts ---------------------------------------------------------------------------------------------
def test_verdicts_oversize_and_many_hits(gpu_ctx, oracle):
    """use_hc 0 and 1; a finite t_v with pairs of one distance (variance NaN: rejected); pairs past the LDS match capacity, accepted and
    rejected, so that the oversize relaunch and its second verdict add hits; more than 8 192 hits in one evaluation."""
    rng = np.random.default_rng(11)
    same = family(110, 1, 12, exon=(30, 40), both=False, sub=0.01, ins=0.005, dele=0.005)     # one transcript, one strand
    iso = family(200, 6, 13, isoforms=3)                                # exon skips: large variances
    one = []                                                            # 30 nt pairs sharing one 11-mer: two matches, one distance
    for _ in range(40):
        seg = rnd(rng, 11)
        a, b = int(rng.integers(0, 19)), int(rng.integers(0, 19))
        one += [rnd(rng, a) + seg + rnd(rng, 19 - a), rnd(rng, b) + seg + rnd(rng, 19 - b)]
    rep = [b"AC" * 640, b"CA" * 640 + b"GGT", b"AC" * 400 + rnd(rng, 400), b"AC" * 250 + rnd(rng, 2000)]
    reads = same + iso + one + rep
    S = np.arange(len(same), dtype=np.uint32)
    I = np.arange(len(same), len(same) + len(iso), dtype=np.uint32)
    O = np.arange(I[-1] + 1, I[-1] + 1 + len(one), dtype=np.uint32)
    R = np.arange(O[-1] + 1, O[-1] + 1 + len(rep), dtype=np.uint32)
    ref = Ref(oracle, reads, 10, True)
    gpu_ctx.load_reads(reads, 10, True)
    # many hits, and the repeat reads past the LDS capacity: t_s 0.5 accepts some of them and rejects others
    rects = [(S[:100], S, 0.0), (R, R[::-1].copy(), 0.0), (R[:2], None, 0.0)]
    exp = expected(ref, rects)
    for mode in MODES:
        got, st = check(gpu_ctx, ref, rects, mode, 0.5, exp=exp, label="many hits + oversize")
        assert st["hits"] > 8192 and got["oversize_pairs"] > 0
    over = [(i, j, s) for (i, j, s), v in ref.verdicts.items() if v[4] > 400 and i in R and j in R]
    acc = sum(ref.verdict(i, j, s, 0.5, 1e6, False)[0] for i, j, s in over)
    assert 0 < acc < len(over), (acc, len(over))
    print(f"[oversize] {len(over)} kept repeat pairs past the LDS match capacity, {acc} of them accepted")
    # use_hc and a finite t_v; the one-distance pairs reach the variance test with NaN
    rects = [(O[0::2], O[1::2], 0.0), (I[:60], I[60:], 0.2), (I[:30], None, 0.1), (np.concatenate([I[:10], O[:10]]), None, 0.0)]
    exp = expected(ref, rects)
    hits = {}
    for use_hc in (False, True):
        for mode in MODES:
            got, st = check(gpu_ctx, ref, rects, mode, 0.3, 25.0, use_hc, exp=exp, label=f"verdicts use_hc={int(use_hc)} t_v=25")
            assert st["nd1_kept"] >= 5
            hits.setdefault(use_hc, []).append(st["hits"])
    assert len(set(hits[False])) == 1 and len(set(hits[True])) == 1
    nan_scored = sum(1 for (i, j, s), v in ref.verdicts.items() if v[2] == 1 and np.isnan(v[3])
                     and float(v[0]) / min(len(reads[i]), len(reads[j])) >= 0.3)
    assert nan_scored >= 3          # pairs that pass the score and are rejected on the NaN variance alone
    # t_s = 0 with empty reads: 0 / 0 is NaN, never kept, never accepted
    reads0 = family(30, 3, 14) + [b"", b"", b"ACGT"]
    ref0 = Ref(oracle, reads0, 10, True)
    gpu_ctx.load_reads(reads0, 10, True)
    rects = [(np.arange(len(reads0), dtype=np.uint32), None, 0.0), (np.array([30, 31], np.uint32), np.arange(33, dtype=np.uint32), 0.0)]
    for mode in MODES:
        check(gpu_ctx, ref0, rects, mode, 0.0, label="t_s = 0, empty reads")


# ---- the survivor-capacity retry ------------------------------------------------------------------------------------------------
def test_capacity_retry(oracle):
    """The first evaluation of a fresh context leaves 2.2 M survivors (1 100 x 1 000 short reads at thr = 0, both strands), more than
    the survivor list starts with (2^20 entries, as reserve() rounds it: 1.3 M): kernel A runs again with room for all of them, and
    nothing is lost."""
    reads = family(2100, 150, 61, exon=(15, 22))
    ref = Ref(oracle, reads, 10, True)
    rects = [(np.arange(1100, dtype=np.uint32), np.arange(1100, 2100, dtype=np.uint32), 0.0)]
    exp = expected(ref, rects)
    assert len(exp["key"]) > (1 << 20)
    for mode in MODES:
        ctx = Context(0)
        try:
            ctx.load_reads(reads, 10, True)
            got, st = check(ctx, ref, rects, mode, 0.3, exp=exp, label="capacity retry")
            assert got["filter_launches"] == 2 and st["hits"] > 0
            got = ctx.debug_evaluate(rects, 0.3, count_pass=mode)      # the grown list is kept: one launch now
            assert got["filter_launches"] == 1 and len(got["survivors"]["seed"]) == len(exp["key"])
        finally:
            ctx.close()
