"""The "index" count pass (pair_index.hip: an inverted k-mer index over the seeds of one evaluation, every candidate's hash list
streamed once) pair by pair against the plain reference of tests/test_gpu_cluster_eval.py, through rattle_hip_debug_evaluate with
the pass forced to "index".

What the pass is held to, for every survivor of kernel A:
  k <= 10: its count is exactly |common|;
  k >  10: its count is the sum over the candidate's k-mers b of the multiplicity of fold(hash(b)) among the seed's folded hashes
           (Ref.folded: Af @ Cf.T, WITHOUT the repeat-list overflow branch of the seed-major pass), and never below |common|.
Everything behind the count is compared with the same evaluation forced to "search": counters [0] [1], the hits, and the kept pairs
with counter [5].  For k <= 10 the two counts are the same number, so the kept pairs are the same set.  For k > 10 the index count
of a pair whose k-mers fold onto the seed's with OTHER hashes lies above |common|: where the reference side shows such a pair on
the other side of the bar t_s (`straddle` below), the index pass must keep exactly the search pass's pairs plus those, and the full
comparison must still reject them -- the hits are equal in every case.  Counter [2] is the sum of the counts.

Every scenario asserts from the reference side (computed on the CPU) that it holds the work it is named for."""
import numpy as np
import pytest

from rattle_amd import synth  # noqa: F401  (the generators below come from the cluster-evaluation tests)
from test_gpu_cluster_eval import PC_REP, Ref, expected, family, fold_twin, keys, n_pairs, rectangle_list, revcomp, rnd

pytestmark = pytest.mark.gpu


def expected_ix(ref, rects):
    """expected() of the cluster-evaluation tests plus "indexc": the index pass's documented count of every survivor"""
    E = expected(ref, rects)
    out = []
    strands = (0, 1) if ref.both else (0,)
    for r, (seeds, cands, thr) in enumerate(rects):
        cl = seeds if cands is None else cands
        if len(seeds) == 0 or len(cl) == 0:
            continue
        surv = ref.tables(seeds, cl, thr, cands is None)[0]
        Af = ref.folded[0][np.asarray(seeds, np.int64)]
        for st in strands:
            Cf = (ref.folded[0] if st == 0 else ref.folded[1])[np.asarray(cl, np.int64)]
            s, c = np.nonzero(surv[st])
            prod = (Af @ Cf.T).toarray()
            out.append((keys(np.full(len(s), r), s, c, np.full(len(s), st)), prod[s, c]))
    key = np.concatenate([o[0] for o in out]) if out else np.zeros(0, np.int64)
    val = np.concatenate([o[1] for o in out]) if out else np.zeros(0, np.int64)
    o = np.argsort(key)
    assert np.array_equal(key[o], E["key"])
    E["indexc"] = val[o]
    if ref.k <= 10:
        assert np.array_equal(E["indexc"], E["common"])            # no fold: the two definitions are one
    return E


def sorted_keys(P):
    return np.sort(keys(P["rect"], P["seed"], P["cand"], P["strand"]))


def check_index(ctx, ref, rects, t_s, t_v=1000000.0, use_hc=False, exp=None, label=""):
    k = ref.k
    if exp is None:
        exp = expected_ix(ref, rects)
    got = ctx.debug_evaluate(rects, t_s, t_v, use_hc, not ref.both, "index")
    S = got["survivors"]
    gk = keys(S["rect"], S["seed"], S["cand"], S["strand"])
    o = np.argsort(gk)
    gk, cnt = gk[o], S["count"][o].astype(np.int64)
    assert len(gk) == len(exp["key"]) and np.array_equal(gk, exp["key"]), (label, len(gk), len(exp["key"]))
    if len(gk):
        assert got["count_pass"] == {"index"}, (label, got["count_pass"])
    # the count: never below |common|, and exactly the documented number
    assert (cnt >= exp["common"]).all(), (label, np.nonzero(cnt < exp["common"])[0][:5])
    want = exp["common"] if k <= 10 else exp["indexc"]
    bad = np.nonzero(cnt != want)[0]
    assert len(bad) == 0, (label, len(bad), [(int(exp["i"][b]), int(exp["j"][b]), int(exp["key"][b] & 1), int(cnt[b]), int(want[b]),
                                              int(exp["common"][b])) for b in bad[:5]])
    # count_bound_kernel on the device's own count
    mn = np.minimum(ref.len[exp["i"]], ref.len[exp["j"]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (cnt * k).astype(np.float64) / mn
        v_common = (exp["common"] * k).astype(np.float64) / mn
    keep = v >= t_s
    kk = sorted_keys(got["kept"])
    assert np.array_equal(kk, exp["key"][keep]), (label, len(kk), int(keep.sum()))
    # the full pass and the verdicts: the hits are the kept pairs the reference's cluster_together accepts
    want_hits = []
    for q in np.nonzero(keep)[0]:
        ok, nm, _ = ref.verdict(exp["i"][q], exp["j"][q], exp["key"][q] & 1, t_s, t_v, use_hc)
        assert nm == exp["common"][q], (label, q, nm, exp["common"][q])
        if ok:
            want_hits.append(exp["key"][q])
    hk = sorted_keys(got["hits"])
    assert len(np.unique(hk)) == len(hk)
    assert np.array_equal(hk, np.sort(np.array(want_hits, np.int64))), (label, len(hk), len(want_hits))
    for r, (seeds, cands, thr) in enumerate(rects):
        m = exp["rect"] == r
        want_c = (n_pairs(seeds, cands) if len(seeds) and (cands is None or len(cands)) else 0, int(m.sum()), int(cnt[m].sum()),
                  int((keep & m).sum()))
        c = got["counters"][r]
        assert (int(c[0]), int(c[1]), int(c[2]), int(c[5])) == want_c, (label, r, c, want_c)
    # the same evaluation through the per-pair search
    srch = ctx.debug_evaluate(rects, t_s, t_v, use_hc, not ref.both, "search")
    assert not len(gk) or srch["count_pass"] == {"search"}
    straddle = keep & ~(v_common >= t_s)             # kept on a folded collision only (k > 10); the reference side says which
    assert k > 10 or not straddle.any()
    sk = sorted_keys(srch["kept"])
    assert np.array_equal(sk, exp["key"][keep & ~straddle]), (label, len(sk), int(keep.sum()), int(straddle.sum()))
    assert np.array_equal(sorted_keys(srch["hits"]), hk), label
    assert np.array_equal(srch["counters"][:, [0, 1]], got["counters"][:, [0, 1]]), label
    for r in range(len(rects)):
        assert int(got["counters"][r][5]) == int(srch["counters"][r][5]) + int((straddle & (exp["rect"] == r)).sum()), (label, r)
    if not straddle.any():
        assert np.array_equal(kk, sk) and np.array_equal(srch["counters"][:, 5], got["counters"][:, 5])
    stats = {"survivors": len(gk), "kept": int(keep.sum()), "hits": len(hk), "above_common": int((cnt > exp["common"]).sum()),
             "kept_on_collisions_only": int(straddle.sum())}
    print(f"[{label}] index pass -> {stats}")
    return got, stats


def bar_t_s(ref, exp, lo):
    """t_s on the exact bar of a pair: the smallest double(k * |common|) / min_len >= lo"""
    mn = np.minimum(ref.len[exp["i"]], ref.len[exp["j"]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (exp["common"] * ref.k).astype(np.float64) / mn
    v = v[np.isfinite(v) & (v >= lo)]
    return float(v.min()) if len(v) else lo


@pytest.mark.parametrize("both", [True, False], ids=["cdna", "rna"])
@pytest.mark.parametrize("k", [3, 6, 10, 11, 16])
def test_index_rectangle_lists(gpu_ctx, oracle, k, both):
    """Dozens of rectangles in one evaluation (one index over the seeds of all of them: a candidate must only count the seeds of its
    own rectangle), triangular and empty ones among them, every k class, both strands and one."""
    rng = np.random.default_rng(170 + k + 100 * both)
    reads = family(240, 30, 500 + k, both=both) + [b"", rnd(rng, k - 1), rnd(rng, k), rnd(rng, k + 1), rnd(rng, 40)]
    ref = Ref(oracle, reads, k, both)
    gpu_ctx.load_reads(reads, k, both)
    rects = rectangle_list(rng, len(reads)) + rectangle_list(rng, len(reads))
    exp = expected_ix(ref, rects)
    tri = [r for r, (s, c, t) in enumerate(rects) if c is None and (exp["rect"] == r).any()]
    empty = [r for r, (s, c, t) in enumerate(rects) if len(s) == 0 or (c is not None and len(c) == 0)]
    assert len(rects) >= 40 and len(exp["key"]) >= 1000 and len(tri) >= 4 and len(empty) >= 4
    assert len(np.unique(exp["rect"])) >= 30                       # survivors in (nearly) every rectangle that has pairs
    t_s = bar_t_s(ref, exp, 0.3) if k >= 10 else 0.3
    _, st = check_index(gpu_ctx, ref, rects, t_s, exp=exp, label=f"rects k={k} {'cdna' if both else 'rna'}")
    assert st["hits"] > 0
    if k >= 10:
        assert 0 < st["kept"] < st["survivors"]


@pytest.mark.parametrize("k,both", [(6, False), (10, True), (11, True), (16, False)])
def test_index_low_complexity_and_fold_twins(gpu_ctx, oracle, k, both):
    """Seeds whose repeats exceed the seed-major pass's 2048-entry repeat list (homopolymers, a periodic read): the seed-major count
    is an over-count there, the index count must be exact for k <= 10 and the plain folded sum for k > 10.  Candidates of 0, 1, 63 ..
    513 k-mers (every loop of the streaming code), reads of length <= k on both sides.  For k > 10, candidates built from k-mers that
    fold onto the seeds' with other hashes: counted above |common|, kept by the bound, rejected by the full comparison."""
    rng = np.random.default_rng(1300 + k)
    fam = family(300, 20, 900 + k, both=both)
    n_list = (0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 512, 513)
    uniq = rnd(rng, 400)
    h0 = oracle.extract_kmers(uniq + b"C" * (k + 1), k, False)[0]
    base_nrep = len(h0) - len(np.unique(h0))
    homo = [b"C" * (k + 2050), b"C" * (k + 2600), uniq + b"C" * (k + 1 + 2100 - base_nrep)]
    periodic = [b"ACGGT" * 2000]
    homo_c = [b"C" * (k + m) for m in n_list] + [b"C" * 30 + rnd(rng, k + m) for m in n_list] + [uniq[50:300], uniq[:k + 5] + b"C" * 40]
    mixed_c = [(b"ACGGT" * 120)[: k + m] for m in n_list] + [fam[m % len(fam)][: k + m] for m in (0, 1, 63, 64, 65)]
    short = [b"", rnd(rng, max(k - 3, 0)), rnd(rng, k), b"A" * k, b"A" * (k + 1)]
    twins = []
    if k > 10:
        for s in fam[:20]:
            parts = []
            for p in range(0, min(len(s) - k, 200), 17):
                t = fold_twin(s[p:p + k], k)
                if t:
                    parts.append(t + rnd(rng, 3))
            twins.append(b"".join(parts))
    reads = fam + homo + periodic + homo_c + mixed_c + short + twins
    F = np.arange(len(fam), dtype=np.uint32)
    H = np.arange(len(fam), len(fam) + 3, dtype=np.uint32)
    P = np.array([len(fam) + 3], np.uint32)
    b0 = len(fam) + 4
    HC = np.arange(b0, b0 + len(homo_c), dtype=np.uint32)
    MC = np.arange(HC[-1] + 1, HC[-1] + 1 + len(mixed_c), dtype=np.uint32)
    SH = np.arange(MC[-1] + 1, MC[-1] + 1 + len(short), dtype=np.uint32)
    TW = np.arange(SH[-1] + 1, SH[-1] + 1 + len(twins), dtype=np.uint32)
    rects = [
        (H, HC, 0.0),
        (np.concatenate([H, P]), MC, 0.0),
        (P, np.concatenate([HC, MC]), 0.0),
        (np.concatenate([H, P, F[:5]]), None, 0.0),                      # the low-complexity seeds are candidates too
        (np.concatenate([SH, F[:3]]), np.concatenate([SH, F[3:40], MC]), 0.0),
        (F[:40], F[40:300], 0.2),
    ]
    ref = Ref(oracle, reads, k, both)
    gpu_ctx.load_reads(reads, k, both)
    exp = expected_ix(ref, rects)
    assert (ref.nrep[H] > PC_REP).all() and ref.nrep[P[0]] > 4 * PC_REP, (ref.nrep[H], ref.nrep[P[0]])
    assert [len(ref.fh[c]) for c in HC[:len(n_list)]] == list(n_list)
    over = exp["seedc"] > exp["indexc"]
    assert over.sum() >= 20, over.sum()                                 # pairs the seed-major pass over-counts and this one must not
    # no kept pairs here: the homopolymer pairs would each cost the oracle millions of matches
    got, st = check_index(gpu_ctx, ref, rects, 1e9, exp=exp, label=f"low complexity k={k}")
    assert st["kept"] == 0 and (k > 10 or st["above_common"] == 0)
    if k > 10:
        rects = [(F[:20], TW, 0.0), (F[20:30], F[30:80], 0.0)]
        exp = expected_ix(ref, rects)
        twin = (exp["rect"] == 0) & (exp["indexc"] > exp["common"])
        assert twin.sum() >= 10, twin.sum()                             # the folded collisions are there
        _, st = check_index(gpu_ctx, ref, rects, 0.3, exp=exp, label=f"fold twins k={k}")
        assert st["above_common"] >= twin.sum() and st["kept_on_collisions_only"] >= 1 and st["hits"] > 0


def test_index_seed_chunks(gpu_ctx, oracle):
    """Rectangles with more seeds than a wavefront's counter array holds (1024): 2100 seeds x 40 candidates beside a triangular
    rectangle of 1300 seeds (every candidate slot of it counts a different prefix of the seed chunks) and a small one."""
    reads = family(2600, 120, 41, exon=(15, 22))
    ref = Ref(oracle, reads, 10, True)
    gpu_ctx.load_reads(reads, 10, True)
    perm = np.random.default_rng(5).permutation(len(reads)).astype(np.uint32)
    rects = [(perm[:2100], perm[2100:2140], 0.0), (np.sort(perm[200:1500]), None, 0.3), (perm[2140:2150], perm[2150:2600], 0.1)]
    exp = expected_ix(ref, rects)
    for r, floor in ((0, 100000), (1, 2000), (2, 100)):
        assert (exp["rect"] == r).sum() >= floor, (r, int((exp["rect"] == r).sum()))
    seed_of = (exp["key"] >> 21) & ((1 << 21) - 1)
    for r in (0, 1):                                                     # survivors with a positive count in every seed chunk
        for lo in range(0, len(rects[r][0]), 1024):
            m = (exp["rect"] == r) & (seed_of >= lo) & (seed_of < lo + 1024) & (exp["common"] > 0)
            assert m.sum() >= 50, (r, lo, int(m.sum()))
    _, st = check_index(gpu_ctx, ref, rects, bar_t_s(ref, exp, 0.3), exp=exp, label="seed chunks")
    assert st["hits"] > 0 and st["kept"] > 0


@pytest.mark.parametrize("both", [True, False], ids=["cdna", "rna"])
def test_index_long_candidate(gpu_ctx, oracle, both):
    """A candidate of 20 kb (and seeds of 2 - 4 kb cut from it, some reverse-complemented, some with an internal repeat) at k = 10."""
    rng = np.random.default_rng(2000 + both)
    big = rnd(rng, 20000)
    longs = [rnd(rng, int(rng.integers(2600, 3900))) for _ in range(3)]
    frags = []
    for n, flen in enumerate((2000, 3000, 4000, 300, 450)):
        a = int(rng.integers(0, len(big) - flen))
        f = big[a:a + flen]
        frags.append(revcomp(f) if both and n % 2 else f)
    frags.append(big[500:900] + big[700:1400])                           # an internal repeat: cross products
    others = family(30, 4, 77, both=both)
    reads = [big] + longs + frags + others
    B = np.array([0], np.uint32)
    Lg = np.arange(1, 4, dtype=np.uint32)
    Fr = np.arange(4, 4 + len(frags), dtype=np.uint32)
    Ot = np.arange(4 + len(frags), len(reads), dtype=np.uint32)
    rects = [(np.concatenate([Fr, Lg]), np.concatenate([B, Ot, Lg]), 0.0), (B, np.concatenate([Fr, Ot]), 0.0), (np.concatenate([B, Fr]), None, 0.0)]
    ref = Ref(oracle, reads, 10, both)
    gpu_ctx.load_reads(reads, 10, both)
    exp = expected_ix(ref, rects)
    long_c = (exp["j"] == 0) & (exp["common"] > 250)
    assert len(ref.fh[0]) >= 19990 and long_c.sum() >= 5             # the 20 kb list as a candidate of seeds that share hundreds of k-mers
    _, st = check_index(gpu_ctx, ref, rects, 0.3, exp=exp, label=f"20 kb candidate {'cdna' if both else 'rna'}")
    assert st["hits"] >= 5
