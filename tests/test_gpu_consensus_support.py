"""The report form of kernel D's mode 2 (csrc/post_msa.hip, post_msa_kernel<2, true>: the consensus support) alone on hand-built MSAs,
through the test hook rattle_hip_debug_consensus_support (the driver's own stage layout and launch), against oracle.post_msa(mode=2)
on the same rows, which returns per column the winner's count `occ` and the number of rows that voted `total_occ`.

Every comparison is exact.  Level 2 (rows that are reads): support / depth of the consensus' bases are occ / total_occ of the columns
whose winner is a base, in column order.  Level 3 (rows that are pack consensi with a support and a depth per base): a numpy
restatement of the definition in include/rattle_hip.h, fed with the oracle's rows after fix_msa_ends, windows and winners.  Each test
asserts, from the oracle's answer, that the situations it aims at occur."""
import numpy as np
import pytest

from rattle_amd.api import msa_pack

pytestmark = pytest.mark.gpu

GAP = ord("-")
DEFAULT_ORDER = b"U-GTCA"


def to_rows(mat):
    return [m.tobytes() for m in np.asarray(mat, np.uint8)]


def noisy_msa(rng, R, W, gap=0.15, sub=0.1, alphabet=b"ACGT", ends=True):
    """R noisy copies of one random sequence over W columns: a cell is a gap with probability `gap`, another letter with `sub`.
    The first and last 12 columns hold no gap; with `ends`, rows 1 and 2 of every five start / end with a block of 1..8 bases
    and 20 or more gaps (something for fix_msa_ends to cut)."""
    abc = np.frombuffer(alphabet, np.uint8)
    cons = abc[rng.integers(0, len(abc), W)]
    mat = np.tile(cons, (R, 1))
    m = rng.random((R, W)) < sub
    mat[m] = abc[rng.integers(0, len(abc), int(m.sum()))]
    g = rng.random((R, W)) < gap
    g[:, :12] = False
    g[:, max(W - 12, 0):] = False
    mat[g] = GAP
    if ends and W >= 60:
        for i in range(R):
            k = int(rng.integers(1, 9))
            if i % 5 == 1:
                mat[i, :30] = GAP
                mat[i, 2:2 + k] = cons[2:2 + k]
            elif i % 5 == 2:
                mat[i, W - 30:] = GAP
                mat[i, W - 2 - k:W - 2] = cons[W - 2 - k:W - 2]
    return mat


def with_ties(mat):
    """four columns in the middle (inside every row's window) where bases tie for the lead: A, C, G in turn over the rows when there
    are fewer than six of them (1 : 1 : 1 or 2 : 2 : 1 ...), else A and C in turn and a G in the last row of an odd count"""
    R, W = mat.shape
    syms = np.frombuffer(b"ACG", np.uint8)
    for k in range(W // 2 - 2, W // 2 + 2):
        if R < 6:
            mat[:, k] = syms[np.arange(R) % 3]
        else:
            mat[:, k] = syms[np.arange(R) % 2]
            if R % 2:
                mat[R - 1, k] = syms[2]
    return mat


def oracle_post(oracle, rows, order=DEFAULT_ORDER):
    oracle.set_cv_order(order)
    try:
        return oracle.post_msa(rows, None, mode=2)
    finally:
        oracle.set_cv_order(DEFAULT_ORDER)


def evidence(want, order=DEFAULT_ORDER):
    """from the oracle's answer: is there a column whose winner is a base with occ < total_occ; a column whose winner is a base
    and that the window of a trimmed row does not cover; a base winner that leads only by the tie order"""
    mat = np.frombuffer(b"".join(want["rows"]), np.uint8).reshape(len(want["rows"]), -1)
    W = mat.shape[1]
    win = np.frombuffer(want["winner"], np.uint8)
    base = win != GAP
    k = np.arange(W)
    cover = (k[None, :] >= want["rfirst"][:, None]) & (k[None, :] <= want["rlast"][:, None])
    trimmed = want["erased"].sum(1) > 0
    uncovered = base & (~cover[trimmed]).any(0) if trimmed.any() else np.zeros(W, bool)
    counts = np.stack([((mat == s) & cover).sum(0) for s in order])
    assert np.array_equal(counts.max(0)[base], want["occ"][base]) and np.array_equal(counts.sum(0)[base], want["total_occ"][base])
    tie = base & ((counts == counts.max(0)[None, :]).sum(0) > 1)
    for c in np.nonzero(tie)[0]:
        assert win[c] == order[int(np.argmax(counts[:, c] == counts[:, c].max()))]      # the first slot in the order takes it
    return bool((base & (want["occ"] < want["total_occ"])).any()), bool(uncovered.any()), bool(tie.any())


@pytest.fixture(scope="module")
def ctx_on(gpu_ctx):
    gpu_ctx.set_consensus_support(True)
    yield gpu_ctx
    gpu_ctx.set_consensus_support(False)


# ---- level 2 ------------------------------------------------------------------------------------------------------------
SHAPES_A = [(1, 40), (3, 64), (7, 257), (64, 300), (200, 90)]      # 257 and 300 cross the 256-column stride and the 64-lane ballot blocks


@pytest.fixture(scope="module")
def packs_a():
    rng = np.random.default_rng(4100)
    return [to_rows(noisy_msa(rng, R, W) if R == 1 else with_ties(noisy_msa(rng, R, W))) for R, W in SHAPES_A]


def skipped_pack():
    """a pack of width 0 that has bases: what a pack looks like whose POA was skipped"""
    seqs = [b"ACGTACGT", b"TTGA", b"C"]
    return 0, seqs, [np.full(len(s), 12345, np.uint32) for s in seqs], None


def check_level2(got, want, tag):
    base = np.frombuffer(want["winner"], np.uint8) != GAP
    assert got["level"] == 2 and got["consensus"] == want["consensus"], f"{tag}: consensus"
    assert len(want["consensus"]) == int(base.sum())
    assert np.array_equal(got["support"], want["occ"][base]), f"{tag}: support"
    assert np.array_equal(got["depth"], want["total_occ"][base]), f"{tag}: depth"
    assert got["pack_support"] is None and got["pack_depth"] is None
    assert np.all(got["depth"] >= 1) and np.all(got["support"] <= got["depth"])


@pytest.mark.parametrize("order", [DEFAULT_ORDER, b"ACGTU-"])
def test_level_2_is_the_votes_own_count_and_total(ctx_on, oracle, packs_a, order):
    """All five packs and a pack of width 0 between them in one call.  In every pack of three rows or more there is a base column
    with occ < total_occ, one that a trimmed row's window does not cover, and a winner chosen by the tie order; a pack of one row can
    have none of the three (every covered column is 1 of 1), it is the case where support == depth == 1 everywhere."""
    want = [oracle_post(oracle, rows, order) for rows in packs_a]
    inputs = [msa_pack(rows) for rows in packs_a]
    inputs.insert(2, skipped_pack())
    got = ctx_on.debug_consensus_support(inputs, vote_order=order)
    assert got[2]["consensus"] == b"" and len(got[2]["support"]) == 0 and len(got[2]["depth"]) == 0
    del got[2]
    for (R, W), rows, w, g in zip(SHAPES_A, packs_a, want, got):
        check_level2(g, w, f"{R} x {W}")
        if R == 1:
            assert np.all(g["support"] == 1) and np.all(g["depth"] == 1) and len(g["support"]) == W
        else:
            assert evidence(w, order) == (True, True, True), (R, W, evidence(w, order))
    if order != DEFAULT_ORDER:
        # the order matters: some tie goes to another base under the reference's order
        ref = [oracle_post(oracle, rows) for rows in packs_a]
        assert any(a["winner"] != b["winner"] for a, b in zip(want, ref))


# ---- level 3 ------------------------------------------------------------------------------------------------------------
SHAPES_B = [(3, 70), (4, 130), (5, 300)]


def compose(rows, want, sup, dep):
    """include/rattle_hip.h, level 3, per column: of the rows whose window covers K, the support of those that hold the winner
    at K, and the depth of all of them -- a row's base at K or, at a gap, its last base before K.  rows: the input; want: the oracle's
    answer (rows after fix_msa_ends, windows, winners).  A base's index in its row is the number of bases before it in the input row."""
    orig = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
    fixed = np.frombuffer(b"".join(want["rows"]), np.uint8).reshape(orig.shape)
    win = np.frombuffer(want["winner"], np.uint8)
    k = np.arange(orig.shape[1])
    cover = (k[None, :] >= want["rfirst"][:, None]) & (k[None, :] <= want["rlast"][:, None])
    idx = np.maximum(np.cumsum(orig != GAP, 1) - 1, 0)          # the base at the cell, or the last one before it
    sup_c = np.stack([np.asarray(s, np.int64)[i] for s, i in zip(sup, idx)])
    dep_c = np.stack([np.asarray(d, np.int64)[i] for d, i in zip(dep, idx)])
    support = (sup_c * (cover & (fixed == win[None, :]))).sum(0)
    depth = (dep_c * cover).sum(0)
    return support[win != GAP], depth[win != GAP], cover, fixed, win


def test_level_3_composes_the_rows_own_support_and_depth(ctx_on, oracle):
    rng = np.random.default_rng(4200)
    packs, sups, deps = [], [], []
    for R, W in SHAPES_B:
        rows = to_rows(noisy_msa(rng, R, W, gap=0.1, sub=0.08))
        n = [W - r.count(b"-") for r in rows]
        dep = [rng.integers(1, 201, m).astype(np.uint32) for m in n]
        sup = [rng.integers(1, d + 1).astype(np.uint32) for d in dep]      # 1 <= sup <= dep <= 200
        packs.append(rows); sups.append(sup); deps.append(dep)
    got = ctx_on.debug_consensus_support([msa_pack(r) for r in packs], sups, deps)
    seen = {"gap in window": 0, "losing base": 0, "blanked end": 0}
    for (R, W), rows, sup, dep, g in zip(SHAPES_B, packs, sups, deps, got):
        want = oracle_post(oracle, rows)
        support, depth, cover, fixed, win = compose(rows, want, sup, dep)
        base = win != GAP
        assert g["level"] == 3 and g["consensus"] == want["consensus"], (R, W)
        assert np.array_equal(g["support"], support), (R, W)
        assert np.array_equal(g["depth"], depth), (R, W)
        assert np.array_equal(g["pack_support"], want["occ"][base]) and np.array_equal(g["pack_depth"], want["total_occ"][base]), (R, W)
        assert np.all(g["support"] <= g["depth"]) and np.all(g["depth"] >= 1)
        seen["gap in window"] += int((cover & (fixed == GAP) & base[None, :]).sum())          # the carry-forward rule
        seen["losing base"] += int((cover & (fixed != GAP) & (fixed != win[None, :]) & base[None, :]).sum())
        seen["blanked end"] += int((want["erased"].sum(1) > 0).sum())
        assert (want["erased"].sum(1) > 0).any(), (R, W)
    assert all(v > 0 for v in seen.values()), seen


# ---- the switch ---------------------------------------------------------------------------------------------------------
def test_with_the_switch_off_the_hook_returns_no_arrays_and_mode_2_is_unchanged(gpu_ctx, oracle, packs_a):
    inputs = [msa_pack(rows) for rows in packs_a]
    gpu_ctx.set_consensus_support(False)
    off = gpu_ctx.debug_consensus_support(inputs)
    post_off = gpu_ctx.debug_post_msa(inputs, 2)
    gpu_ctx.set_consensus_support(True)
    try:
        on = gpu_ctx.debug_consensus_support(inputs)
        post_on = gpu_ctx.debug_post_msa(inputs, 2)
    finally:
        gpu_ctx.set_consensus_support(False)
    for rows, a, b in zip(packs_a, off, on):
        assert all(a[f] is None for f in ("support", "depth", "pack_support", "pack_depth"))
        assert a["consensus"] == b["consensus"] == oracle_post(oracle, rows)["consensus"] and b["support"] is not None
    for a, b in zip(post_off, post_on):
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key
