"""Kernel D (csrc/post_msa.hip) at the edges of its wide passes: the 16-byte lines of step a, the 64-cell blocks of steps b and d, the
four columns per thread and the 1024-column stride of step c, the four wavefronts that share a pack's rows, the row width up to which
step a builds a row in LDS.  Through ctx.debug_post_msa against oracle.post_msa under the rules of tests/test_gpu_post_msa.py (its
Checker): every comparison is exact -- bytes, integers, doubles by their bit pattern.  The report forms ride along: the six counters
of the correction report against the recount of tests/test_gpu_correction_report.py, the consensus support against the vote's own
counts as in tests/test_gpu_consensus_support.py.  Each test asserts, from the oracle's answer, that the case it aims at occurred."""
import numpy as np
import pytest

from rattle_amd._lib import REPORT_COUNTERS
from rattle_amd.api import msa_pack
from test_gpu_consensus_support import check_level2
from test_gpu_correction_report import recount
from test_gpu_post_msa import Checker, noisy_msa, quals_for, to_rows, width_pack

pytestmark = pytest.mark.gpu

GAP = ord("-")
ACGT = np.frombuffer(b"ACGT", np.uint8)
STAGE_W = 2048          # POST_STAGE_W of post_msa.hip: the widest row step a builds in LDS; a wider pack is filled, then scattered


@pytest.fixture(scope="module")
def chk(gpu_ctx, oracle):
    return Checker(gpu_ctx, oracle)


def run_with_report(chk, packs, want):
    """mode 1 of the packs in one launch, without and with the correction report; both against the oracle's answers, the counters
    against the recount; returns the recounts"""
    off = chk.got(packs, 1)
    chk.ctx.set_correction_report(True)
    try:
        on = chk.got(packs, 1)
    finally:
        chk.ctx.set_correction_report(False)
    counts = []
    for j, ((rows, quals), w, a, b) in enumerate(zip(packs, want, off, on)):
        tag = f"pack {j}: {len(rows)} x {len(rows[0])}"
        chk.compare(a, w, rows, 1, tag=tag)
        chk.compare(b, w, rows, 1, tag=tag + ", report on")
        cnt = recount(w, 0.3)
        for f in REPORT_COUNTERS:
            assert f not in a and b[f].dtype == np.uint32 and np.array_equal(b[f], cnt[f]), f"{tag}: {f}\n{b[f]}\n{cnt[f]}"
        counts.append(cnt)
    return counts


# ---- widths -------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 3, 15, 16, 17, 63, 64, 65, 127, 129, 255, 257, 1025]


@pytest.mark.parametrize("W", WIDTHS)
def test_widths(chk, W):
    """Seven rows of every width around the 4 columns of a thread, the 16 bytes of a line, the 64 cells of a block and the 1024
    columns of one pass of step c, in modes 1 and 2 and with the correction report.  With seven rows of a width that is no multiple
    of 16 every row starts at another offset in its line.  Every width keeps a non-gap winner in at least half of its columns
    (Checker.compare asserts it), so the whole rule set applies to all of them."""
    rng = np.random.default_rng(1300 + W)
    rows = width_pack(rng, W)
    quals = quals_for(rows, rng)
    assert len(rows) == 7 and len(rows[0]) == W
    want = chk.want(rows, quals, 1)
    cnt = run_with_report(chk, [(rows, quals)], [want])[0]
    want2, got2 = chk.run(rows, quals, 2)
    assert want2["winner"] == want["winner"] and len(got2["consensus"]) == len(want["consensus"]) > 0
    whole = np.ones(7, bool) if W > 1 else np.frombuffer(b"".join(rows), np.uint8) != GAP          # (the 7 x 1 pack has a row that is a gap)
    assert want["erased"].sum() == 0 and np.all(want["rfirst"][whole] == 0) and np.all(want["rlast"][whole] == W - 1)
    assert np.all(want["rlast"][~whole] == -1) and np.array_equal(want["empty"], ~whole)
    assert int(cnt["match"].sum()) > 0
    if W >= 63:
        assert all(int(cnt[f].sum()) > 0 for f in ("match", "inserted", "deleted")), {f: int(cnt[f].sum()) for f in REPORT_COUNTERS}
        assert any(len(s) != W for s, _ in want["reads"]), "no row was compacted"


# ---- rows ---------------------------------------------------------------------------------------------------------------
ROWS = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 300]


@pytest.mark.parametrize("R", ROWS)
def test_row_counts(chk, R):
    """Row counts around the four wavefronts of steps a, b and d and around 64 and 256, at a width (131) that is no multiple of 4:
    mode 2 for all of them, mode 1 up to 257 rows."""
    rng = np.random.default_rng(1400 + R)
    rows = to_rows(noisy_msa(rng, R, 131))
    quals = quals_for(rows, rng)
    want, _ = chk.run(rows, quals, 2)
    if R > 5:
        assert want["erased"][:, 0].sum() > 0 and want["erased"][:, 1].sum() > 0
        assert want["erased"][R - R % 4 - 4:].sum() > 0 or R % 5 == 0, "no row of the last round of wavefronts was cut"
    if R <= 257:
        want1, _ = chk.run(rows, quals, 1)
        assert np.array_equal(want1["rfirst"], want["rfirst"])
        if R > 5:
            last = want1["reads"][R - 1][0]
            assert 0 < len(last) and last != rows[R - 1].replace(b"-", b""), "the last row was not corrected"


# ---- several packs in one launch ----------------------------------------------------------------------------------------
MIXED = [(3, 17), (64, 64), (5, 1), (200, 333), (1, 129), (257, 65)]


@pytest.fixture(scope="module")
def mixed_packs():
    rng = np.random.default_rng(1500)
    packs = []
    for R, W in MIXED:
        rows = [b"A", b"A", b"C", b"-", b"A"] if W == 1 else to_rows(noisy_msa(rng, R, W))
        assert len(rows) == R
        packs.append((rows, quals_for(rows, rng)))
    return packs


def test_mixed_launch(chk, mixed_packs):
    """Six packs of mixed rows x width in one launch, modes 1 (with the correction report) and 2: matrices that start on a 16-byte
    line but on no 64-byte one, and rows that start at odd addresses in four of the packs."""
    want1 = [chk.want(r, q, 1) for r, q in mixed_packs]
    run_with_report(chk, mixed_packs, want1)
    got2 = chk.got(mixed_packs, 2)
    for (rows, quals), g, (R, W) in zip(mixed_packs, got2, MIXED):
        chk.compare(g, chk.want(rows, quals, 2), rows, 2, tag=f"{R} x {W}")
    moff = [g["moff"] for g in got2]
    assert all(m % 16 == 0 for m in moff) and sum(m % 64 != 0 for m in moff) >= 2, moff
    assert sum(any((m + i * W) % 2 for i in range(R)) for m, (R, W) in zip(moff, MIXED)) == 4
    assert sum(int(w["erased"].sum() > 0) for w in want1) >= 3
    assert want1[2]["reads"][3] == (b"", b"") and want1[2]["winner"] == b"A"


# ---- long rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [STAGE_W, STAGE_W + 1, 5000])
def test_long_rows(chk, W):
    """Three rows of the last width step a builds in LDS, of the first it does not, and of 5000 columns."""
    rng = np.random.default_rng(1600 + W)
    rows = to_rows(noisy_msa(rng, 3, W))
    quals = quals_for(rows, rng)
    want, _ = chk.run(rows, quals, 1)
    want2, _ = chk.run(rows, quals, 2)
    assert tuple(want["erased"][1]) != (0, 0) and tuple(want["erased"][2]) != (0, 0) and np.all(want["rlast"] > W - 40)
    assert W // 2 < len(want2["consensus"]) < W and all(len(s) > W // 2 for s, _ in want["reads"])


# ---- ends ---------------------------------------------------------------------------------------------------------------
def end_rows(W):
    """[(row, bases erased in front, at the back, keeps a window)]: the left-hand cases and their mirror images.  With 257 columns
    each case stands behind 58 or 40 gaps, so that its blocks and gap runs lie across column 64 (and, mirrored, across column 192,
    the 64th cell from the right); with 65 columns the runs of the whole-row cases end in column 64 / 0."""
    g = lambda k: b"-" * k
    b = lambda k: (b"ACGTTGCATGCA" * 25)[:k]
    lead = 58 if W == 257 else 0
    left = []
    for sz, run in ((9, 19), (9, 20), (10, 19), (10, 20)):
        flank = g(lead) + b(sz) + g(run)
        left.append((flank + b(W - len(flank)), sz if (sz, run) == (9, 20) else 0))
    lead = 40 if W == 257 else 0
    flank = g(lead) + b(3) + g(20) + b(4) + g(21)                      # two cuts on one side, the second block across column 64
    left.append((flank + b(W - len(flank)), 7))
    flank = g(lead) + b(2) + g(20) + b(9) + g(20) + b(5) + g(19)        # two cuts, then a short block that stays
    if W == 257:
        left.append((flank + b(W - len(flank)), 11))
    cases = []
    for row, t in left:
        assert len(row) == W
        cases.append((row, t, 0, True))
        cases.append((row[::-1], 0, t, True))
    cases.append((g(40) + b(4) + g(W - 44), 4, 0, False))               # blanked whole from the left: the run ends with the row
    cases.append((g(W - 44) + b(4) + g(40), 4, 0, False))
    cases.append((b(3) + g(25) + b(6) + g(W - 34), 9, 0, False))        # ... by two cuts
    cases.append((g(W - 28) + b(3) + g(20) + b(5), 3, 5, False))        # phase 1 stops on the last block, phase 2 blanks it and the rest
    cases.append((g(W - 9) + b(9), 0, 9, False))                        # phase 1 stops at once, phase 2 cuts the only block
    cases.append((b(10) + g(W - 35) + b(4) + g(21), 0, 4, True))        # phase 2 cuts, then runs over the whole row to a block at column 0
    assert all(len(c[0]) == W for c in cases)
    return cases


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("W", [65, 257])
def test_ends(chk, W, mode):
    """fix_msa_ends where a cut, or the gap run that decides it, crosses a 64-cell block: 9 / 10 bases before 19 / 20 gaps, two cuts
    on one side, rows blanked whole in phase 1 and in phase 2 -- with 30 full rows that carry the vote."""
    rng = np.random.default_rng(1700 + W)
    cases = end_rows(W)
    rows = [c[0] for c in cases]
    full = ACGT[rng.integers(0, 4, W)]
    for _ in range(30):
        a = full.copy()
        m = rng.random(W) < 0.03
        a[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        rows.append(a.tobytes())
    quals = quals_for(rows, rng)
    want, got = chk.run(rows, quals, mode)
    for i, (row, t1, t2, keeps) in enumerate(cases):
        assert tuple(want["erased"][i]) == (t1, t2), (i, row)
        assert (want["rlast"][i] >= 0) == keeps, (i, row)
        if not keeps:
            assert want["rfirst"][i] == W and want["rows"][i] == b"-" * W
        elif t1 or t2:
            assert want["rows"][i] != row and want["rows"][i].replace(b"-", b"") in row.replace(b"-", b"")
    if W == 257:
        # the cuts lie across the block edges
        cut = [np.nonzero(np.frombuffer(c[0], np.uint8) != np.frombuffer(w, np.uint8))[0] for c, w in zip(cases, want["rows"])]
        assert any(len(c) and c.min() < 64 <= c.max() for c in cut) and any(len(c) and c.min() < 192 <= c.max() for c in cut)
    assert want["rfirst"][len(cases) - 1] == 0 and want["rlast"][len(cases) - 1] == 9
    if mode == 1:
        assert np.array_equal(got["tfront"][:len(cases)], [c[1] for c in cases]) and np.array_equal(got["tback"][:len(cases)], [c[2] for c in cases])


# ---- in-place compaction ------------------------------------------------------------------------------------------------
def test_in_place_compaction(chk):
    """Step d writes a row's output over the row, 64 columns a block, 257 columns a row.  Pack 0: five gapless rows of one sequence,
    every column emits and nothing moves.  Pack 1: eight rows with two runs of 12 gap columns; row 8 holds bases only in the first run
    (its window is that run, every column of it is deleted: a window that emits nothing); row 9 holds bases only in the two runs, so
    its window spans both, its own bases are deleted and all it emits are the consensus' bases put into its gaps."""
    rng = np.random.default_rng(1800)
    W = 257
    seq = ACGT[rng.integers(0, 4, W)]
    full = [seq.tobytes()] * 5
    mat = np.tile(seq, (10, 1))
    mat[:8, 100:112] = GAP
    mat[:8, 150:162] = GAP
    mat[8] = GAP; mat[8, 100:112] = seq[100:112]
    mat[9] = GAP; mat[9, 100:112] = seq[100:112]; mat[9, 150:162] = seq[150:162]
    holes = to_rows(mat)
    packs = [(full, quals_for(full, rng)), (holes, quals_for(holes, rng))]
    want = [chk.want(r, q, 1) for r, q in packs]
    cnt = run_with_report(chk, packs, want)
    assert all(s == seq.tobytes() for s, _ in want[0]["reads"]) and np.all(cnt[0]["match"] == W)
    w, c = want[1], cnt[1]
    assert w["erased"].sum() == 0 and (w["rfirst"][8], w["rlast"][8]) == (100, 111) and (w["rfirst"][9], w["rlast"][9]) == (100, 161)
    assert w["reads"][8] == (b"", b"") and c["deleted"][8] == 12 and sum(int(c[f][8]) for f in REPORT_COUNTERS) == 12
    assert w["reads"][9][0] == seq[112:150].tobytes() and c["inserted"][9] == 38 and c["deleted"][9] == 24
    assert sum(int(c[f][9]) for f in ("match", "substituted", "mismatch_kept", "gap_kept")) == 0
    assert all(len(s) == W - 24 for s, _ in w["reads"][:8])


# ---- the consensus support ----------------------------------------------------------------------------------------------
def test_consensus_support_on_two_of_the_shapes(chk, mixed_packs):
    """post_msa_kernel<2, true> on the seven rows of 257 columns and on the mixed launch's 200 x 333."""
    rng = np.random.default_rng(1300 + 257)
    packs = [width_pack(rng, 257), mixed_packs[3][0]]
    chk.ctx.set_consensus_support(True)
    try:
        got = chk.ctx.debug_consensus_support([msa_pack(r) for r in packs])
    finally:
        chk.ctx.set_consensus_support(False)
    for rows, g in zip(packs, got):
        want = chk.want(rows, None, 2)
        check_level2(g, want, f"{len(rows)} x {len(rows[0])}")
        base = np.frombuffer(want["winner"], np.uint8) != GAP
        assert np.any(want["occ"][base] < want["total_occ"][base])
