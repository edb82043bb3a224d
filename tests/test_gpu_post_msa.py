"""Kernel D (csrc/post_msa.hip: fix_msa_ends, the column vote, the per-read correction, the pack consensus) alone on hand-built
MSAs, through the test hook rattle_hip_debug_post_msa (the driver's own stage layout and launch), against the oracle's restatement
of the same operation on the same rows (oracle.post_msa; tied to the whole-path oracle in tests/test_oracle_correct.py).

Every comparison is exact -- bytes, integers, doubles by their bit pattern -- under these conditions:
  * err and sym only in columns whose winner is not '-' (the reference reads them nowhere else);
  * flag only in columns that some row's window covers; every mode 1 case has a non-gap winner in at least half of its columns;
  * tfront and tback each for a row that keeps a window, their sum for a row that was blanked whole.
Each test also asserts, from the oracle's answer, that the branch it aims at was taken."""
import itertools

import numpy as np
import pytest

from rattle_amd import synth
from rattle_amd.api import msa_pack

pytestmark = pytest.mark.gpu

GAP = ord("-")
DEFAULT_ORDER = b"U-GTCA"


def to_rows(mat):
    return [m.tobytes() for m in np.asarray(mat, np.uint8)]


def quals_for(rows, rng, lo=33, hi=126):
    return [rng.integers(lo, hi + 1, len(r) - r.count(b"-")).astype(np.uint8).tobytes() for r in rows]


def quals_of_matrix(mat, qmat):
    """per row, the quality bytes of its bases out of a cell-by-cell quality matrix"""
    return [q[m != GAP].tobytes() for m, q in zip(mat, qmat)]


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


class Checker:
    """runs packs through the hook and through the oracle and compares them under the module's rules"""

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle = ctx, oracle

    def want(self, rows, quals, mode, min_occ=0.3, gap_occ=0.3, err_ratio=30.0, order=DEFAULT_ORDER):
        self.oracle.set_cv_order(order)
        try:
            return self.oracle.post_msa(rows, quals if mode == 1 else None, min_occ, gap_occ, err_ratio, mode)
        finally:
            self.oracle.set_cv_order(DEFAULT_ORDER)

    def got(self, packs, mode, min_occ=0.3, gap_occ=0.3, err_ratio=30.0, order=DEFAULT_ORDER):
        return self.ctx.debug_post_msa([msa_pack(r, q if mode == 1 else None) for r, q in packs], mode, min_occ, gap_occ, err_ratio, order)

    @staticmethod
    def compare(got, want, rows, mode, min_occ=0.3, gap_occ=0.3, tag=""):
        R, W = len(rows), len(rows[0])
        assert np.array_equal(got["rfirst"], want["rfirst"]) and np.array_equal(got["rlast"], want["rlast"]), f"{tag}: windows"
        assert got["cons"] == want["winner"], f"{tag}: column winners"
        if mode == 2:
            assert got["consensus"] == want["consensus"], f"{tag}: consensus"
            return
        keeps = want["rlast"] >= 0
        er = want["erased"]
        assert np.array_equal(got["tfront"][keeps], er[keeps, 0]) and np.array_equal(got["tback"][keeps], er[keeps, 1]), f"{tag}: trimmed"
        assert np.array_equal((got["tfront"] + got["tback"])[~keeps], er[~keeps].sum(1)), f"{tag}: trimmed (blanked rows)"
        win = np.frombuffer(want["winner"], np.uint8)
        base = win != GAP
        assert 2 * int(base.sum()) >= W, f"{tag}: fewer than half of the columns have a non-gap winner"
        assert np.array_equal(got["err"].view(np.uint64)[base], want["err_bits"][base]), f"{tag}: mean error bits"
        assert np.array_equal(got["sym"][base], want["sym"][base]), f"{tag}: quality symbols"
        k = np.arange(W)
        covered = ((k[None, :] >= want["rfirst"][:, None]) & (k[None, :] <= want["rlast"][:, None])).any(0)
        assert np.all(want["total_occ"][covered] > 0)
        ratio = want["occ"][covered].astype(np.float64) / want["total_occ"][covered].astype(np.float64)
        flag = (ratio >= gap_occ).astype(np.uint8) | ((ratio >= min_occ).astype(np.uint8) << 1)
        assert np.array_equal(got["flag"][covered], flag), f"{tag}: occupancy flags"
        assert got["reads"] == want["reads"], f"{tag}: corrected reads"
        assert np.array_equal(got["olen"], [len(s) for s, _ in want["reads"]]) and np.array_equal(got["olen"] == 0, want["empty"])

    def run(self, rows, quals, mode, **kw):
        """one pack through both; returns the oracle's answer for the branch evidence"""
        want = self.want(rows, quals, mode, **kw)
        got = self.got([(rows, quals)], mode, **kw)[0]
        self.compare(got, want, rows, mode, kw.get("min_occ", 0.3), kw.get("gap_occ", 0.3))
        return want, got


@pytest.fixture(scope="module")
def chk(gpu_ctx, oracle):
    return Checker(gpu_ctx, oracle)


# ---- ends ---------------------------------------------------------------------------------------------------------------
FLANK, CORE = 80, 60


def end_cases():
    """(left flank of 80 columns, bases fix_msa_ends erases from it), worked out by hand from correct.cpp:32-92: a block is ended by 4
    gaps; a block of fewer than 10 bases is cut if, with the gaps behind it, 20 or more gaps follow its last base"""
    g = lambda k: b"-" * k
    b = lambda k: (b"ACGTTGCATG" * 3)[:k]
    cases = [
        (b(9) + g(71), 9),                                            # block of 9 at column 0
        (g(51) + b(9) + g(20), 9),                                    # 9 bases, 20 gaps: cut
        (g(52) + b(9) + g(19), 0),                                    # 9 bases, 19 gaps: stays
        (g(50) + b(10) + g(20), 0),                                   # 10 bases: stays
        (b(5) + g(3) + b(5) + g(67), 0),                              # 5 + 3 gaps + 5 is ONE block of 10
        (b(4) + g(3) + b(5) + g(68), 9),                              # 4 + 3 gaps + 5 is one block of 9
        (b(4) + g(4) + b(5) + g(67), 0),                              # 4 gaps end the block of 4; only 4 gaps follow it
        (b(3) + g(3) + b(3) + g(3) + b(3) + g(65), 9),                # two inner runs of 3
        (b(3) + g(20) + b(4) + g(21) + b(2) + g(30), 9),              # three short blocks, cut one after another
        (g(12) + b(3) + g(20) + b(4) + g(20) + b(2) + g(19), 7),      # ... the third one stays (19 gaps)
        (g(80), 0),
    ]
    assert all(len(f) == FLANK for f, _ in cases)
    return cases


def ends_pack(rng):
    """hand-written rows over a common 60-base core (columns 80..139 of 220) + 30 full-length rows that carry the vote"""
    W = 2 * FLANK + CORE
    abc = np.frombuffer(b"ACGT", np.uint8)
    full = abc[rng.integers(0, 4, W)].tobytes()
    core = full[FLANK:FLANK + CORE]
    g = lambda k: b"-" * k
    rows, expect = [], []
    for flank, t in end_cases():
        rows.append(flank + core + g(FLANK)); expect.append((t, 0, True))
        rows.append(g(FLANK) + core + flank[::-1]); expect.append((0, t, True))          # the mirror image: phase 2
    cases = end_cases()
    for (fa, ta), (fb, tb) in zip(cases[:6], cases[4:10]):                                  # both ends of one row
        rows.append(fa + core + fb[::-1]); expect.append((ta, tb, True))
    # blanked whole in phase 1: a cut that reaches the row end; several cuts, the last one reaching the row end
    rows.append(g(10) + b"ACGTA" + g(W - 15)); expect.append((5, 0, False))
    rows.append(b"ACG" + g(25) + b"TTGACA" + g(W - 34)); expect.append((9, 0, False))
    rows.append(g(W - 9) + b"ACGTTGCAT"); expect.append((0, 9, False))                      # a block that ends at column W-1: phase 1 stops, phase 2 cuts
    # blanked whole in phase 2: phase 1 stops on the short last block, phase 2 blanks it and runs over what phase 1 left
    rows.append(g(W - 28) + b"ACG" + g(20) + b"ACGTA"); expect.append((3, 5, False))
    rows.append(g(W)); expect.append((0, 0, False))
    hand = len(rows)
    for i in range(30):
        a = np.frombuffer(full, np.uint8).copy()
        m = rng.random(W) < 0.03
        a[m] = abc[rng.integers(0, 4, int(m.sum()))]
        rows.append(a.tobytes())
        expect.append((0, 0, True))
    assert all(len(r) == W for r in rows)
    return rows, expect, hand


@pytest.mark.parametrize("mode", [1, 2])
def test_ends(chk, mode):
    """The constants of fix_phase (block size 9 / 10, trailing gap run 19 / 20, inner gap run 3 / 4) at both ends, rows blanked whole
    in phase 1 and in phase 2, an all-gap row; and the reference's own example of a row phase 2 blanks whole, as a pack of its own."""
    rng = np.random.default_rng(101)
    rows, expect, hand = ends_pack(rng)
    quals = quals_for(rows, rng)
    small = [b"ACG" + b"-" * 20 + b"ACGTA", b"ACGTTGCAAGGCTTAACGGATCAGTCAT", b"ACGTTGCAAGGCTTAACGGATCAGTCAT", b"ACGTTGCATGGCTTAACGGATCAGTCAT"]
    squals = quals_for(small, rng)
    want = [chk.want(rows, quals, mode), chk.want(small, squals, mode)]
    got = chk.got([(rows, quals), (small, squals)], mode)
    chk.compare(got[0], want[0], rows, mode, tag="hand rows")
    chk.compare(got[1], want[1], small, mode, tag="ACG + 20 gaps + ACGTA")
    # the cuts really happen, where and as large as worked out by hand
    W = len(rows[0])
    for i, (t1, t2, keeps) in enumerate(expect):
        assert tuple(want[0]["erased"][i]) == (t1, t2), (i, rows[i])
        assert (want[0]["rlast"][i] >= 0) == keeps, (i, rows[i])
        if not keeps:
            assert want[0]["rfirst"][i] == W and want[0]["rows"][i] == b"-" * W
    assert tuple(want[1]["erased"][0]) == (3, 5) and want[1]["rows"][0] == b"-" * 28 and want[1]["rlast"][0] == -1
    if mode == 1:
        assert want[0]["empty"][:hand].sum() == 5 and want[1]["empty"][0] and want[1]["reads"][0] == (b"", b"")
        assert np.array_equal(got[0]["tfront"][:hand], [e[0] for e in expect[:hand]])
        assert np.array_equal(got[0]["tback"][:hand], [e[1] for e in expect[:hand]])


# ---- rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("R", [1, 2, 255, 256, 257, 300])
def test_row_counts(chk, R, mode):
    """Steps b and d walk the rows 256 at a time and step c walks all of them for every column: one row more or fewer than the
    workgroup has threads.  Qualities from the whole range 33..126, so the mean error of a column has the oracle's bits only if
    the rows were summed in row order."""
    rng = np.random.default_rng(200 + R)
    rows = to_rows(noisy_msa(rng, R, 130))
    quals = quals_for(rows, rng)
    want, _ = chk.run(rows, quals, mode)
    if R > 5:
        assert want["erased"][:, 0].sum() > 0 and want["erased"][:, 1].sum() > 0
    if R > 256:
        # the rows behind the 256th are cut, keep windows and change the vote
        assert want["erased"][256:].sum() > 0 and np.all(want["rlast"][256:] > want["rfirst"][256:])
        head = chk.want(rows[:256], quals[:256], mode)
        assert not np.array_equal(head["occ"], want["occ"])
        if mode == 1:
            assert not np.array_equal(head["err_bits"], want["err_bits"])
            assert any(s != r.replace(b"-", b"") for (s, _), r in zip(want["reads"][256:], rows[256:])), "no read behind the 256th was corrected"
    if R >= 255 and mode == 1:
        # the order of the sum shows in the bits: the same rows summed last to first give other means
        back = chk.want(rows[::-1], quals[::-1], mode)
        assert back["winner"] == want["winner"] and not np.array_equal(back["err_bits"], want["err_bits"])


# ---- widths -------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]


def width_pack(rng, W):
    """7 rows; where the width allows it: columns 0..63 without a gap (W >= 127), 64..127 where '-' wins 5 : 2 and 128..191 without a gap
    again (W >= 255), the rest noisy with a gap winner sprinkled in -- the 64-column ballots of the consensus compaction see full,
    empty and partial masks.  No row has anything to cut: the first and last 12 columns hold no gap."""
    R = 7
    if W == 1:
        return [b"A", b"A", b"C", b"A", b"-", b"A", b"A"]
    mat = noisy_msa(rng, R, W, ends=False)
    cons = mat[0].copy()
    cons[cons == GAP] = ord("A")
    sprinkle = rng.random(W) < 0.2
    sprinkle[:12] = False
    sprinkle[max(W - 12, 0):] = False
    for k in np.nonzero(sprinkle)[0]:
        mat[:5, k] = GAP
    if W >= 127:
        mat[:, :64] = np.where(mat[:, :64] == GAP, cons[None, :64], mat[:, :64])
    if W >= 255:
        mat[:5, 64:128] = GAP
        mat[5:, 64:128] = cons[None, 64:128]
        mat[:, 128:192] = np.where(mat[:, 128:192] == GAP, cons[None, 128:192], mat[:, 128:192])
    return to_rows(mat)


def ballot_kinds(winner):
    w = np.frombuffer(winner, np.uint8) != GAP
    kinds = set()
    for a in range(0, len(w), 64):
        n, size = int(w[a:a + 64].sum()), len(w[a:a + 64])
        kinds.add("empty" if n == 0 else "full" if n == 64 else "tail" if size < 64 and n == size else "partial")
    return kinds


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("W", WIDTHS)
def test_widths(chk, W, mode):
    """Widths around the 64 lanes of the compaction ballot and the 256 threads of the column loop, W = 1, and 1000."""
    rng = np.random.default_rng(300 + W)
    rows = width_pack(rng, W)
    quals = quals_for(rows, rng)
    want, got = chk.run(rows, quals, mode)
    kinds = ballot_kinds(want["winner"])
    if W >= 255:
        assert {"empty", "full", "partial"} <= kinds, kinds
    elif W >= 127:
        assert "full" in kinds and len(kinds) > 1, kinds
    elif W > 1:
        assert "partial" in kinds, kinds
    assert want["erased"].sum() == 0
    assert 0 < len(want["consensus"]) < W or W == 1
    if mode == 2:
        assert len(got["consensus"]) == len(want["consensus"])


# ---- ties and thresholds ------------------------------------------------------------------------------------------------
SYMS = b"ACGTU-"


def column_of(rng, counts, R):
    col = np.concatenate([np.full(n, s, np.uint8) for s, n in counts])
    assert len(col) == R
    return rng.permutation(col)


def vote_packs(rng):
    """Three packs of 10, 20 and 100 rows, every row a full window (12 gapless columns at either end), every column between them a
    chosen multiset of symbols: all 2-way ties at 5 : 5 and 3-way ties at 3 : 3 : 3 : 1, winners at exactly 3 of 10, 6 of 20 and
    29 of 100 (a base and '-'), and winners well above and below."""
    packs = []
    for R in (10, 20, 100):
        cols = []
        if R == 10:
            for x, y in itertools.combinations(SYMS, 2):
                cols.append([(x, 5), (y, 5)])
            for x, y, z in itertools.combinations(SYMS, 3):
                w = next(s for s in SYMS if s not in (x, y, z))
                cols.append([(x, 3), (y, 3), (z, 3), (w, 1)])
            for x in SYMS:
                o = [s for s in SYMS if s != x]
                cols.append([(x, 3), (o[0], 2), (o[1], 2), (o[2], 2), (o[3], 1)])          # 3 / 10
                cols.append([(x, 6), (o[4], 2), (o[1], 2)])                                # 0.6
                cols.append([(x, 4), (o[2], 3), (o[3], 3)])                                # 0.4
        elif R == 20:
            for x in SYMS:
                o = [s for s in SYMS if s != x]
                cols.append([(x, 6), (o[0], 5), (o[1], 5), (o[2], 4)])                     # 6 / 20
                cols.append([(x, 5), (o[3], 4), (o[4], 4), (o[0], 4), (o[1], 3)])          # 0.25
                cols.append([(x, 10), (o[2], 10)])                                         # 0.5, a tie
        else:
            for x in SYMS:
                o = [s for s in SYMS if s != x]
                cols.append([(x, 29), (o[0], 28), (o[1], 28), (o[2], 15)])                 # 29 / 100
                cols.append([(x, 25), (o[3], 24), (o[4], 24), (o[0], 24), (o[1], 3)])      # 0.25
                cols.append([(x, 50), (o[2], 49), (o[3], 1)])                              # 0.5
                cols.append([(x, 51), (o[4], 49)])
                cols.append([(x, 23), (o[4], 22), (o[0], 22), (o[1], 22), (o[2], 11)])     # 0.23, below every threshold
        body = np.stack([column_of(rng, c, R) for c in cols], 1)
        # a gapless column between any two chosen ones keeps the non-gap winners above half and the gap runs of a row short
        abc = np.frombuffer(b"ACGU", np.uint8)
        W = 12 + 2 * len(cols) + 12
        mat = np.tile(abc[rng.integers(0, 4, W)], (R, 1))
        mat[:, 12:12 + 2 * len(cols):2] = body
        packs.append((to_rows(mat), cols))
    return packs


def tied(counts):
    top = max(n for _, n in counts)
    return [s for s, n in counts if n == top]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("occ", [(0.3, 0.3), (0.25, 0.5), (0.5, 0.25)])
@pytest.mark.parametrize("order", [b"U-GTCA", b"U-GTAC"])
def test_ties_and_thresholds(chk, order, occ, mode):
    rng = np.random.default_rng(400)
    packs = vote_packs(rng)
    min_occ, gap_occ = occ
    kw = dict(min_occ=min_occ, gap_occ=gap_occ, order=order)
    quals = [quals_for(rows, rng, 40, 90) for rows, _ in packs]
    want = [chk.want(rows, q, mode, **kw) for (rows, _), q in zip(packs, quals)]
    got = chk.got([(rows, q) for (rows, _), q in zip(packs, quals)], mode, **kw)
    flags, ins, dele = set(), {True: 0, False: 0}, {True: 0, False: 0}
    n_ties = 0
    for (rows, cols), q, w, g in zip(packs, quals, want, got):
        chk.compare(g, w, rows, mode, min_occ, gap_occ, tag=f"{len(rows)} rows")
        assert w["erased"].sum() == 0 and np.all(w["rfirst"] == 0)
        mat = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
        for j, counts in enumerate(cols):
            k = 12 + 2 * j
            t = tied(counts)
            first = min(t, key=order.index)                                    # a tie goes to the first slot in the order
            assert w["winner"][k] == first and w["occ"][k] == max(n for _, n in counts) and w["total_occ"][k] == len(rows)
            n_ties += len(t) > 1
            ratio = w["occ"][k] / w["total_occ"][k]
            flags.add(int(ratio >= gap_occ) | int(ratio >= min_occ) << 1)
            if first == GAP:
                dele[ratio >= gap_occ] += int((mat[:, k] != GAP).sum())        # bases under a gap winner: deleted / kept
            else:
                ins[ratio >= gap_occ] += int((mat[:, k] == GAP).sum())         # gaps under a base winner: filled / left
    assert n_ties >= 15 + 20 + 6
    # the A : C tie is what the two orders disagree on
    ac = [(12 + 2 * j) for j, c in enumerate(packs[0][1]) if sorted(tied(c)) == [ord("A"), ord("C")]]
    assert len(ac) == 1 and all(want[0]["winner"][k] == (ord("C") if order == b"U-GTCA" else ord("A")) for k in ac)
    # 3 / 10 and 6 / 20 ARE the literal 0.3 in double, 29 / 100 is below it
    assert 3 / 10 == 0.3 and 6 / 20 == 0.3 and 29 / 100 < 0.3
    assert flags == ({0, 3} if min_occ == gap_occ else {0, 3, 2} if min_occ < gap_occ else {0, 3, 1}), flags
    assert min(ins.values()) > 0 and min(dele.values()) > 0, (ins, dele)       # both sides of gap_occ, under both kinds of winner


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def test_uniform_quality_columns(chk):
    """Every base of column j has the quality 33 + j, in packs of 1, 2, 3, 7 and 10 identical rows: the mean error is the sum of occ
    equal terms over occ, on (or an ulp beside) the Phred threshold of that quality, and the truncation decides the symbol."""
    rng = np.random.default_rng(500)
    abc = np.frombuffer(b"ACGT", np.uint8)
    seq = abc[rng.integers(0, 4, 94)].tobytes()
    q = bytes(range(33, 127))
    packs = [([seq] * occ, [q] * occ) for occ in (1, 2, 3, 7, 10)]
    want = [chk.want(r, qq, 1) for r, qq in packs]
    got = chk.got(packs, 1)
    perr = np.array([10.0 ** (-(c - 33) / 10.0) for c in range(33, 127)])
    moved = 0
    for (rows, _), w, g in zip(packs, want, got):
        chk.compare(g, w, rows, 1, tag=f"occupancy {len(rows)}")
        assert w["winner"] == seq and np.all(w["occ"] == len(rows))
        assert np.all(np.abs(w["err_bits"].view(np.float64) / perr - 1) < 1e-15)
        moved += int((w["err_bits"] != perr.view(np.uint64)).sum())
        assert np.all((w["sym"] == np.arange(33, 127)) | (w["sym"] == np.arange(32, 126))), "the symbol of a quality's own error is that quality or the one below"
        assert g["reads"] == [(seq, q)] * len(rows)
    assert moved > 0, "no mean left the exact power of ten: the division never rounded"


@pytest.mark.parametrize("err_ratio", [30.0, 1.0])
def test_substitution_threshold(chk, err_ratio):
    """One dissenting base per column against eleven agreeing ones; its quality sweeps 33..126 while the consensus' stays fixed per
    column: `err_ratio * perr[q] > cerr` is true for the low qualities and false for the high ones, and with err_ratio 1 it is
    decided at equal qualities by the last bit of the mean."""
    rng = np.random.default_rng(600)
    R, W = 12, 94 * 3
    abc = np.frombuffer(b"ACGT", np.uint8)
    cons = abc[rng.integers(0, 4, W)]
    mat = np.tile(cons, (R, 1))
    qmat = np.tile((45 + 15 * (np.arange(W) // 94)).astype(np.uint8), (R, 1))      # consensus quality 45, 60, 75
    who = rng.integers(0, R, W)
    for k in range(W):
        mat[who[k], k] = abc[(np.searchsorted(abc, cons[k]) + 1 + k % 3) % 4]
        qmat[who[k], k] = 33 + k % 94
    rows, quals = to_rows(mat), quals_of_matrix(mat, qmat)
    want, got = chk.run(rows, quals, 1, err_ratio=err_ratio)
    assert want["winner"] == cons.tobytes() and np.all(want["occ"] == 11)
    out = np.frombuffer(b"".join(s for s, _ in want["reads"]), np.uint8).reshape(R, W)      # no gaps: nothing moves
    made = out[who, np.arange(W)] == cons
    assert np.array_equal(out[who, np.arange(W)][~made], mat[who, np.arange(W)][~made])
    perr = 10.0 ** (-(qmat[who, np.arange(W)].astype(np.float64) - 33) / 10.0)
    assert np.array_equal(made, err_ratio * perr > want["err_bits"].view(np.float64))
    for third in range(3):
        m = made[94 * third:94 * (third + 1)]
        assert m.any() and not m.all(), "the sweep must cross the threshold"
        assert np.array_equal(m, np.sort(m)[::-1]), "made below a quality, refused above it"
    oq = np.frombuffer(b"".join(q for _, q in want["reads"]), np.uint8).reshape(R, W)
    assert np.array_equal(oq[who, np.arange(W)][made], want["sym"][made])                  # a substituted base carries the column's symbol


# ---- several packs in one launch ----------------------------------------------------------------------------------------
SHAPES = [(3, 5), (300, 70), (1, 1), (4, 0), (40, 1000), (2, 17)]


@pytest.fixture(scope="module")
def shape_packs():
    rng = np.random.default_rng(700)
    packs = []
    for R, W in SHAPES:
        if W == 0:
            packs.append(None)
            continue
        rows = to_rows(noisy_msa(rng, R, W, ends=W >= 60)) if W > 1 else [b"G"]
        packs.append((rows, quals_for(rows, rng)))
    return packs


def skipped_pack(mode):
    """a pack of width 0 that has bases: what a pack looks like whose POA was skipped (its columns are whatever was there)"""
    seqs = [b"ACGTACGT", b"TTGA", b"C", b"GATTACA"]
    cols = [np.full(len(s), 12345, np.uint32) for s in seqs]
    return 0, seqs, cols, [b"I" * len(s) for s in seqs] if mode == 1 else None


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("reverse", [False, True])
def test_several_packs_in_one_launch(chk, shape_packs, reverse, mode):
    """Packs of very different sizes, a 1 x 1 pack and a pack of width 0 between two live ones, in one launch: the matrix offsets are
    rounded to 16 bytes and the column offsets are not; every pack's result is that of the same pack launched alone."""
    idx = list(range(len(SHAPES)))[::-1] if reverse else list(range(len(SHAPES)))
    as_input = lambda i: skipped_pack(mode) if shape_packs[i] is None else msa_pack(shape_packs[i][0], shape_packs[i][1] if mode == 1 else None)
    got = chk.ctx.debug_post_msa([as_input(i) for i in idx], mode)
    cells = cols = 0
    for g, i in zip(got, idx):
        R, W = SHAPES[i]
        assert g["moff"] % 16 == 0 and g["moff"] >= cells and g["coff"] == cols
        cells, cols = g["moff"] + R * W, cols + W
    assert any(g["coff"] % 16 for g in got), "no pack starts at an odd column offset"
    for g, i in zip(got, idx):
        alone = chk.ctx.debug_post_msa([as_input(i)], mode)[0]
        for key in g:
            if key in ("moff", "coff"):
                continue
            a, b = g[key], alone[key]
            if key == "err":
                a, b = a.view(np.uint64), b.view(np.uint64)
            same = np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
            assert same, (SHAPES[i], key)
        if shape_packs[i] is None:
            assert np.all(g["rlast"] == -1) and g["cons"] == b""
            if mode == 1:
                assert not g["olen"].any() and not g["tfront"].any() and not g["tback"].any() and g["reads"] == [(b"", b"")] * 4
            else:
                assert g["consensus"] == b""
        else:
            rows, quals = shape_packs[i]
            chk.compare(g, chk.want(rows, quals, mode), rows, mode, tag=str(SHAPES[i]))


# ---- a real MSA and the RNA alphabet ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_a_real_msa(chk, mode):
    """The MSA kernel C makes of 20 synthetic reads of one transcript, as (sequence, column of every base)."""
    seqs, quals, tid, _ = synth.reads(120, 3, 1, False, seed=21)
    ids = [i for i in range(len(seqs)) if tid[i] == tid[0]][:20]
    assert len(ids) == 20
    seqs, quals = [seqs[i] for i in ids], [quals[i] for i in ids]
    rows, width, _ = chk.ctx.poa_msa([seqs])
    rows = rows[0]
    assert [r.replace(b"-", b"") for r in rows] == seqs and len(rows[0]) == width[0] > max(len(s) for s in seqs)
    want, _ = chk.run(rows, quals, mode)
    if mode == 1:
        assert sum(s != r for (s, _), r in zip(want["reads"], seqs)) >= 15, "hardly a read was corrected"
    assert len(want["consensus"]) > 500


@pytest.mark.parametrize("mode", [1, 2])
def test_rna_alphabet(chk, mode):
    rng = np.random.default_rng(800)
    rows = to_rows(noisy_msa(rng, 33, 150, alphabet=b"ACGU"))
    want, _ = chk.run(rows, quals_for(rows, rng), mode)
    assert want["consensus"].count(b"U") > 20 and b"T" not in want["consensus"] and want["erased"].sum() > 0


# ---- T and U in one column ----------------------------------------------------------------------------------------------
T, U = ord("T"), ord("U")


def t_and_u_packs(rng):
    """Two packs of 6 and 10 rows built like vote_packs (every row a full window, a gapless column between any two chosen ones), whose
    chosen columns split between T and U: 3 : 3 (a tie), 4 : 2, 2 : 4 and T : U : '-' at 2 : 2 : 2; and winners whose share lies on both
    sides of the literal 0.3 -- of 6 rows, 2 (0.33) and 1 (0.17: 1.8 falls between the counts), of 10 rows, 3 (exactly 0.3) and 2."""
    A, C, G = b"ACG"
    chosen = {
        6: [[(T, 3), (U, 3)], [(T, 4), (U, 2)], [(T, 2), (U, 4)], [(T, 2), (U, 2), (GAP, 2)],
            [(T, 2), (U, 1), (A, 1), (C, 1), (G, 1)], [(U, 2), (T, 1), (A, 1), (C, 1), (G, 1)], [(T, 2), (U, 2), (A, 1), (C, 1)],
            [(T, 1), (U, 1), (A, 1), (C, 1), (G, 1), (GAP, 1)]],
        10: [[(T, 5), (U, 5)], [(T, 6), (U, 4)], [(T, 4), (U, 6)], [(T, 4), (U, 4), (GAP, 2)],
             [(T, 3), (U, 2), (A, 2), (C, 2), (G, 1)], [(U, 3), (T, 2), (A, 2), (C, 2), (G, 1)], [(T, 3), (U, 3), (A, 2), (C, 2)],
             [(T, 2), (U, 2), (A, 2), (C, 2), (G, 2)], [(T, 2), (U, 2), (GAP, 2), (A, 2), (C, 2)]],
    }
    packs = []
    abc = np.frombuffer(b"ACGTU", np.uint8)
    for R, cols in chosen.items():
        cols = cols * 6                                                # six draws of every column: other rows, other qualities
        body = np.stack([column_of(rng, c, R) for c in cols], 1)
        W = 12 + 2 * len(cols) + 12
        mat = np.tile(abc[rng.integers(0, 5, W)], (R, 1))
        mat[:, 12:12 + 2 * len(cols):2] = body
        qmat = rng.integers(33, 127, mat.shape).astype(np.uint8)
        packs.append((mat, qmat, cols))
    return packs


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("order", [b"U-GTCA", b"U-GTAC"])
def test_t_and_u_in_one_column(chk, order, mode):
    """What POA #1 of reads written with U gives when some members were reverse-complemented (their A became T): T and U vote in slots of
    their own.  A tie goes to the slot that comes first in the order (strict >: U before '-' before T, in both orders); in mode 1 the
    qualities cover 33 .. 126, so that `err_ratio * perr[q] > cerr` holds and fails for T rows under a U winner and for U rows under a T winner."""
    rng = np.random.default_rng(900)
    packs = t_and_u_packs(rng)
    inputs = [(to_rows(mat), quals_of_matrix(mat, qmat)) for mat, qmat, _ in packs]
    want = [chk.want(rows, q, mode, order=order) for rows, q in inputs]
    got = chk.got(inputs, mode, order=order)
    n_ties, flags = 0, set()
    made = {(T, U): set(), (U, T): set()}                              # (row's letter, winner) -> outcomes of the substitution test
    for (mat, qmat, cols), (rows, q), w, g in zip(packs, inputs, want, got):
        R = len(rows)
        chk.compare(g, w, rows, mode, tag=f"{R} rows")
        assert w["erased"].sum() == 0 and np.all(w["rfirst"] == 0)
        for j, counts in enumerate(cols):
            k = 12 + 2 * j
            t = tied(counts)
            first = min(t, key=order.index)
            assert w["winner"][k] == first and w["occ"][k] == max(n for _, n in counts) and w["total_occ"][k] == R
            n_ties += len(t) > 1 and T in t and U in t
            if len(t) > 1 and T in t and U in t:
                assert first == U                                       # U is slot 0
            ratio = w["occ"][k] / w["total_occ"][k]
            flags.add(int(ratio >= 0.3))
            if mode == 1 and first in (T, U) and ratio >= 0.3:
                cerr = float(w["err_bits"][k:k + 1].view(np.float64)[0])
                for i in np.nonzero(mat[:, k] == (T if first == U else U))[0]:
                    made[(int(mat[i, k]), first)].add(bool(30.0 * 10.0 ** (-(int(qmat[i, k]) - 33) / 10.0) > cerr))
    assert n_ties >= 6 * 9 and flags == {0, 1}
    assert 2 / 6 > 0.3 > 1 / 6 and 3 / 10 == 0.3 > 2 / 10
    if mode == 1:
        assert made == {(T, U): {True, False}, (U, T): {True, False}}, made
        # the corrected reads hold both letters, and some T became U and some U became T
        out = b"".join(s for w in want for s, _ in w["reads"])
        assert out.count(b"T") > 20 and out.count(b"U") > 20
        for (mat, _, _), w in zip(packs, want):
            before = (int((mat == T).sum()), int((mat == U).sum()))
            after = (sum(s.count(b"T") for s, _ in w["reads"]), sum(s.count(b"U") for s, _ in w["reads"]))
            assert before != after
    else:
        assert all(b"T" in w["consensus"] and b"U" in w["consensus"] for w in want)
