"""The per-read correction report (rattle_hip_set_correction_report): the six counters kernel D's report form keeps per row, first
through the test hook on hand-built MSAs and then through `correct_reads`, against a recomputation from the oracle.

The recomputation (recount) re-derives none of kernel D's arithmetic.  It takes, from oracle.post_msa, the rows as fix_msa_ends left
them, every row's window rfirst..rlast, the column winners, occ / total_occ (bit 0 of a column's flag is
float(occ) / float(total) >= gap_occ in IEEE double) and the corrected read, walks the window with a cursor into that read and
classifies each column by the branch of step d that must have handled it; where the row's base and the winner are different bases,
the emitted symbol tells a substitution from a mismatch that was kept.  The cursor must end at the read's length."""
import ctypes as C

import numpy as np
import pytest

from rattle_amd import _lib, synth
from rattle_amd._lib import REPORT_COUNTERS, REPORT_FIELDS
from rattle_amd.api import Clusters, msa_pack
from test_dist_cpu import _plan

pytestmark = pytest.mark.gpu

GAP = ord("-")
ACGT = np.frombuffer(b"ACGT", np.uint8)
MIN_OCC, GAP_OCC, ERR_RATIO = 0.3, 0.5, 30.0          # the hook cases: gap_occ above min_occ, so that a gap winner below gap_occ exists in six rows


def recount(want, gap_occ):
    """{counter: uint32[n_rows]} from the oracle's answer for one pack"""
    rows, win = want["rows"], want["winner"]
    n, W = len(rows), len(rows[0])
    tot, occ = want["total_occ"].astype(np.float64), want["occ"].astype(np.float64)
    bit0 = np.zeros(W, bool)
    voted = tot > 0
    bit0[voted] = occ[voted] / tot[voted] >= gap_occ
    out = {f: np.zeros(n, np.uint32) for f in REPORT_COUNTERS}
    for i in range(n):
        read, cur = want["reads"][i][0], 0
        for k in range(int(want["rfirst"][i]), int(want["rlast"][i]) + 1):
            nt, c = rows[i][k], win[k]
            if nt != GAP and c != GAP:
                emitted = read[cur]
                cur += 1
                if nt == c:
                    assert emitted == nt
                    out["match"][i] += 1
                elif emitted == c:
                    out["substituted"][i] += 1
                else:
                    assert emitted == nt
                    out["mismatch_kept"][i] += 1
            elif nt == GAP and c != GAP:
                if bit0[k]:
                    assert read[cur] == c
                    cur += 1
                    out["inserted"][i] += 1
            elif nt != GAP:
                if bit0[k]:
                    out["deleted"][i] += 1
                else:
                    assert read[cur] == nt
                    cur += 1
                    out["gap_kept"][i] += 1
        assert cur == len(read), f"row {i}: the walk emitted {cur} symbols, the read has {len(read)}"
    return out


def identities(rep, in_len, out_len, tfront, tback, tag):
    s = lambda *names: sum(rep[f].astype(np.int64) for f in names)
    assert np.array_equal(out_len, s("match", "substituted", "mismatch_kept", "inserted", "gap_kept")), f"{tag}: out_len identity"
    assert np.array_equal(in_len, tfront.astype(np.int64) + tback + s("match", "substituted", "mismatch_kept", "deleted", "gap_kept")), f"{tag}: in_len identity"


# ---- the hook cases ---------------------------------------------------------------------------------------------------------
def q_of(rows, q=50, special=()):
    """quality bytes of every row's bases: q everywhere, (row, column, value) where given"""
    qm = np.full((len(rows), len(rows[0])), q, np.uint8)
    for i, k, v in special:
        qm[i, k] = v
    return [qm[i][np.frombuffer(r, np.uint8) != GAP].tobytes() for i, r in enumerate(rows)]


def branches_pack():
    """6 rows x 40 columns: copies of one sequence with one column for every branch of step d (min_occ 0.3, gap_occ 0.5)"""
    cons = np.frombuffer(b"ACGTTGCAGTCATGACCGTAAGCTTGCAATCGGATCCATG", np.uint8)
    mat = np.tile(cons, (6, 1))
    other = lambda k: ACGT[(np.searchsorted(ACGT, cons[k]) + 1) % 4]
    mat[0, 10] = other(10)                      # against 5 of 6 with a bad quality: substituted
    mat[1, 12] = other(12)                      # ... with an excellent one: kept
    mat[2, 15] = GAP                            # a gap under a base winner with 5 of 6: inserted
    mat[:4, 17] = GAP                           # a gap winner with 4 of 6: rows 4 and 5 lose their base
    mat[:2, 20] = GAP                           # a gap winner with 2 of 6 (< gap_occ): the four bases stay, whatever they are
    mat[2:, 20] = np.frombuffer(b"ACGT", np.uint8)
    mat[0, 23] = GAP                            # a base winner with 2 of 6 (< gap_occ): the gap is not filled (counted nowhere)
    mat[1:, 23] = np.frombuffer(b"AACGT", np.uint8)
    rows = [m.tobytes() for m in mat]
    return rows, q_of(rows, 50, [(0, 10, 35), (1, 12, 120)])


def ends_pack():
    """8 rows x 120 columns: six full rows, a row fix_msa_ends blanks whole, a row trimmed by five bases at either end"""
    rng = np.random.default_rng(11)
    cons = ACGT[rng.integers(0, 4, 120)]
    mat = np.tile(cons, (8, 1))
    mat[6, 5:] = GAP
    mat[7, 5:30] = GAP
    mat[7, 90:115] = GAP
    mat[3, 60] = GAP
    rows = [m.tobytes() for m in mat]
    return rows, q_of(rows, 45)


def noisy_pack(seed, R, W):
    """R noisy copies of one sequence over W columns: 12 % gaps, 10 % other letters, qualities over the whole range"""
    rng = np.random.default_rng(seed)
    cons = ACGT[rng.integers(0, 4, W)]
    mat = np.tile(cons, (R, 1))
    m = rng.random((R, W)) < 0.10
    mat[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
    mat[rng.random((R, W)) < 0.12] = GAP
    gapcol = rng.random(W) < 0.08               # columns where the gap wins
    mat[:, gapcol] = np.where(rng.random((R, int(gapcol.sum()))) < 0.7, GAP, mat[:, gapcol])
    split = np.nonzero(rng.random(W) < 0.1)[0]  # columns where the gap wins with about 40 %, the bases sharing the rest: below gap_occ
    mat[:, split] = np.where(rng.random((R, len(split))) < 0.4, GAP, ACGT[rng.integers(0, 4, (R, len(split)))])
    rows = [m.tobytes() for m in mat]
    return rows, [rng.integers(33, 127, W - r.count(b"-")).astype(np.uint8).tobytes() for r in rows]


ZERO_WIDTH = (0, [b"ACGTACGT", b"TTGA", b"C"], [np.full(n, 4321, np.uint32) for n in (8, 4, 1)], [b"I" * 8, b"I" * 4, b"I"])


@pytest.fixture(scope="module")
def hook_cases(oracle):
    """[(name, rows, quals, the oracle's answer, its recount)]; the width-0 pack is (name, None, ...)"""
    cases = []
    for name, (rows, quals) in (("branches 6 x 40", branches_pack()), ("ends 8 x 120", ends_pack()), ("width 0", (None, None)),
                                ("300 x 24", noisy_pack(31, 300, 24)), ("5 x 300", noisy_pack(32, 5, 300))):
        if rows is None:
            cases.append((name, None, None, None, None))
            continue
        want = oracle.post_msa(rows, quals, MIN_OCC, GAP_OCC, ERR_RATIO, 1)
        cases.append((name, rows, quals, want, recount(want, GAP_OCC)))
    return cases


def test_the_cases_reach_what_they_aim_at(hook_cases):
    """on the oracle's side, so that the comparison below cannot pass vacuously"""
    by = {c[0]: c for c in hook_cases}
    _, rows, _, want, cnt = by["branches 6 x 40"]
    assert all(cnt[f].sum() > 0 for f in REPORT_COUNTERS), {f: int(cnt[f].sum()) for f in REPORT_COUNTERS}
    assert cnt["substituted"][0] == 1 and cnt["mismatch_kept"][1] == 1 and cnt["inserted"][2] == 1
    assert list(cnt["deleted"]) == [0, 0, 0, 0, 1, 1] and list(cnt["gap_kept"]) == [0, 0, 1, 1, 1, 1]
    assert want["winner"][23:24] == b"A" and len(want["reads"][0][0]) == 40 - 3          # row 0: columns 17, 20 and 23 emit nothing
    _, rows, _, want, cnt = by["ends 8 x 120"]
    assert want["rlast"][6] == -1 and want["rfirst"][6] == 120 and tuple(want["erased"][6]) == (5, 0)
    assert tuple(want["erased"][7]) == (5, 5) and want["rfirst"][7] == 30 and want["rlast"][7] == 89
    assert all(cnt[f][6] == 0 for f in REPORT_COUNTERS) and cnt["match"][7] == 60
    _, rows, _, want, cnt = by["300 x 24"]
    assert all(cnt[f][256:].sum() > 0 for f in REPORT_COUNTERS), "a counter never moves behind the 256th row"
    _, rows, _, want, cnt = by["5 x 300"]
    assert np.all(want["rlast"] >= 290) and np.all(want["rfirst"] <= 10)
    assert all(cnt[f].sum() > 0 for f in REPORT_COUNTERS)


def as_input(case):
    return ZERO_WIDTH if case[1] is None else msa_pack(case[1], case[2])


def check_pack(got, case, tag):
    name, rows, quals, want, cnt = case
    assert set(REPORT_COUNTERS) <= set(got), f"{tag} {name}: the hook returned no counters"
    if rows is None:
        assert all(not got[f].any() and len(got[f]) == 3 for f in REPORT_COUNTERS), f"{tag} {name}: a pack of width 0 counts nothing"
        assert not got["olen"].any()
        return
    for f in REPORT_COUNTERS:
        assert got[f].dtype == np.uint32 and np.array_equal(got[f], cnt[f]), f"{tag} {name}: {f}\n{got[f]}\n{cnt[f]}"
    assert got["reads"] == want["reads"], f"{tag} {name}: corrected reads"
    in_len = np.array([len(q) for q in quals], np.int64)
    identities(got, in_len, got["olen"].astype(np.int64), got["tfront"], got["tback"], f"{tag} {name}")


def test_hook_counters_equal_the_recount(gpu_ctx, hook_cases):
    """all packs in one launch (the pack of width 0 between two real ones), then every pack in a launch of its own"""
    gpu_ctx.set_correction_report(True)
    try:
        kw = dict(min_occ=MIN_OCC, gap_occ=GAP_OCC, err_ratio=ERR_RATIO)
        together = gpu_ctx.debug_post_msa([as_input(c) for c in hook_cases], 1, **kw)
        alone = [gpu_ctx.debug_post_msa([as_input(c)], 1, **kw)[0] for c in hook_cases]
        in_mode_2 = gpu_ctx.debug_post_msa([msa_pack(hook_cases[0][1])], 2, **kw)[0]
    finally:
        gpu_ctx.set_correction_report(False)
    for g, c in zip(together, hook_cases):
        check_pack(g, c, "one launch")
    for g, c in zip(alone, hook_cases):
        check_pack(g, c, "alone")
    assert not set(REPORT_COUNTERS) & set(in_mode_2), "mode 2 has no report"


def test_switch_off_leaves_every_other_field_as_it_is(gpu_ctx, hook_cases):
    kw = dict(min_occ=MIN_OCC, gap_occ=GAP_OCC, err_ratio=ERR_RATIO)
    packs = [as_input(c) for c in hook_cases]
    off = gpu_ctx.debug_post_msa(packs, 1, **kw)
    gpu_ctx.set_correction_report(True)
    try:
        on = gpu_ctx.debug_post_msa(packs, 1, **kw)
    finally:
        gpu_ctx.set_correction_report(False)
    for a, b, c in zip(off, on, hook_cases):
        assert not set(REPORT_COUNTERS) & set(a), "counters without the switch"
        assert set(b) == set(a) | set(REPORT_COUNTERS)
        for key in a:
            x, y = a[key], b[key]
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (c[0], key)
            else:
                assert x == y, (c[0], key)


# ---- end to end -------------------------------------------------------------------------------------------------------------
SPLIT = 200


@pytest.fixture(scope="module")
def job():
    """three clusters of 12 reads of ~300 nt and one of 220 reads of ~200 nt (two packs at split 200), 10 % error, one strand"""
    s3, q3, t3, _ = synth.reads(150, 3, 1, False, seed=61, tx_seed=62, exon=(30, 45))
    s1, q1, _, _ = synth.reads(220, 1, 1, False, seed=63, tx_seed=64, exon=(20, 30))
    seqs, quals, clusters = [], [], []
    for t in range(3):
        ids = [i for i in range(len(s3)) if t3[i] == t][:12]
        assert len(ids) == 12
        clusters.append(list(range(len(seqs), len(seqs) + 12)))
        seqs += [s3[i] for i in ids]; quals += [q3[i] for i in ids]
    clusters.append(list(range(len(seqs), len(seqs) + 220)))
    seqs += s1; quals += q1
    rng = np.random.default_rng(65)                 # file order is not cluster order
    perm = rng.permutation(len(seqs))
    inv = np.argsort(perm)
    seqs, quals = [seqs[i] for i in perm], [quals[i] for i in perm]
    clusters = [((int(inv[m[0]]), 0, -1), [(int(inv[i]), 0, -1) for i in m]) for m in clusters]
    assert 250 < np.mean([len(seqs[s[0]]) for s in clusters[0][1]]) < 350 and 150 < np.mean([len(seqs[s[0]]) for s in clusters[3][1]]) < 250
    return seqs, quals, clusters


@pytest.fixture(scope="module")
def job_runs(gpu_ctx, job):
    seqs, quals, clusters = job
    off = gpu_ctx.correct_reads(seqs, quals, clusters, split=SPLIT)
    gpu_ctx.set_correction_report(True)
    try:
        on = gpu_ctx.correct_reads(seqs, quals, clusters, split=SPLIT)
    finally:
        gpu_ctx.set_correction_report(False)
    return off, on


def test_correct_reads_outputs_do_not_change_with_the_report(gpu_ctx, job, job_runs):
    off, on = job_runs
    assert "report" not in off and "report" in on
    for key in ("corrected", "uncorrected", "consensi", "skipped"):
        assert off[key] == on[key], key
    assert np.array_equal(off["counters"], on["counters"])
    assert len(on["corrected"]) > 240 and len(on["consensi"]) == 4
    # the same through the handle: the digest over every output array, report() and its refusal
    seqs, quals, clusters = job
    from rattle_amd.api import pack_reads
    cat, o = pack_reads(seqs)
    qcat, _ = pack_reads(quals)
    coff = np.zeros(len(clusters) + 1, np.uint32)
    coff[1:] = np.cumsum([len(m) for _, m in clusters])
    cl = Clusters(np.array([m[0] for m, _ in clusters], np.int32), np.zeros(len(clusters), np.uint8), coff,
                  np.array([s[0] for _, m in clusters for s in m], np.int32), np.zeros(int(coff[-1]), np.uint8), np.zeros(8, np.uint64))
    h0 = gpu_ctx.correct_packed(cat, qcat, o, cl, split=SPLIT, keep=True)
    gpu_ctx.set_correction_report(True)
    try:
        h1 = gpu_ctx.correct_packed(cat, qcat, o, cl, split=SPLIT, keep=True)
    finally:
        gpu_ctx.set_correction_report(False)
    assert h0.digest() == h1.digest() and h0.counts()[:3] == h1.counts()[:3]
    rep = h1.report()
    assert all(np.array_equal(rep[f], on["report"][f]) for f in REPORT_FIELDS)
    with pytest.raises(_lib.RattleError, match="rattle_hip_set_correction_report"):
        h0.report()
    h0.free(); h1.free()


def test_report_lengths_and_identities(job, job_runs):
    seqs, _, _ = job
    _, on = job_runs
    rep, cor = on["report"], on["corrected"]
    assert list(rep) == list(REPORT_FIELDS) and all(v.dtype == np.uint32 and len(v) == len(cor) for v in rep.values())
    assert np.array_equal(rep["out_len"], [len(r[3]) for r in cor])
    assert np.array_equal(rep["in_len"], [len(seqs[r[0]]) for r in cor])
    identities(rep, rep["in_len"].astype(np.int64), rep["out_len"].astype(np.int64), rep["trim_front"], rep["trim_back"], "correct_reads")
    # (these reads carry low qualities: the error test always passes and no gap winner stays below gap_occ -- the hook cases above have those)
    assert all(rep[f].sum() > 0 for f in ("match", "substituted", "inserted", "deleted")), {f: int(rep[f].sum()) for f in REPORT_COUNTERS}


def test_report_equals_the_recount_over_the_oracles_msa(oracle, job, job_runs):
    """the packs as rattle_hip_plan_packs builds them, oracle.poa_msa for their MSA, oracle.post_msa + recount for the counters"""
    seqs, quals, clusters = job
    _, on = job_runs
    cat_off = np.zeros(len(seqs) + 1, np.uint64)
    cat_off[1:] = np.cumsum([len(s) for s in seqs])
    coff = np.zeros(len(clusters) + 1, np.uint32)
    coff[1:] = np.cumsum([len(m) for _, m in clusters])
    mid = np.array([s[0] for _, m in clusters for s in m], np.int32)
    plan = _plan(cat_off, coff, mid, np.zeros(len(mid), np.uint8), 1, split=SPLIT)
    assert len(plan["cluster"]) == 5 and list(plan["cluster"]) == [0, 1, 2, 3, 3]
    want = {f: [] for f in REPORT_FIELDS}
    rids, cids = [], []
    for p in range(5):
        members = [int(x) for x in plan["member"][plan["first"][p]:plan["first"][p + 1]]]
        rows, _ = oracle.poa_msa([seqs[i] for i in members])
        w = oracle.post_msa(rows, [quals[i] for i in members], 0.3, 0.3, 30.0, 1)
        cnt = recount(w, 0.3)
        for j, rid in enumerate(members):
            if not len(w["reads"][j][0]):
                continue
            rids.append(rid); cids.append(int(plan["cluster"][p]))
            want["in_len"].append(len(seqs[rid])); want["out_len"].append(len(w["reads"][j][0]))
            want["trim_front"].append(int(w["erased"][j][0])); want["trim_back"].append(int(w["erased"][j][1]))
            for f in REPORT_COUNTERS:
                want[f].append(int(cnt[f][j]))
    assert [r[0] for r in on["corrected"]] == rids and [r[1] for r in on["corrected"]] == cids
    for f in REPORT_FIELDS:
        assert np.array_equal(on["report"][f], want[f]), f
