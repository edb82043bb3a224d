"""Kernel F's read mode (pair_cigar_kernel<*, true>, csrc/pair_cigar.hip) against the contract in plain Python (tests/align_ends_ref.py): the
ops of every pair, exactly -- the reference's walk over the full matrices -- and beside them the records, field for field.  The cases
and scorings of tests/test_gpu_pair_align_ends.py: leading I runs emitted from the left column across block edges, walks that begin
with a switch into U, pairs with t_end == t_start, whose one op the host writes between the device's.  The op sums are the record's
counts and spans; the two device forms against each other at 5,4,8,8; RATTLE_ALIGN_LOCAL through the new call against the old calls;
max_cells, empty input; the pair chunk, the cap on code bytes and the input order change nothing; the stats ids.  No test hands the
reference more than 2e6 cells."""
import os

import numpy as np
import pytest

import align_affine_ref as A
import align_ends_ref as E
import align_ref as R
import cigar_ref as CR

pytestmark = pytest.mark.gpu
ALL = E.all_cases()
FORMS = (None, A.ENGINE, A.MM2, A.LONG, E.CHEAP_GAP)          # None: the linear form, whose scoring is 5,4,8,8
RUNS = [(n, sc) for n in sorted(ALL) for sc in FORMS if sc in (None, A.ENGINE) or n in E.EDGE_CASES]


def ref_scoring(sc):
    return A.LINEAR if sc is None else sc


def run(ctx, case, sc, **kw):
    targets, reads, tor, rev = case
    return ctx.align_cigars(targets, reads, tor, rev, scoring=sc, mode="read", **kw)


def expect(got, case, sc, label, max_cells=0):
    """records == the reference's, every CIGAR == the reference's, the offsets consistent with both, the op sums the record's counts"""
    rec, offsets, ops = got
    want = E.records(*case, ref_scoring(sc), max_cells=max_cells)
    bad = R.same(rec, want)
    assert not bad, (label, bad[:8])
    assert offsets.dtype == np.uint64 and ops.dtype == np.uint32 and len(offsets) == len(case[1]) + 1 and offsets[0] == 0
    assert int(offsets[-1]) == len(ops) and (np.diff(offsets.astype(np.int64)) >= 0).all()
    strings, ref = CR.split(offsets, ops), E.cigars(*case, ref_scoring(sc), max_cells=max_cells)
    wrong = [(r, strings[r][:60], ref[r][:60]) for r in range(len(ref)) if strings[r] != ref[r]]
    assert not wrong, (label, wrong[:4])
    assert all((s == b"") == (st != 0) for s, st in zip(strings, want["status"]))
    for r in range(len(ref)):
        mine = ops[int(offsets[r]):int(offsets[r + 1])]
        sums = [int((mine[(mine & 15) == code] >> 4).sum()) for code in (7, 8, 1, 2)]
        assert sums == [int(rec[f][r]) for f in ("matches", "mismatches", "q_gap", "t_gap")], (label, r)
        if want["status"][r] == 0:
            assert sums[0] + sums[1] + sums[2] == len(case[1][r]) and sums[0] + sums[1] + sums[3] == int(rec["t_end"][r] - rec["t_start"][r])
            assert mine[0] & 15 != 2 and mine[-1] & 15 != 2               # never a D at either end


@pytest.mark.parametrize("name,sc", RUNS, ids=[f"{n}-{'linear' if sc is None else '.'.join(map(str, sc))}" for n, sc in RUNS])
def test_the_ops_of_every_pair(gpu_ctx, name, sc):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    expect(run(gpu_ctx, case, sc), case, sc, name)


def test_the_host_writes_the_op_of_a_pair_without_a_column(gpu_ctx):
    """under 1,64,1,1 four pairs of ends_edges are one I run each, t_end == t_start: they lie between pairs kernel F walked, and a chunk of
    one pair holds nothing else"""
    case = E.ends_edge_case()
    want = E.records(*case, E.CHEAP_GAP)
    none = np.nonzero((want["status"] == 0) & (want["t_end"] == want["t_start"]))[0]
    assert {E.E_UNRELATED, E.E_NO_COLUMN, E.E_NO_COLUMN_LONG, E.E_ONE_ONE_X} <= set(int(r) for r in none)
    for chunk in (0, 1, 3):
        rec, offsets, ops = run(gpu_ctx, case, E.CHEAP_GAP, pair_chunk=chunk)
        expect((rec, offsets, ops), case, E.CHEAP_GAP, f"chunk {chunk}")
        for r in none:
            assert list(ops[int(offsets[r]):int(offsets[r + 1])]) == [len(case[1][r]) << 4 | 1]


def same_bytes(a, b):
    return all(a[0][f].tobytes() == b[0][f].tobytes() for f, _ in R.FIELDS) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("name", sorted({**R.CASES, **CR.CASES, **E.CASES}))
def test_5_4_8_8_is_the_linear_form_byte_for_byte(gpu_ctx, name):
    """two device forms against each other"""
    case = ALL[name]()
    assert same_bytes(run(gpu_ctx, case, A.LINEAR), run(gpu_ctx, case, None))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_local_through_the_new_call_is_the_old_call(gpu_ctx, name):
    """mode=0 is RATTLE_ALIGN_LOCAL handed to rattle_hip_align_cigars_mode; mode="local" goes to the calls without a mode"""
    targets, reads, tor, rev = R.CASES[name]()
    for sc in (None, A.ENGINE):
        assert same_bytes(gpu_ctx.align_cigars(targets, reads, tor, rev, scoring=sc, mode=0), gpu_ctx.align_cigars(targets, reads, tor, rev, scoring=sc)), sc


def test_the_statuses_and_max_cells(gpu_ctx):
    case = R.status_case()
    for sc in (None, A.ENGINE):
        for cap, last in ((0, 0), (24 * 30 - 1, 2), (24 * 30, 0)):        # no cap, one below and on Lq * Lt
            got = run(gpu_ctx, case, sc, max_cells=cap)
            assert list(got[0]["status"]) == [0, 1, 1, 3, last]
            expect(got, case, sc, f"max_cells {cap}", max_cells=cap)
    rec, offsets, ops = gpu_ctx.align_cigars([b"ACGT"], [], [], [], scoring=A.ENGINE, mode="read")
    assert all(len(rec[f]) == 0 for f, _ in R.FIELDS) and list(offsets) == [0] and len(ops) == 0
    rec, offsets, ops = gpu_ctx.align_cigars([], [b"ACGT", b""], [-1, -1], [0, 0], mode="read")
    assert list(rec["status"]) == [3, 3] and list(offsets) == [0, 0, 0] and len(ops) == 0


@pytest.mark.parametrize("sc", (None, A.ENGINE), ids=("linear", "5.4.8.6"))
def test_the_chunks_the_cap_and_the_order_change_nothing(gpu_ctx, sc):
    case = R.random_case()
    base = run(gpu_ctx, case, sc)
    expect(base, case, sc, "random")
    for chunk in (1, 7):
        assert same_bytes(run(gpu_ctx, case, sc, pair_chunk=chunk), base), chunk
    # a cap on the code bytes that splits the case: 60 000 bytes of 32-byte records (30 000 of 16-byte ones) hold a few of its pairs, and
    # the largest need more alone (they run alone)
    rec_bytes, k_align, k_cigar = (16, 6, 7) if sc is None else (32, 8, 9)
    cap = 1875 * rec_bytes
    gpu_ctx.reset_stats()
    os.environ["RATTLE_CIGAR_CODE_BYTES"] = str(cap)
    try:
        capped = run(gpu_ctx, case, sc)
    finally:
        del os.environ["RATTLE_CIGAR_CODE_BYTES"]
    # the sub-chunks as csrc/cigar_plan.h closes them: greedily, when the next pair's record bytes, ceil(R / 64) (C + 63) of them, do not fit
    want = E.records(*case, ref_scoring(sc))
    n_sub, held, alone = 1, 0, 0
    for r in np.nonzero((want["status"] == 0) & (want["t_end"] > want["t_start"]))[0]:
        rows, cols = int(want["q_end"][r] - want["q_start"][r]), int(want["t_end"][r] - want["t_start"][r])
        need = rec_bytes * ((rows + 63) // 64) * (cols + 63)
        alone += need > cap
        if held and held + need > cap:
            n_sub, held = n_sub + 1, 0
        held += need
    assert n_sub > 5 and alone >= 1 and gpu_ctx.kernel_stats(k_cigar)[1] == n_sub and gpu_ctx.kernel_stats(k_align)[1] == 1
    assert all(gpu_ctx.kernel_stats(k)[1] == 0 for k in (6, 7, 8, 9) if k not in (k_align, k_cigar))
    assert same_bytes(capped, base)
    targets, reads, tor, rev = case
    perm = np.random.default_rng(5).permutation(len(reads))
    tperm = np.random.default_rng(6).permutation(len(targets))           # the targets move too: target_of_read follows them
    where = np.argsort(tperm)
    got = gpu_ctx.align_cigars([targets[i] for i in tperm], [reads[i] for i in perm], [int(where[tor[i]]) for i in perm], [rev[i] for i in perm],
                               pair_chunk=13, scoring=sc, mode="read")
    assert all(got[0][f].tobytes() == base[0][f][perm].tobytes() for f, _ in R.FIELDS)
    assert CR.split(got[1], got[2]) == [CR.split(base[1], base[2])[i] for i in perm]


def test_the_launches_count_under_the_ids_of_their_gap_form(gpu_ctx):
    """ids 6 and 7 (linear), 8 and 9 (affine) move and nothing else; alg_bytes by the formulas of include/rattle_hip.h with the read
    mode's rectangles: per pair R + C + rec (ceil(R / 64) (C - 1) + R) + 4 ops + 4, and nothing for a pair without a column"""
    case = R.long_case()
    for sc, rec_bytes, k_align, k_cigar in ((None, 16, 6, 7), (A.ENGINE, 32, 8, 9)):
        want = E.records(*case, ref_scoring(sc))
        nbytes = 0
        for r, (q, x, s) in enumerate(zip(case[1], case[2], case[3])):
            rows, cols = len(q), int(want["t_end"][r] - want["t_start"][r])
            assert cols > 0
            nbytes += rows + cols + rec_bytes * ((rows + 63) // 64 * (cols - 1) + rows) + 4 * len(E.pair(q, case[0][x], s, ref_scoring(sc))[1]) + 4
        gpu_ctx.reset_stats()
        run(gpu_ctx, case, sc)
        assert gpu_ctx.kernel_stats(k_cigar)[1:] == (1, nbytes) and gpu_ctx.kernel_stats(k_align)[1:] == (1, 2 * (200 + 700) + 2 * 40)
        assert all(gpu_ctx.kernel_stats(k)[1:] == (0, 0) for k in range(10) if k not in (k_align, k_cigar))
    # a pair without a column is no launch and no byte of kernel F
    gpu_ctx.reset_stats()
    rec, offsets, ops = gpu_ctx.align_cigars([b"AA"], [b"CC"], [0], [0], scoring=E.CHEAP_GAP, mode="read")
    assert list(ops) == [2 << 4 | 1] and rec["t_end"][0] == rec["t_start"][0] == 1
    assert gpu_ctx.kernel_stats(9)[1:] == (0, 0) and gpu_ctx.kernel_stats(8)[1] == 1
