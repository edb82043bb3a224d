"""The three-state kernel F (pair_cigar_kernel<true>, csrc/pair_cigar.hip) against the contract in plain Python (tests/align_affine_ref.py): the ops of
every pair, exactly -- the reference's walk over the same matrices -- and beside them the records, field for field.  The cases and
scorings of tests/test_gpu_pair_align_affine.py; the four op sums are the record's four counts; 5,4,8,8 against kernels E and F
themselves; max_cells, empty input; the pair chunk, the cap on code bytes (32-byte records) and the input order change nothing; kernel id
9 of the stats beside id 7.  No test hands the reference more than 2e6 cells."""
import os

import numpy as np
import pytest

import align_affine_ref as A
import align_ref as R
import cigar_ref as CR

pytestmark = pytest.mark.gpu
ALL = A.all_cases()
RUNS = [(n, sc) for n in sorted(ALL) for sc in A.SCORINGS if sc in (A.LINEAR, A.ENGINE) or n in A.EDGE_CASES]


def run(ctx, case, sc, **kw):
    targets, reads, tor, rev = case
    return ctx.align_cigars(targets, reads, tor, rev, scoring=sc, **kw)


def expect(got, case, sc, label, max_cells=0):
    """records == the reference's, every CIGAR == the reference's, the offsets consistent with both, the op sums the record's counts"""
    rec, offsets, ops = got
    want = A.records(*case, sc, max_cells=max_cells)
    bad = R.same(rec, want)
    assert not bad, (label, bad[:8])
    assert offsets.dtype == np.uint64 and ops.dtype == np.uint32 and len(offsets) == len(case[1]) + 1 and offsets[0] == 0
    assert int(offsets[-1]) == len(ops) and (np.diff(offsets.astype(np.int64)) >= 0).all()
    strings, ref = CR.split(offsets, ops), A.cigars(*case, sc, max_cells=max_cells)
    wrong = [(r, strings[r][:60], ref[r][:60]) for r in range(len(ref)) if strings[r] != ref[r]]
    assert not wrong, (label, wrong[:4])
    assert all((s == b"") == (st != 0) for s, st in zip(strings, want["status"]))
    for r in range(len(ref)):
        mine = ops[int(offsets[r]):int(offsets[r + 1])]
        sums = [int((mine[(mine & 15) == code] >> 4).sum()) for code in (7, 8, 1, 2)]
        assert sums == [int(rec[f][r]) for f in ("matches", "mismatches", "q_gap", "t_gap")], (label, r)


@pytest.mark.parametrize("name,sc", RUNS, ids=[f"{n}-{'.'.join(map(str, sc))}" for n, sc in RUNS])
def test_the_ops_of_every_pair(gpu_ctx, name, sc):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    expect(run(gpu_ctx, case, sc), case, sc, name)


def same_bytes(a, b):
    return all(a[0][f].tobytes() == b[0][f].tobytes() for f, _ in R.FIELDS) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("name", sorted({**R.CASES, **CR.CASES}))
def test_5_4_8_8_is_kernels_e_and_f(gpu_ctx, name):
    """two device implementations against each other"""
    case = ALL[name]()
    assert same_bytes(run(gpu_ctx, case, A.LINEAR), gpu_ctx.align_cigars(*case))


def test_the_statuses_and_max_cells(gpu_ctx):
    case = R.status_case()
    for cap, last in ((24 * 30 - 1, 2), (24 * 30, 0)):                    # one below and on Lq * Lt
        got = run(gpu_ctx, case, A.ENGINE, max_cells=cap)
        assert got[0]["status"][4] == last
        expect(got, case, A.ENGINE, f"max_cells {cap}", max_cells=cap)
    rec, offsets, ops = gpu_ctx.align_cigars([b"ACGT"], [], [], [], scoring=A.ENGINE)
    assert all(len(rec[f]) == 0 for f, _ in R.FIELDS) and list(offsets) == [0] and len(ops) == 0
    rec, offsets, ops = gpu_ctx.align_cigars([], [b"ACGT", b""], [-1, -1], [0, 0], scoring=A.ENGINE)
    assert list(rec["status"]) == [3, 3] and list(offsets) == [0, 0, 0] and len(ops) == 0


def test_the_chunks_the_cap_and_the_order_change_nothing(gpu_ctx):
    case, sc = R.random_case(), A.ENGINE
    base = run(gpu_ctx, case, sc)
    expect(base, case, sc, "random")
    for chunk in (1, 7):
        assert same_bytes(run(gpu_ctx, case, sc, pair_chunk=chunk), base), chunk
    # a cap on the code bytes that splits the case: 60 000 bytes hold a few of its pairs, and the largest need more alone (they run alone)
    gpu_ctx.reset_stats()
    os.environ["RATTLE_CIGAR_CODE_BYTES"] = "60000"
    try:
        capped = run(gpu_ctx, case, sc)
    finally:
        del os.environ["RATTLE_CIGAR_CODE_BYTES"]
    # the sub-chunks as csrc/cigar_plan.h closes them: greedily, when the next aligned pair's 32 ceil(R / 64) (C + 63) bytes do not fit
    want = A.records(*case, sc)
    n_sub, held, alone = 1, 0, 0
    for r in np.nonzero(want["status"] == 0)[0]:
        rows, cols = int(want["q_end"][r] - want["q_start"][r]), int(want["t_end"][r] - want["t_start"][r])
        need = 32 * ((rows + 63) // 64) * (cols + 63)
        alone += need > 60000
        if held and held + need > 60000:
            n_sub, held = n_sub + 1, 0
        held += need
    assert n_sub > 5 and alone >= 1 and gpu_ctx.kernel_stats(9)[1] == n_sub and gpu_ctx.kernel_stats(8)[1] == 1      # one launch per sub-chunk
    assert gpu_ctx.kernel_stats(7)[1] == 0 and gpu_ctx.kernel_stats(6)[1] == 0
    assert same_bytes(capped, base)
    targets, reads, tor, rev = case
    perm = np.random.default_rng(5).permutation(len(reads))
    tperm = np.random.default_rng(6).permutation(len(targets))           # the targets move too: target_of_read follows them
    where = np.argsort(tperm)
    got = gpu_ctx.align_cigars([targets[i] for i in tperm], [reads[i] for i in perm], [int(where[tor[i]]) for i in perm], [rev[i] for i in perm],
                               pair_chunk=13, scoring=sc)
    assert all(got[0][f].tobytes() == base[0][f][perm].tobytes() for f, _ in R.FIELDS)
    assert CR.split(got[1], got[2]) == [CR.split(base[1], base[2])[i] for i in perm]


def test_the_three_state_kernel_f_is_kernel_9_of_the_stats(gpu_ctx):
    """one launch per sub-chunk (the gather is not counted), the three-state kernel E's launches under id 8, and alg_bytes as
    include/rattle_hip.h defines them: per aligned pair R + C + 32 (ceil(R / 64) (C - 1) + R) + 4 ops + 4 -- id 7's formula with 32 for 16,
    which a run of kernels E and F on the same pairs shows beside it"""
    case = R.long_case()
    want = R.records(*case)
    n_ops = [len(CR.pair(q, case[0][x], s)[1]) for q, x, s in zip(case[1], case[2], case[3])]
    nbytes = {16: 0, 32: 0}
    for r in range(2):
        rows, cols = int(want["q_end"][r] - want["q_start"][r]), int(want["t_end"][r] - want["t_start"][r])
        for rb in nbytes:
            nbytes[rb] += rows + cols + rb * ((rows + 63) // 64 * (cols - 1) + rows) + 4 * n_ops[r] + 4
    gpu_ctx.reset_stats()
    run(gpu_ctx, case, A.LINEAR)                                         # (the linear scoring: the rectangles and ops of kernels E and F)
    ms, launches, got = gpu_ctx.kernel_stats(9)
    assert launches == 1 and got == nbytes[32] and ms >= 0
    assert gpu_ctx.kernel_stats(8)[1:] == (1, 2 * (200 + 700) + 2 * 40)
    assert gpu_ctx.kernel_stats(7)[1:] == (0, 0) and gpu_ctx.kernel_stats(6)[1:] == (0, 0)
    run(gpu_ctx, case, A.LINEAR, pair_chunk=1)
    assert gpu_ctx.kernel_stats(9)[1:] == (3, 2 * nbytes[32]) and gpu_ctx.kernel_stats(8)[1] == 3
    gpu_ctx.align_cigars(*case)                                          # scoring=None is kernels E and F
    assert gpu_ctx.kernel_stats(7)[1:] == (1, nbytes[16]) and gpu_ctx.kernel_stats(6)[1] == 1 and gpu_ctx.kernel_stats(9)[1] == 3
    gpu_ctx.reset_stats()
    gpu_ctx.align_pairs(*case, scoring=A.ENGINE)                         # align_pairs never launches a traceback kernel
    assert gpu_ctx.kernel_stats(9)[1:] == (0, 0) and gpu_ctx.kernel_stats(8)[1] == 1
