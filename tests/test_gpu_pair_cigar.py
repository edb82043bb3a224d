"""Kernel F (csrc/pair_cigar.hip) against the contract in plain Python (tests/cigar_ref.py on tests/align_ref.py): the ops of every pair,
exactly, and beside them the records of kernel E, field for field.  All of align_ref.CASES; rectangles of 1, 63, 64, 65, 127, 128, 129
rows and columns that do not begin at the matrix origin (kernel F's blocks are counted from the rectangle's first row), 1 x 1 and 129 x
129; gap runs of 70 across a window of the walk and a block edge, an up move out of lane 0, a run in almost every column, homopolymer
ties, strand 1 with U; max_cells, empty input, nothing submitted; the pair chunk, the cap on code bytes and the input order change
nothing; kernel id 7 of the stats.  No test hands the reference more than 2e6 cells."""
import os

import numpy as np
import pytest

import align_ref as R
import cigar_ref as CR

pytestmark = pytest.mark.gpu
ALL = {**R.CASES, **CR.CASES}


def run(ctx, case, **kw):
    targets, reads, tor, rev = case
    return ctx.align_cigars(targets, reads, tor, rev, **kw)


def expect(got, case, label, max_cells=0):
    """records == align_ref.records, every CIGAR == cigar_ref's, the offsets consistent with both"""
    rec, offsets, ops = got
    want = R.records(*case, max_cells=max_cells)
    bad = R.same(rec, want)
    assert not bad, (label, bad[:8])
    assert offsets.dtype == np.uint64 and ops.dtype == np.uint32 and len(offsets) == len(case[1]) + 1 and offsets[0] == 0
    assert int(offsets[-1]) == len(ops) and (np.diff(offsets.astype(np.int64)) >= 0).all()
    strings, ref = CR.split(offsets, ops), CR.cigars(*case, max_cells=max_cells)
    wrong = [(r, strings[r][:60], ref[r][:60]) for r in range(len(ref)) if strings[r] != ref[r]]
    assert not wrong, (label, wrong[:4])
    assert all((s == b"") == (st != 0) for s, st in zip(strings, want["status"]))


@pytest.mark.parametrize("name", sorted(ALL))
def test_the_ops_of_every_pair(gpu_ctx, name):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    expect(run(gpu_ctx, case), case, name)


def test_the_statuses_and_max_cells(gpu_ctx):
    case = R.status_case()
    for cap, last in ((24 * 30 - 1, 2), (24 * 30, 0)):                    # one below and on Lq * Lt
        got = run(gpu_ctx, case, max_cells=cap)
        assert got[0]["status"][4] == last
        expect(got, case, f"max_cells {cap}", max_cells=cap)
    rec, offsets, ops = gpu_ctx.align_cigars([b"ACGT"], [], [], [])
    assert all(len(rec[f]) == 0 for f, _ in R.FIELDS) and list(offsets) == [0] and len(ops) == 0
    rec, offsets, ops = gpu_ctx.align_cigars([], [b"ACGT", b""], [-1, -1], [0, 0])
    assert list(rec["status"]) == [3, 3] and list(offsets) == [0, 0, 0] and len(ops) == 0


def same_bytes(a, b):
    return all(a[0][f].tobytes() == b[0][f].tobytes() for f, _ in R.FIELDS) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_the_chunks_the_cap_and_the_order_change_nothing(gpu_ctx):
    case = R.random_case()
    base = run(gpu_ctx, case)
    expect(base, case, "random")
    for chunk in (1, 7):
        assert same_bytes(run(gpu_ctx, case, pair_chunk=chunk), base), chunk
    # a cap on the code bytes that splits the case: 30 000 bytes hold a few of its pairs, and the largest need more alone (they run alone)
    gpu_ctx.reset_stats()
    os.environ["RATTLE_CIGAR_CODE_BYTES"] = "30000"
    try:
        capped = run(gpu_ctx, case)
    finally:
        del os.environ["RATTLE_CIGAR_CODE_BYTES"]
    # the sub-chunks as csrc/cigar_plan.h closes them: greedily, when the next aligned pair's 16 ceil(R / 64) (C + 63) bytes do not fit
    want = R.records(*case)
    n_sub, held, alone = 1, 0, 0
    for r in np.nonzero(want["status"] == 0)[0]:
        rows, cols = int(want["q_end"][r] - want["q_start"][r]), int(want["t_end"][r] - want["t_start"][r])
        need = 16 * ((rows + 63) // 64) * (cols + 63)
        alone += need > 30000
        if held and held + need > 30000:
            n_sub, held = n_sub + 1, 0
        held += need
    assert n_sub > 5 and alone >= 1 and gpu_ctx.kernel_stats(7)[1] == n_sub and gpu_ctx.kernel_stats(6)[1] == 1      # one launch of kernel F per sub-chunk
    assert same_bytes(capped, base)
    targets, reads, tor, rev = case
    perm = np.random.default_rng(5).permutation(len(reads))
    tperm = np.random.default_rng(6).permutation(len(targets))           # the targets move too: target_of_read follows them
    where = np.argsort(tperm)
    got = gpu_ctx.align_cigars([targets[i] for i in tperm], [reads[i] for i in perm], [int(where[tor[i]]) for i in perm], [rev[i] for i in perm],
                               pair_chunk=13)
    assert all(got[0][f].tobytes() == base[0][f][perm].tobytes() for f, _ in R.FIELDS)
    assert CR.split(got[1], got[2]) == [CR.split(base[1], base[2])[i] for i in perm]


def test_kernel_f_is_kernel_7_of_the_stats(gpu_ctx):
    """one launch of kernel F per sub-chunk (the gather is not counted), kernel E's launches under id 6 as before, and alg_bytes as
    include/rattle_hip.h defines them: per aligned pair R + C + 16 (ceil(R / 64) (C - 1) + R) + 4 ops + 4"""
    case = R.long_case()
    want = R.records(*case)
    n_ops = [len(CR.pair(q, case[0][x], s)[1]) for q, x, s in zip(case[1], case[2], case[3])]
    nbytes = 0
    for r in range(2):
        rows, cols = int(want["q_end"][r] - want["q_start"][r]), int(want["t_end"][r] - want["t_start"][r])
        nbytes += rows + cols + 16 * ((rows + 63) // 64 * (cols - 1) + rows) + 4 * n_ops[r] + 4
    gpu_ctx.reset_stats()
    run(gpu_ctx, case)
    ms, launches, got = gpu_ctx.kernel_stats(7)
    assert launches == 1 and got == nbytes and ms >= 0
    e_ms, e_launches, e_bytes = gpu_ctx.kernel_stats(6)
    assert e_launches == 1 and e_bytes == 2 * (200 + 700) + 2 * 40       # what test_gpu_pair_align pins for align_pairs
    run(gpu_ctx, case, pair_chunk=1)
    assert gpu_ctx.kernel_stats(7)[1:] == (3, 2 * nbytes) and gpu_ctx.kernel_stats(6)[1:] == (3, 2 * e_bytes)      # two more launches, the bytes again
    gpu_ctx.reset_stats()
    gpu_ctx.align_pairs(*case)                                           # align_pairs never launches kernel F
    assert gpu_ctx.kernel_stats(7)[1:] == (0, 0) and gpu_ctx.kernel_stats(6)[1] == 1
