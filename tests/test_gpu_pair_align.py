"""Kernel E (csrc/pair_align.hip) against the contract in plain Python (tests/align_ref.py, the classic fill + traceback): every field
of every pair, exactly.  Lengths 1 and one below, on and one above the kernel's block of 64 rows (the hand-over strip is written from
65 rows on, read and written from 129) and its refill of 64 columns, crossed; a 200 x 700 pair over several blocks and refills and its
transpose; ties between predecessors and between end cells; the zero rule; strand 1 with U against T and a read whose aligned part is
not centred; every status; 60 random pairs; the pair chunk and the input order.  No test hands the reference more than 2e6 cells."""
import numpy as np
import pytest

import align_ref as R

pytestmark = pytest.mark.gpu


def run(ctx, case, **kw):
    targets, reads, tor, rev = case
    return ctx.align_pairs(targets, reads, tor, rev, **kw)


def expect(got, want, label):
    bad = R.same(got, want)
    assert not bad, (label, bad[:8])


@pytest.mark.parametrize("name", ["edges", "long", "ties", "two_ends", "zero_crossing", "strand", "random"])
def test_every_field_of_every_pair(gpu_ctx, name):
    case = R.CASES[name]()
    assert R.cells(case) <= 2_000_000
    want = R.records(*case)
    assert (want["status"] == 0).sum() >= len(want["status"]) - 6         # (a few wrong-strand / unrelated pairs may align nothing)
    expect(run(gpu_ctx, case), want, name)


def test_the_statuses_and_max_cells(gpu_ctx):
    case = R.status_case()
    want = R.records(*case)
    assert list(want["status"]) == [1, 1, 1, 3, 0]
    expect(run(gpu_ctx, case), want, "status")
    for cap, last in ((24 * 30 - 1, 2), (24 * 30, 0)):                    # one below and on Lq * Lt
        want = R.records(*case, max_cells=cap)
        assert want["status"][4] == last
        expect(run(gpu_ctx, case, max_cells=cap), want, f"max_cells {cap}")
    empty = gpu_ctx.align_pairs([b"ACGT"], [], [], [])
    assert all(len(empty[f]) == 0 for f, _ in R.FIELDS)
    none = gpu_ctx.align_pairs([], [b"ACGT", b""], [-1, -1], [0, 0])
    assert list(none["status"]) == [3, 3]


def test_the_pair_chunk_and_the_order_change_nothing(gpu_ctx):
    case = R.random_case()
    want = R.records(*case)
    base = run(gpu_ctx, case)
    expect(base, want, "random")
    for chunk in (1, 7):
        got = run(gpu_ctx, case, pair_chunk=chunk)
        assert all(got[f].tobytes() == base[f].tobytes() for f, _ in R.FIELDS), chunk
    targets, reads, tor, rev = case
    perm = np.random.default_rng(5).permutation(len(reads))
    tperm = np.random.default_rng(6).permutation(len(targets))           # the targets move too: target_of_read follows them
    where = np.argsort(tperm)
    got = gpu_ctx.align_pairs([targets[i] for i in tperm], [reads[i] for i in perm], [int(where[tor[i]]) for i in perm], [rev[i] for i in perm],
                              pair_chunk=13)
    assert all(got[f].tobytes() == base[f][perm].tobytes() for f, _ in R.FIELDS)


def test_kernel_e_is_kernel_6_of_the_stats(gpu_ctx):
    case = R.long_case()
    gpu_ctx.reset_stats()
    run(gpu_ctx, case)
    ms, launches, nbytes = gpu_ctx.kernel_stats(6)
    assert launches == 1 and nbytes == 2 * (200 + 700) + 2 * 40 and ms >= 0      # the sequence bytes read + the records written
    run(gpu_ctx, case, pair_chunk=1)
    assert gpu_ctx.kernel_stats(6)[1:] == (3, 2 * nbytes)
