"""The three-state kernel E (pair_align_kernel<true>, csrc/pair_align.hip) against the contract in plain Python (tests/align_affine_ref.py, fill + walk):
every field of every pair, exactly.  Every case of align_ref, cigar_ref and align_affine_ref under 5,4,8,8 and 5,4,8,6, the edge and the
new cases -- long gaps whose U state crosses block edges through the strip, gaps that end and begin on row 64, a D run across two
refills, open / extend ties -- under 2,4,4,2 and 5,4,12,1 as well; 5,4,8,8 against kernel E itself, field for field; statuses and
max_cells; the pair chunk and the input order; kernel id 8 of the stats.  No test hands the reference more than 2e6 cells."""
import numpy as np
import pytest

import align_affine_ref as A
import align_ref as R

pytestmark = pytest.mark.gpu
ALL = A.all_cases()
RUNS = [(n, sc) for n in sorted(ALL) if n != "status" for sc in A.SCORINGS if sc in (A.LINEAR, A.ENGINE) or n in A.EDGE_CASES]


def run(ctx, case, sc, **kw):
    targets, reads, tor, rev = case
    return ctx.align_pairs(targets, reads, tor, rev, scoring=sc, **kw)


def expect(got, want, label):
    bad = R.same(got, want)
    assert not bad, (label, bad[:8])


@pytest.mark.parametrize("name,sc", RUNS, ids=[f"{n}-{'.'.join(map(str, sc))}" for n, sc in RUNS])
def test_every_field_of_every_pair(gpu_ctx, name, sc):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    want = A.records(*case, sc)
    assert (want["status"] == 0).sum() >= len(want["status"]) - 6         # (a few wrong-strand / unrelated pairs may align nothing)
    expect(run(gpu_ctx, case, sc), want, name)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_5_4_8_8_is_kernel_e_field_for_field(gpu_ctx, name):
    """two device implementations against each other"""
    case = R.CASES[name]()
    expect(run(gpu_ctx, case, A.LINEAR), gpu_ctx.align_pairs(*case), name)


def test_the_statuses_and_max_cells(gpu_ctx):
    case = R.status_case()
    for sc in A.SCORINGS:
        want = A.records(*case, sc)
        assert list(want["status"]) == [1, 1, 1, 3, 0]
        expect(run(gpu_ctx, case, sc), want, "status")
    for cap, last in ((24 * 30 - 1, 2), (24 * 30, 0)):                    # one below and on Lq * Lt
        want = A.records(*case, A.ENGINE, max_cells=cap)
        assert want["status"][4] == last
        expect(run(gpu_ctx, case, A.ENGINE, max_cells=cap), want, f"max_cells {cap}")
    empty = gpu_ctx.align_pairs([b"ACGT"], [], [], [], scoring=A.ENGINE)
    assert all(len(empty[f]) == 0 for f, _ in R.FIELDS)
    none = gpu_ctx.align_pairs([], [b"ACGT", b""], [-1, -1], [0, 0], scoring=A.ENGINE)
    assert list(none["status"]) == [3, 3]
    with pytest.raises(Exception):
        gpu_ctx.align_pairs([b"ACGT"], [b"ACGT"], [0], [0], scoring=(5, 4, 6, 8))


def test_the_pair_chunk_and_the_order_change_nothing(gpu_ctx):
    case = R.random_case()
    base = run(gpu_ctx, case, A.ENGINE)
    expect(base, A.records(*case, A.ENGINE), "random")
    for chunk in (1, 7):
        got = run(gpu_ctx, case, A.ENGINE, pair_chunk=chunk)
        assert all(got[f].tobytes() == base[f].tobytes() for f, _ in R.FIELDS), chunk
    targets, reads, tor, rev = case
    perm = np.random.default_rng(5).permutation(len(reads))
    tperm = np.random.default_rng(6).permutation(len(targets))           # the targets move too: target_of_read follows them
    where = np.argsort(tperm)
    got = gpu_ctx.align_pairs([targets[i] for i in tperm], [reads[i] for i in perm], [int(where[tor[i]]) for i in perm], [rev[i] for i in perm],
                              pair_chunk=13, scoring=A.ENGINE)
    assert all(got[f].tobytes() == base[f][perm].tobytes() for f, _ in R.FIELDS)


def test_the_three_state_kernel_e_is_kernel_8_of_the_stats(gpu_ctx):
    case = R.long_case()
    gpu_ctx.reset_stats()
    run(gpu_ctx, case, A.LINEAR)
    ms, launches, nbytes = gpu_ctx.kernel_stats(8)
    assert launches == 1 and nbytes == 2 * (200 + 700) + 2 * 40 and ms >= 0      # id 6's formula: the sequence bytes read + the records written
    assert gpu_ctx.kernel_stats(6)[1:] == (0, 0) and gpu_ctx.kernel_stats(7)[1:] == (0, 0) and gpu_ctx.kernel_stats(9)[1:] == (0, 0)
    run(gpu_ctx, case, A.ENGINE, pair_chunk=1)
    assert gpu_ctx.kernel_stats(8)[1:] == (3, 2 * nbytes) and gpu_ctx.kernel_stats(6)[1] == 0
    gpu_ctx.align_pairs(*case)                                           # scoring=None is kernel E
    assert gpu_ctx.kernel_stats(8)[1] == 3 and gpu_ctx.kernel_stats(6)[1] == 1
