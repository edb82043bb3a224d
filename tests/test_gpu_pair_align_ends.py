"""Kernel E's read mode (pair_align_kernel<*, true>, csrc/pair_align.hip) against the contract in plain Python (tests/align_ends_ref.py,
fill + walk): every field of every pair, exactly.  Every case of the three references below and the new ones under 5,4,8,8 -- the linear
form, scoring=None -- and 5,4,8,6; the edge and the new cases -- overhangs whose border run crosses a block edge, a foreign exon,
negative and zero scores, a zero passed through, t_end == t_start -- under 2,4,4,2, 5,4,12,1 and 1,64,1,1 as well; the two device
forms against each other at 5,4,8,8; RATTLE_ALIGN_LOCAL through the new call against the four old calls; statuses and max_cells; the
pair chunk and the input order; the stats ids.  No test hands the reference more than 2e6 cells."""
import numpy as np
import pytest

import align_affine_ref as A
import align_ends_ref as E
import align_ref as R

pytestmark = pytest.mark.gpu
ALL = E.all_cases()
FORMS = (None, A.ENGINE, A.MM2, A.LONG, E.CHEAP_GAP)          # None: the linear form, whose scoring is 5,4,8,8
RUNS = [(n, sc) for n in sorted(ALL) for sc in FORMS if sc in (None, A.ENGINE) or n in E.EDGE_CASES]


def ref_scoring(sc):
    return A.LINEAR if sc is None else sc


def run(ctx, case, sc, **kw):
    targets, reads, tor, rev = case
    return ctx.align_pairs(targets, reads, tor, rev, scoring=sc, mode="read", **kw)


def expect(got, want, label):
    bad = R.same(got, want)
    assert not bad, (label, bad[:8])


def same_bytes(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f, _ in R.FIELDS)


@pytest.mark.parametrize("name,sc", RUNS, ids=[f"{n}-{'linear' if sc is None else '.'.join(map(str, sc))}" for n, sc in RUNS])
def test_every_field_of_every_pair(gpu_ctx, name, sc):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    want = E.records(*case, ref_scoring(sc))
    got = run(gpu_ctx, case, sc)
    expect(got, want, name)
    ok = want["status"] == 0
    assert (got["q_start"][ok] == 0).all() and (got["q_end"][ok] == np.array([len(q) for q in case[1]])[ok]).all()


@pytest.mark.parametrize("name", sorted({**R.CASES, **E.CASES}))
def test_5_4_8_8_is_the_linear_form_byte_for_byte(gpu_ctx, name):
    """two device forms against each other"""
    case = ALL[name]()
    assert same_bytes(run(gpu_ctx, case, A.LINEAR), run(gpu_ctx, case, None))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_local_through_the_new_call_is_the_old_call(gpu_ctx, name):
    """mode=0 is RATTLE_ALIGN_LOCAL handed to rattle_hip_align_pairs_mode; mode="local" goes to the calls without a mode"""
    targets, reads, tor, rev = R.CASES[name]()
    for sc in (None, A.ENGINE):
        assert same_bytes(gpu_ctx.align_pairs(targets, reads, tor, rev, scoring=sc, mode=0), gpu_ctx.align_pairs(targets, reads, tor, rev, scoring=sc)), sc


def test_the_statuses_and_max_cells(gpu_ctx):
    case = R.status_case()
    for sc in FORMS:
        want = E.records(*case, ref_scoring(sc))
        assert list(want["status"]) == [0, 1, 1, 3, 0] and want["score"][0] < 0      # AAAA on CCCC is aligned, at a cost
        expect(run(gpu_ctx, case, sc), want, "status")
    for sc in (None, A.ENGINE):
        for cap, last in ((24 * 30 - 1, 2), (24 * 30, 0)):                # one below and on Lq * Lt
            want = E.records(*case, ref_scoring(sc), max_cells=cap)
            assert want["status"][4] == last
            expect(run(gpu_ctx, case, sc, max_cells=cap), want, f"max_cells {cap}")
    empty = gpu_ctx.align_pairs([b"ACGT"], [], [], [], mode="read")
    assert all(len(empty[f]) == 0 for f, _ in R.FIELDS)
    none = gpu_ctx.align_pairs([], [b"ACGT", b""], [-1, -1], [0, 0], scoring=A.ENGINE, mode="read")
    assert list(none["status"]) == [3, 3]


@pytest.mark.parametrize("sc", (None, A.ENGINE), ids=("linear", "5.4.8.6"))
def test_the_pair_chunk_and_the_order_change_nothing(gpu_ctx, sc):
    case = R.random_case()
    base = run(gpu_ctx, case, sc)
    expect(base, E.records(*case, ref_scoring(sc)), "random")
    for chunk in (1, 7):
        assert same_bytes(run(gpu_ctx, case, sc, pair_chunk=chunk), base), chunk
    targets, reads, tor, rev = case
    perm = np.random.default_rng(5).permutation(len(reads))
    tperm = np.random.default_rng(6).permutation(len(targets))           # the targets move too: target_of_read follows them
    where = np.argsort(tperm)
    got = gpu_ctx.align_pairs([targets[i] for i in tperm], [reads[i] for i in perm], [int(where[tor[i]]) for i in perm], [rev[i] for i in perm],
                              pair_chunk=13, scoring=sc, mode="read")
    assert all(got[f].tobytes() == base[f][perm].tobytes() for f, _ in R.FIELDS)


def test_the_launches_count_under_the_ids_of_their_gap_form(gpu_ctx):
    """ids 6 and 8 move, by id 6's formula (the sequence bytes read + the records written); nothing else does"""
    case = R.long_case()
    nbytes = 2 * (200 + 700) + 2 * 40
    gpu_ctx.reset_stats()
    run(gpu_ctx, case, None)
    assert gpu_ctx.kernel_stats(6)[1:] == (1, nbytes)
    assert all(gpu_ctx.kernel_stats(k)[1:] == (0, 0) for k in range(10) if k != 6)
    run(gpu_ctx, case, A.ENGINE, pair_chunk=1)
    assert gpu_ctx.kernel_stats(8)[1:] == (2, nbytes) and gpu_ctx.kernel_stats(6)[1:] == (1, nbytes)
    assert all(gpu_ctx.kernel_stats(k)[1:] == (0, 0) for k in range(10) if k not in (6, 8))
