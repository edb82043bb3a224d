"""Kernels E and F (csrc/pair_align.hip, csrc/pair_cigar.hip), all eight instantiations -- linear and affine gaps, local and read mode, the
records alone and with the traceback -- against the contracts in plain Python (tests/align_affine_ref.py, tests/align_ends_ref.py) on
the cases of tests/align_sweep.py, which tests/test_align_sweep.py shows to sit where a wrong rule or index changes the answer:

  end_order       the end cell's order (i before j) across lanes, blocks and refills; last-row ties across three refills
  shifted_*       diagonal before up before left, open before extend, on and around rows and columns 64 and 128
  strand_edges    strand 1 with the span on 1, 63 - 65, 127 - 129 rows and q_start 0, 3 and 64; overhangs on the reverse strand
  many_blocks*    18 row blocks and 17 refills, an alignment of more than 1024 rows
  SWEEP_SCORINGS  both ends of every magnitude on a device; x > 2 o in local mode ("up before left" decides 84 pairs of edges +
                  random); o == e other than 8,8, where the contract is the linear path

Every field with align_ref.same, every CIGAR string, the offsets and the op sums, through Context.align_pairs and Context.align_cigars
in both modes.  scoring=None is the linear form, whose contract is 5,4,8,8.  No test hands the reference more than 2e6 cells; a pair's
reference is computed once and shared (the references remember pairs)."""
import os

import numpy as np
import pytest

import align_affine_ref as A
import align_ref as R
import align_sweep as S
import cigar_ref as CR

pytestmark = pytest.mark.gpu
ALL = S.all_cases()
STANDARD = (None, A.ENGINE, A.MM2)
RUNS = [(n, sc, mode) for n in sorted(S.CASES) for sc in STANDARD for mode in S.MODES]
RUNS += [(n, sc, mode) for n in S.SWEPT for sc in S.SWEEP_SCORINGS for mode in S.MODES]


def ref_scoring(sc):
    return A.LINEAR if sc is None else sc


def run_id(run):
    return f"{run[0]}-{S.scoring_id(run[1])}-{run[2]}"


def expect(pairs_rec, got, case, sc, mode, label):
    """align_pairs' records and align_cigars' == the reference's; every CIGAR == the reference's; the offsets consistent with both; the
    op sums the record's counts and spans"""
    rec, offsets, ops = got
    want = S.records(case, ref_scoring(sc), mode)
    for mine in (pairs_rec, rec):
        bad = R.same(mine, want)
        assert not bad, (label, bad[:8])
    assert offsets.dtype == np.uint64 and ops.dtype == np.uint32 and len(offsets) == len(case[1]) + 1 and offsets[0] == 0
    assert int(offsets[-1]) == len(ops) and (np.diff(offsets.astype(np.int64)) >= 0).all()
    strings, ref = CR.split(offsets, ops), S.cigars(case, ref_scoring(sc), mode)
    wrong = [(r, strings[r][:60], ref[r][:60]) for r in range(len(ref)) if strings[r] != ref[r]]
    assert not wrong, (label, wrong[:4])
    assert all((s == b"") == (st != 0) for s, st in zip(strings, want["status"]))
    for r in range(len(ref)):
        mine = ops[int(offsets[r]):int(offsets[r + 1])]
        sums = [int((mine[(mine & 15) == code] >> 4).sum()) for code in (7, 8, 1, 2)]
        assert sums == [int(rec[f][r]) for f in ("matches", "mismatches", "q_gap", "t_gap")], (label, r)
        if want["status"][r] == 0:
            assert sums[0] + sums[1] + sums[2] == int(rec["q_end"][r] - rec["q_start"][r]), (label, r)
            assert sums[0] + sums[1] + sums[3] == int(rec["t_end"][r] - rec["t_start"][r]), (label, r)


def both_calls(ctx, case, sc, mode, **kw):
    targets, reads, tor, rev = case
    return ctx.align_pairs(targets, reads, tor, rev, scoring=sc, mode=mode, **kw), ctx.align_cigars(targets, reads, tor, rev, scoring=sc, mode=mode, **kw)


def same_bytes(a, b):
    """(align_pairs' records, align_cigars' triple) twice: the same bytes"""
    return (all(a[0][f].tobytes() == b[0][f].tobytes() and a[1][0][f].tobytes() == b[1][0][f].tobytes() for f, _ in R.FIELDS)
            and a[1][1].tobytes() == b[1][1].tobytes() and a[1][2].tobytes() == b[1][2].tobytes())


@pytest.mark.parametrize("name,sc,mode", RUNS, ids=[run_id(r) for r in RUNS])
def test_every_field_and_every_op(gpu_ctx, name, sc, mode):
    case = ALL[name]()
    assert R.cells(case) <= 2_000_000
    pairs_rec, got = both_calls(gpu_ctx, case, sc, mode)
    expect(pairs_rec, got, case, sc, mode, run_id((name, sc, mode)))
    if mode == "read":
        ok = got[0]["status"] == 0
        assert (got[0]["q_start"][ok] == 0).all() and (got[0]["q_end"][ok] == np.array([len(q) for q in case[1]])[ok]).all()


@pytest.mark.parametrize("sc", STANDARD, ids=S.scoring_id)
def test_the_first_of_two_end_cells_wins(gpu_ctx, sc):
    """beside the full comparison: locally the cell (20, Lt) wins over (Lq, 20) -- smaller i, in a higher lane, an earlier block, a later
    refill -- and the read that lies three times in its transcript ends in column 20; in read mode the last row's smallest j wins"""
    case = S.end_order_case()
    pairs_rec, (cigars_rec, _, _) = both_calls(gpu_ctx, case, sc, "local")
    for rec in (pairs_rec, cigars_rec):
        assert (rec["status"] == 0).all() and (rec["q_end"] == 20).all() and (rec["score"] == 20 * ref_scoring(sc)[0]).all()
        assert list(rec["t_end"][S.END_ORDER_LOCAL.start:S.END_ORDER_LOCAL.stop]) == [len(case[0][x]) for x in case[2][:10]]
        assert list(rec["t_end"][S.END_ORDER_READ.start:S.END_ORDER_READ.stop]) == [20, 20]
    pairs_rec, (cigars_rec, _, _) = both_calls(gpu_ctx, case, sc, "read")
    for rec in (pairs_rec, cigars_rec):
        assert list(rec["t_end"][S.END_ORDER_READ.start:S.END_ORDER_READ.stop]) == [20, 20]
        assert list(rec["t_start"][S.END_ORDER_READ.start:S.END_ORDER_READ.stop]) == [0, 0]


@pytest.mark.parametrize("sc", (None, A.ENGINE), ids=S.scoring_id)
@pytest.mark.parametrize("mode", S.MODES)
def test_the_long_pair_alone_in_its_sub_chunk(gpu_ctx, sc, mode):
    """kernel F with the cap on code bytes below what the 18-block pair needs: it runs alone, between sub-chunks of small pairs, and
    the bytes are those of the run without a cap"""
    long_case, small = S.many_blocks_case(), R.tie_cases()
    case = (small[0][:3] + long_case[0] + small[0][3:], small[1][:3] + long_case[1] + small[1][3:], list(range(7)), [0, 0, 0, 1, 0, 0, 0])
    assert R.cells(case) <= 2_000_000
    base = both_calls(gpu_ctx, case, sc, mode)
    expect(*base, case, sc, mode, "uncapped")
    rec_bytes, k_align, k_cigar = (16, 6, 7) if sc is None else (32, 8, 9)
    want = S.records(case, ref_scoring(sc), mode)
    need = [rec_bytes * ((int(want["q_end"][r] - want["q_start"][r]) + 63) // 64) * (int(want["t_end"][r] - want["t_start"][r]) + 63) for r in range(7)]
    cap = 3 * max(need[:3] + need[4:])                                   # holds the three small pairs on either side, not the long one
    assert (int(want["q_end"][3] - want["q_start"][3]) + 63) // 64 >= 17 and need[3] > 20 * cap
    gpu_ctx.reset_stats()
    os.environ["RATTLE_CIGAR_CODE_BYTES"] = str(cap)
    try:
        capped = both_calls(gpu_ctx, case, sc, mode)
    finally:
        del os.environ["RATTLE_CIGAR_CODE_BYTES"]
    assert gpu_ctx.kernel_stats(k_cigar)[1] == 3 and gpu_ctx.kernel_stats(k_align)[1] == 2      # small, the long pair, small; kernel E once per call
    assert same_bytes(capped, base)


@pytest.mark.parametrize("name", S.SHIFTED + ("strand_edges",))
@pytest.mark.parametrize("sc", (None, A.ENGINE), ids=S.scoring_id)
@pytest.mark.parametrize("mode", S.MODES)
def test_the_pair_chunk_changes_nothing(gpu_ctx, name, sc, mode):
    """chunks of one pair and of five: the bytes of the run in one chunk, which the comparison above holds against the reference"""
    case = ALL[name]()
    base = both_calls(gpu_ctx, case, sc, mode)
    for chunk in (1, 5):
        assert same_bytes(both_calls(gpu_ctx, case, sc, mode, pair_chunk=chunk), base), chunk
