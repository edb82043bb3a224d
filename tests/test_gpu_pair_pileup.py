"""Kernel G (csrc/pair_pileup.hip) against the contract in plain Python (tests/pileup_ref.py): the table of `align_pileup`, count for
count, against the model's records and CIGARs (tests/align_model.py) and against the CIGARs the same call returned; beside it the records
and the CIGARs themselves.  Linear / 5,4,8,6 / 2,4,4,2 crossed with local / read.  The cases of align_ref, cigar_ref, align_affine_ref
and align_ends_ref; pairs of 63, 64, 65, 127, 128 and 129 ops (a round of kernel G takes 64); one '=' run, one D run and one I run
across a column step of 64; a pair of one column; 4096 reads on the same 70 positions; targets side by side; the read mode's overhangs;
the pair chunk and the cap on kernel F's code bytes change nothing; kernel id 11 of the stats; the other calls never launch it."""
import os

import numpy as np
import pytest

import align_affine_ref as AF
import align_ends_ref as AE
import align_model as M
import align_ref as R
import cigar_ref as CR
import pileup_ref as P

pytestmark = pytest.mark.gpu


def scoring_of(sc):
    """the linear form is the call without a scoring: the two-state kernels E and F"""
    return None if tuple(sc) == P.LINEAR else sc


def run(ctx, case, sc, mode, **kw):
    return ctx.align_pileup(*case, scoring=scoring_of(sc), mode=mode, **kw)


def stacked(planes):
    return np.array(planes, np.int64).reshape(8, -1)


def got_table(table):
    assert all(table[f].dtype == np.uint32 for f in P.FIELDS)
    return np.stack([table[f].astype(np.int64) for f in P.FIELDS])


def expect(ctx, name, case, sc, mode, max_cells=0, **kw):
    """the call with its CIGARs: records and CIGARs are the model's, the table is pileup_ref's over the model's records and CIGARs and
    over those the call returned; returns what the call returned"""
    rec, cg, table = run(ctx, case, sc, mode, cigars=True, max_cells=max_cells, **kw)
    want_rec, want_cg, want = P.model(name, case, sc, mode, max_cells)
    bad = R.same(rec, want_rec)
    assert not bad, (name, sc, mode, bad[:8])
    strings = CR.split(*cg)
    assert strings == want_cg, (name, sc, mode)
    got = got_table(table)
    assert got.shape == (8, sum(len(t) for t in case[0]))
    for label, ref in (("model", want), ("own CIGARs", P.table(*case, rec, strings))):
        diff = np.argwhere(got != stacked(ref))
        assert not len(diff), (name, sc, mode, label, [(P.FIELDS[k], int(j), int(got[k, j]), ref[k][j]) for k, j in diff[:6]])
    assert P.identities(P.as_lists(table), rec) == []
    return rec, cg, table


def _builder_cases():
    """(name, scoring, mode): edge_case and path_case under all six forms; the other builders of the two per-mode modules under the forms
    their own tests run them in, cut to the three scorings"""
    out = [(name, sc, mode) for name in ("edges", "paths") for sc, mode in P.FORMS]
    for mode, ref in ((M.LOCAL, AF), (M.READ, AE)):
        for name in sorted(ref.all_cases()):
            if name in ("edges", "paths"):                                # (above, under all six)
                continue
            scorings = (P.LINEAR, P.ENGINE, P.MM2) if name in ref.EDGE_CASES else (P.LINEAR, P.ENGINE)
            out += [(name, sc, mode) for sc in scorings]
    return out


@pytest.mark.parametrize("name,sc,mode", _builder_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_the_table_of_the_existing_cases(gpu_ctx, name, sc, mode):
    case = AE.all_cases()[name]()                                         # (align_affine_ref's, and its own)
    assert R.cells(case) <= 2_000_000
    expect(gpu_ctx, name, case, sc, mode)


@pytest.mark.parametrize("name", sorted(P.op_count_pairs()))
def test_pairs_of_63_to_129_ops(gpu_ctx, name):
    sc, mode, ops, q, t = P.op_count_pairs()[name]
    rec, (offsets, _), _ = expect(gpu_ctx, "ops_" + name, R.pairs_case([(q, t, 0)]), sc, mode)
    assert int(offsets[1]) == ops


@pytest.mark.parametrize("sc,mode", P.FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_one_run_across_a_column_step(gpu_ctx, sc, mode):
    """identical pairs of 1, 63, 64, 65, 129 bases (the first is the pair of one column); D and I runs of 63, 64, 65"""
    rec, _, table = expect(gpu_ctx, "identical", P.identical_case(), sc, mode)
    assert int(got_table(table)[:4].sum()) == 1 + 63 + 64 + 65 + 129 and int(table["starts"].sum()) == 5
    expect(gpu_ctx, "long_gaps", P.long_gap_case(), sc, mode)


def test_long_gaps_are_one_run_under_the_engines_scoring(gpu_ctx):
    _, cg, table = expect(gpu_ctx, "long_gaps", P.long_gap_case(), P.ENGINE, M.LOCAL)
    assert CR.split(*cg) == [b"120=%d%s120=" % (n, o) for n in (63, 64, 65) for o in (b"D", b"I")]
    assert int(table["ins"].sum()) == 3 and int(table["del"].sum()) == 63 + 64 + 65


def test_contention_4096_reads_on_70_positions(gpu_ctx):
    case = P.contention_case()
    n = P.CONTENTION_COPIES
    for cigars in (False, True):
        rec, _, table = run(gpu_ctx, case, P.LINEAR, M.LOCAL, cigars=cigars)
        assert (rec["status"] == 0).all() and (rec["matches"] == 70).all()
        got = got_table(table)
        t = case[0][0]
        for j in range(70):
            want = [n if b"ACGT"[k] == t[j] else 0 for k in range(4)] + [0, 0, n if j == 0 else 0, n if j == 69 else 0]
            assert list(got[:, j]) == want, j


@pytest.mark.parametrize("sc,mode", P.FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_neighbouring_targets_and_reads_that_add_nothing(gpu_ctx, sc, mode):
    case = P.neighbours_case()
    rec, _, table = expect(gpu_ctx, "neighbours", case, sc, mode, max_cells=P.NEIGHBOURS_MAX_CELLS)
    assert list(rec["status"]) == [0, 0, 0, 0, 3, 1, 2]
    got = got_table(table)
    assert not got[:, 170:].any()                                         # target 2 is not used
    if mode == M.LOCAL:
        assert got[P.ENDS, 79] == 2 and got[P.STARTS, 80] == 2 and got[:5, 79].sum() == 2 and got[:5, 80].sum() == 2
    assert got[P.STARTS].sum() == 4 and got[P.STARTS, :80].sum() == 2 and got[P.ENDS, 80:].sum() == 2      # no count crosses
    # nothing submitted at all, and no read at all: a table of zeros over the targets
    for reads, tor in (([b"ACGT", b""], [-1, -1]), ([], [])):
        rec, cg, table = gpu_ctx.align_pileup(case[0], reads, tor, [0] * len(reads), scoring=scoring_of(sc), mode=mode, cigars=True)
        assert got_table(table).shape == (8, 220) and not got_table(table).any() and len(cg[1]) == 0


def test_read_mode_overhangs_and_a_pair_without_a_column(gpu_ctx):
    case = P.read_mode_case()
    _, cg, table = expect(gpu_ctx, "read_mode", case, P.ENGINE, M.READ)
    inner = sum(sum(o == b"I" for o, _ in P.parse(s)[1:-1]) for s in CR.split(*cg))
    assert inner >= 3 and int(table["ins"].sum()) == inner                # leading and trailing I runs add nothing
    none = R.pairs_case([(b"CC", b"AA", 0), (b"C" * 70, b"A" * 5, 0)])
    rec, cg, table = expect(gpu_ctx, "no_columns", none, AE.CHEAP_GAP, M.READ)
    assert CR.split(*cg) == [b"2I", b"70I"] and list(rec["status"]) == [0, 0] and not got_table(table).any()
    rec2, cg2, table2 = run(gpu_ctx, none, AE.CHEAP_GAP, M.READ)
    assert cg2 is None and not got_table(table2).any() and not R.same(rec2, rec)


def sub_chunks(rec, cap, rec_bytes=16):
    """the sub-chunks of kernel F as csrc/cigar_plan.h closes them under a cap on the code bytes"""
    n_sub, held = 1, 0
    for r in np.nonzero((rec["status"] == 0) & (rec["t_end"] > rec["t_start"]))[0]:
        rows, cols = int(rec["q_end"][r] - rec["q_start"][r]), int(rec["t_end"][r] - rec["t_start"][r])
        need = rec_bytes * ((rows + 63) // 64) * (cols + 63)
        if held and held + need > cap:
            n_sub, held = n_sub + 1, 0
        held += need
    return n_sub


def alg_bytes(rec, strings):
    """id 11 as include/rattle_hip.h defines it: per aligned pair with a column 4 ops + R + 4 (matches + mismatches + t_gap + internal I
    ops + 2)"""
    total = 0
    for r in np.nonzero((rec["status"] == 0) & (rec["t_end"] > rec["t_start"]))[0]:
        ops = P.parse(strings[r])
        total += 4 * len(ops) + int(rec["q_end"][r] - rec["q_start"][r])
        total += 4 * (int(rec["matches"][r]) + int(rec["mismatches"][r]) + int(rec["t_gap"][r]) + sum(o == b"I" for o, _ in ops[1:-1]) + 2)
    return total


@pytest.mark.parametrize("sc,mode", [(P.LINEAR, M.LOCAL), (P.ENGINE, M.READ)], ids=lambda v: str(v).replace(" ", ""))
def test_the_chunks_and_the_cap_change_nothing_and_kernel_g_is_kernel_11(gpu_ctx, sc, mode):
    case = R.edge_case()
    gpu_ctx.reset_stats()
    rec, cg, table = expect(gpu_ctx, "edges", case, sc, mode)
    strings = CR.split(*cg)
    aligned = int(((rec["status"] == 0) & (rec["t_end"] > rec["t_start"])).sum())
    nbytes = alg_bytes(rec, strings)
    ms, launches, got = gpu_ctx.kernel_stats(11)
    assert (launches, got) == (1, nbytes) and ms >= 0
    base = got_table(table)
    for chunk in (1, 3):
        gpu_ctx.reset_stats()
        rec2, cg2, table2 = run(gpu_ctx, case, sc, mode, cigars=True, pair_chunk=chunk)
        assert (got_table(table2) == base).all() and not R.same(rec2, rec) and cg2[1].tobytes() == cg[1].tobytes(), chunk
        # kernel E's chunks hold `chunk` pairs (every read of the case is submitted); each goes to kernel F whole, as one sub-chunk
        assert (rec["status"] < 2).all()
        alive = list((rec["status"] == 0) & (rec["t_end"] > rec["t_start"]))
        with_ops = sum(any(alive[i:i + chunk]) for i in range(0, len(alive), chunk))
        assert gpu_ctx.kernel_stats(11)[1:] == (with_ops, nbytes), chunk
    assert aligned > 40
    rec_bytes = 16 if scoring_of(sc) is None else 32
    gpu_ctx.reset_stats()
    os.environ["RATTLE_CIGAR_CODE_BYTES"] = "10000"                       # holds a few of the case's pairs; the largest need more alone
    try:
        rec3, cg3, table3 = run(gpu_ctx, case, sc, mode, cigars=True)
        no_ops = run(gpu_ctx, case, sc, mode)
    finally:
        del os.environ["RATTLE_CIGAR_CODE_BYTES"]
    n_sub = sub_chunks(rec, 10000, rec_bytes)
    assert n_sub > 5 and gpu_ctx.kernel_stats(11)[1:] == (2 * n_sub, 2 * nbytes)
    assert gpu_ctx.kernel_stats(7 if rec_bytes == 16 else 9)[1] == 2 * n_sub
    for t in (table3, no_ops[2]):
        assert (got_table(t) == base).all()
    assert not R.same(rec3, rec) and cg3[1].tobytes() == cg[1].tobytes() and cg3[0].tobytes() == cg[0].tobytes()


@pytest.mark.parametrize("sc,mode", P.FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_without_the_cigars_the_table_and_the_records_are_the_same(gpu_ctx, sc, mode):
    case = CR.path_case()
    rec, cg, table = run(gpu_ctx, case, sc, mode, cigars=True)
    rec2, cg2, table2 = run(gpu_ctx, case, sc, mode)
    assert cg2 is None and not R.same(rec2, rec)
    assert (got_table(table2) == got_table(table)).all() and got_table(table).any()
    # ... and both are what align_cigars returns
    rec3, offsets, ops = gpu_ctx.align_cigars(*case, scoring=scoring_of(sc), mode=mode)
    assert not R.same(rec3, rec) and offsets.tobytes() == cg[0].tobytes() and ops.tobytes() == cg[1].tobytes()


def test_the_other_calls_never_launch_kernel_g(gpu_ctx):
    case = CR.path_case()
    gpu_ctx.reset_stats()
    gpu_ctx.align_pairs(*case)
    gpu_ctx.align_cigars(*case)
    gpu_ctx.align_cigars(*case, scoring=P.ENGINE, mode="read")
    assert gpu_ctx.kernel_stats(11)[1:] == (0, 0) and gpu_ctx.kernel_stats(7)[1] == 1 and gpu_ctx.kernel_stats(9)[1] == 1
    run(gpu_ctx, case, P.LINEAR, M.LOCAL)
    assert gpu_ctx.kernel_stats(11)[1] == 1 and gpu_ctx.kernel_stats(7)[1] == 2
