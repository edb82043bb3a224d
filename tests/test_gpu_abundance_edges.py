"""The abundance EM on the device (csrc/abundance.hip) where tests/test_gpu_abundance.py does not reach, against `vector` of
tests/abundance_ref.py by their bits: the scan of more than 1024 histogram entries (every real transcriptome), more than 8 distinct
targets in a later slot of a wavefront inside one run (what em_add_matched leaves to the lanes themselves), whole wavefronts of reads
without a candidate, the lists no assignment makes (a target twice in a read, an incompatible slot in front of a compatible one, a
negative best score), abundances above 2^53 units with a target that decays to exactly 0 while reads still name it, and the plain
scatter of RATTLE_EM_PLAIN=1 on the same lists.  Every case first asserts, from the list alone, that it holds what it is named for."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import abundance_ref as ref
from conftest import ROOT
from test_gpu_abundance import both, expect

pytestmark = pytest.mark.gpu

ONE = ref.ONE


def exact(ctx, cands, nt, label, **kw):
    got = both(ctx, cands, nt, label, **kw)
    assert int(got["units"].sum()) == got["n_placed"] * ONE, label
    return got


@pytest.mark.parametrize("empties", [False, True], ids=["all_placed", "with_empties"])
@pytest.mark.parametrize("nt", ref.SCAN_NT)
def test_the_scan_across_its_rounds_of_1024_entries(gpu_ctx, nt, empties):
    cands = ref.scan_rounds_case(nt, empties)
    assert ref.scan_rounds_holds(cands, nt, empties) and nt + 1 > ref.SCAN - 1
    got = exact(gpu_ctx, cands, nt, f"nt={nt} empties={empties}", max_iters=40)
    assert got["n_placed"] == int((cands["count"] > 0).sum())


@pytest.mark.parametrize("nt,unnamed", ref.SCAN_UNNAMED)
def test_the_scan_with_an_unnamed_index_at_a_round_edge(gpu_ctx, nt, unnamed):
    cands = ref.scan_rounds_case(nt, True, unnamed)
    assert ref.scan_rounds_holds(cands, nt, True, unnamed)
    got = exact(gpu_ctx, cands, nt, f"nt={nt} unnamed={unnamed}", max_iters=40)
    assert got["units"][unnamed] == 0 and got["compatible_reads"][unnamed] == 0


@pytest.mark.parametrize("distinct", [9, 8])
def test_nine_and_eight_distinct_targets_in_slot_1_of_a_one_run_wavefront(gpu_ctx, distinct):
    """9: the ninth target's seven lanes add for themselves; 8: nobody does"""
    cands = ref.leftover_case(distinct)
    assert ref.leftover_holds(cands, distinct) and (distinct > ref.SUMMED) == (distinct == 9)
    got = exact(gpu_ctx, cands, ref.LEFTOVER_NT, f"{distinct} distinct")
    assert got["n_placed"] == 94 and (got["compatible_reads"][1:distinct + 1] >= 7).all()


@pytest.mark.parametrize("alone_every", [0, 5], ids=["every_read_spread", "every_fifth_alone"])
def test_more_than_eight_distinct_targets_in_every_later_slot(gpu_ctx, alone_every):
    cands = ref.spread_case(alone_every)
    assert ref.spread_holds(cands, alone_every)
    got = exact(gpu_ctx, cands, ref.SPREAD_NT, f"spread, alone_every={alone_every}", max_iters=60)
    assert got["n_placed"] == 256 and got["compatible_reads"][0] == 256


def test_whole_wavefronts_of_reads_without_a_candidate(gpu_ctx):
    cands, nt = ref.empty_wavefront_case()
    assert ref.empty_wavefronts(cands) == 2 and int((cands["count"] == 0).sum()) == 200
    got = exact(gpu_ctx, cands, nt, "200 empties beside 100 placed", max_iters=60)
    assert got["n_placed"] == 100 and not got["posterior"][cands["count"] == 0].any()
    cands, nt = ref.run_to_the_edge_case()
    t0 = ref.slot0(cands)
    assert ref.empty_wavefronts(cands) == 1 and len(t0) % ref.WAVE == 0 and int((t0 == t0.max()).sum()) == 130
    got = exact(gpu_ctx, cands, nt, "a run of 130 up to the wavefront edge, then empties", max_iters=60)
    assert got["n_placed"] == 192 and got["compatible_reads"][:2].tolist() == [62, 130]


@pytest.mark.parametrize("k", [4, 8])
def test_lists_no_assignment_would_make(gpu_ctx, k):
    cands = ref.odd_lists(k)
    assert ref.odd_holds(cands) == (True, True, True)
    got = exact(gpu_ctx, cands, ref.ODD_NT, f"odd lists, k={k}", ratio=ref.ODD_RATIO, max_iters=50)
    assert got["compatible_reads"].max() <= len(cands["count"])


def test_a_target_twice_in_a_read_and_a_hole_by_hand(gpu_ctx):
    cands = ref.odd_hand()
    assert ref.odd_holds(cands)[:2] == (True, True)
    assert ref.compatible(cands, ref.ODD_RATIO).tolist() == [[True, True, True], [True, True, True], [True, False, True]]
    got = exact(gpu_ctx, cands, ref.ODD_NT, "odd lists by hand", ratio=ref.ODD_RATIO, max_iters=50)
    assert got["compatible_reads"].tolist() == ref.ODD_HAND_COMPATIBLE and got["units"][2] == ONE and got["units"][4] == 0


@pytest.mark.parametrize("handing_over", [0, 10])
def test_abundances_above_2_to_the_53(gpu_ctx, handing_over):
    """2^21 + 5000 reads on target 0 (2^21 + 1 is the fewest that pass 2^53 units): uint64 -> double rounds in em_shares, est_reads
    and cpm.  Target 1 decays to exactly 0 while 3000 reads name it; with 10 reads (1, 0) it settles at exactly 10 units."""
    cands = ref.beyond_2_53_case(handing_over)
    n = ref.BEYOND_N + handing_over
    want = ref.vector(cands, 2, tol=0.0, max_iters=8)
    assert int(want["units"][0]) > 2 ** 53 and want["units"].tolist() == [n * ONE - handing_over, handing_over]
    assert want["compatible_reads"].tolist() == [n, 3000 + handing_over] and want["converged"] == 1 and want["delta"][-1] == 0
    if not handing_over:
        assert want["delta"].tolist() == [6433256865000, 9180960000, 13101000, 18000, 0]
    assert want["posterior"][:3000].tolist() == [[1.0, 0.0]] * 3000
    got = gpu_ctx.abundance(cands, 2, tol=0.0, max_iters=8)
    expect(got, want, f"above 2^53, {handing_over} handing over")
    assert int(got["units"].sum()) == got["n_placed"] * ONE == n * ONE


# the lists of the plain scatter: (builder, its arguments, n_targets, what Context.abundance takes)
PLAIN = (("scan_rounds_case", (1025, True), 1025, {"max_iters": 40}), ("scan_rounds_case", (3077, False), 3077, {"max_iters": 40}),
         ("spread_case", (0,), ref.SPREAD_NT, {"max_iters": 60}), ("odd_lists", (4,), ref.ODD_NT, {"ratio": ref.ODD_RATIO, "max_iters": 50}),
         ("odd_lists", (8,), ref.ODD_NT, {"ratio": ref.ODD_RATIO, "max_iters": 50}))

CHILD = """
import pickle, sys
sys.path[:0] = [%r, %r]
import abundance_ref as ref
from rattle_amd.api import Context
from test_gpu_abundance_edges import PLAIN
ctx = Context(0)
out = [ctx.abundance(getattr(ref, name)(*args), nt, **kw) for name, args, nt, kw in PLAIN]
ctx.close()
pickle.dump(out, open(sys.argv[1], "wb"))
"""


def test_the_plain_scatter_gives_the_same_bytes_on_these_lists(gpu_ctx, tmp_path):
    """RATTLE_EM_PLAIN=1 in a fresh process (never in this one): no sort, no scan, one atomic per entry"""
    path = tmp_path / "plain.pickle"
    env = dict(os.environ, RATTLE_EM_PLAIN="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), str(path)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = pickle.load(open(path, "rb"))
    assert "RATTLE_EM_PLAIN" not in os.environ and len(plain) == len(PLAIN)
    for (name, args, nt, kw), p in zip(PLAIN, plain):
        expect(p, gpu_ctx.abundance(getattr(ref, name)(*args), nt, **kw), f"plain against merged, {name}{args}")
