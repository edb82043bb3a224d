"""The abundance EM on the device (csrc/abundance.hip) against the rule in tests/abundance_ref.py, on hand-built candidate lists through
Context.abundance: units, compatible_reads, delta, iterations, converged, n_placed, posterior and the two derived doubles by their bits.
The shapes are the smallest at which each thing can go wrong: the edges of a lane, a wavefront and a workgroup, every k the kernels
unroll over, reads without a candidate at either end, one run of equal targets across whole workgroups and no run at all, runs that
begin on lane 0, end on lane 63 or have length 1, unnamed targets, the compatibility edge, the stop rule, every position of the
convergence inside the host's iteration block, the plain scatter of RATTLE_EM_PLAIN=1, two runs, and no trace left on the context."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import abundance_ref as ref
from conftest import ROOT
from rattle_amd import synth
from test_abundance_ref import example, hand

pytestmark = pytest.mark.gpu


def expect(got, want, label):
    bad = ref.same(got, want)
    assert bad is None, (label, bad, got[bad], want[bad])


def both(ctx, cands, nt, label, **kw):
    got = ctx.abundance(cands, nt, **kw)
    kw.pop("iter_block", None)
    expect(got, ref.vector(cands, nt, **kw), label)
    return got


def runs_case():
    """slot-0 targets with these read counts, in this order once sorted: 64 (lanes 0 .. 63 of the first wavefront: begins on lane 0, ends
    on lane 63), 1, 62, 1 (a run of length 1 between long ones, the second ending on lane 63), 63, 1 (ends on lane 63), 130 (begins on
    lane 0, covers two wavefronts and ends inside a third), 1, 1, 1, 70, 0 (a target nobody names), 5; 401 reads, two workgroups.  Slot 1
    names the target two further on for every second read and slot 2 target 0 for every third, shuffled: runs in the later slots too."""
    counts = [64, 1, 62, 1, 63, 1, 130, 1, 1, 1, 70, 0, 5]
    nt = len(counts)
    t0 = np.repeat(np.arange(nt), counts)
    rng = np.random.default_rng(11)
    t0 = t0[rng.permutation(len(t0))]
    rows = []
    for i, t in enumerate(t0):
        row = [(int(t), 0.8)]
        if i % 2 == 0:
            row.append((int((t + 2) % nt) if (t + 2) % nt != 11 else 12, 0.79))
        if i % 3 == 0 and t != 0 and len(row) == 2:
            row.append((0, 0.78))
        rows.append(row)
    return hand(rows, 3), nt


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_lane_wavefront_and_workgroup_edges(gpu_ctx, n, k):
    rng = np.random.default_rng(100 * n + k)
    nt = 24
    cands = ref.lists(n, k, nt, rng, empty=0.1)
    got = both(gpu_ctx, cands, nt, f"n={n} k={k}", max_iters=40)
    assert got["n_placed"] == int((cands["count"] > 0).sum()) and int(got["units"].sum()) == got["n_placed"] * ref.ONE


def test_reads_without_a_candidate_at_the_first_a_middle_and_the_last_position(gpu_ctx):
    rng = np.random.default_rng(7)
    cands = ref.lists(130, 4, 16, rng)
    for r in (0, 64, 129):
        cands["count"][r] = 0
        cands["target"][r] = -1
        cands["score"][r] = -1.0
    got = both(gpu_ctx, cands, 16, "empties", max_iters=60)
    assert got["n_placed"] == 127 and not got["posterior"][[0, 64, 129]].any()
    none = {"count": np.zeros(70, np.uint32), "target": np.full((70, 2), -1, np.int32), "score": np.full((70, 2), -1.0)}
    got = both(gpu_ctx, none, 3, "no read placed")
    assert got["n_placed"] == 0 and got["iterations"] == 1 and not got["units"].any()
    for cands, nt in ((hand([], 3), 4), (none, 0)):
        got = both(gpu_ctx, cands, nt, "empty input")
        assert got["iterations"] == 0 and got["converged"] == 1 and got["posterior"].shape == cands["target"].shape


def test_one_run_across_whole_workgroups_and_no_run_at_all(gpu_ctx):
    one = hand([[(2, 0.5)]] * 700, 1)
    got = both(gpu_ctx, one, 4, "every read on one target")
    assert got["units"].tolist() == [0, 0, 700 * ref.ONE, 0] and got["compatible_reads"].tolist() == [0, 0, 700, 0] and got["iterations"] == 1
    shared = hand([[(2, 0.5), (1, 0.5)]] * 700, 2)
    got = both(gpu_ctx, shared, 4, "every read on the same two targets", max_iters=20)
    assert got["units"][1] + got["units"][2] == 700 * ref.ONE
    apart = hand([[(r, 0.5), ((r + 1) % 300, 0.49)] for r in range(300)], 2)
    got = both(gpu_ctx, apart, 300, "every lane on a different target", max_iters=20)
    assert (got["compatible_reads"] == 2).all()
    got = both(gpu_ctx, hand([[(0, 0.5)]] * 130, 1), 1, "n_targets = 1")
    assert got["units"].tolist() == [130 * ref.ONE] and got["cpm"].tolist() == [1e6]


def test_runs_that_begin_on_lane_0_end_on_lane_63_or_have_length_1(gpu_ctx):
    cands, nt = runs_case()
    got = both(gpu_ctx, cands, nt, "runs", max_iters=50)
    assert got["units"][11] == 0 and got["compatible_reads"][11] == 0 and got["est_reads"][11] == 0.0     # the target nobody names


def test_the_family_draw(gpu_ctx):
    cands = ref.lists(600, 8, 40, np.random.default_rng(0))
    got = both(gpu_ctx, cands, 40, "family draw")
    assert got["converged"] == 1 and 50 < got["iterations"] < 1000 and int(got["units"].sum()) == 600 * ref.ONE
    assert ref.same(got, gpu_ctx.abundance(cands, 40)) is None                                              # two runs: the same bytes


def test_the_ratio_edge_pair(gpu_ctx):
    top, ratio = 0.7, 0.95
    edge = ratio * top
    inside = hand([[(0, top), (1, edge)]] * 3 + [[(0, top)]], 2)
    outside = hand([[(0, top), (1, np.nextafter(edge, 0.0))]] * 3 + [[(0, top)]], 2)
    got = both(gpu_ctx, inside, 2, "at the ratio", ratio=ratio)
    assert got["compatible_reads"].tolist() == [4, 3] and got["units"][1] > 0
    got = both(gpu_ctx, outside, 2, "one ulp below", ratio=ratio)
    assert got["compatible_reads"].tolist() == [4, 0] and got["units"].tolist() == [4 * ref.ONE, 0]


def test_the_stop_rule_and_the_iteration_block(gpu_ctx):
    c = example()
    want = ref.scalar(c, 2)
    assert want["iterations"] == 10 and want["converged"] == 1
    for block in (0, 1, 5, 7, 10, 32):                   # the convergence at the end of, inside and past a block of the host
        expect(gpu_ctx.abundance(c, 2, iter_block=block), want, f"iter_block {block}")
    short = both(gpu_ctx, c, 2, "tol 0", tol=0.0, max_iters=5)
    assert short["converged"] == 0 and short["iterations"] == 5 and short["delta"].tolist() == want["delta"].tolist()[:5]
    for block in (1, 2, 5, 32):
        expect(gpu_ctx.abundance(c, 2, tol=0.0, max_iters=5, iter_block=block), short, f"tol 0, iter_block {block}")
    cands = ref.lists(300, 8, 40, np.random.default_rng(3))
    long = both(gpu_ctx, cands, 40, "family, 70 iterations", tol=0.0, max_iters=70)
    for block in (1, 7, 33, 70):                         # several full blocks and a shorter last one
        expect(gpu_ctx.abundance(cands, 40, tol=0.0, max_iters=70, iter_block=block), long, f"family, iter_block {block}")


CHILD = """
import pickle, sys
sys.path[:0] = [%r, %r]
import numpy as np
import abundance_ref as ref
from rattle_amd.api import Context
from test_gpu_abundance import runs_case
ctx = Context(0)
runs, nt = runs_case()
out = [ctx.abundance(ref.lists(600, 8, 40, np.random.default_rng(0)), 40), ctx.abundance(runs, nt, max_iters=50),
       ctx.abundance(ref.lists(1025, 2, 24, np.random.default_rng(5), empty=0.1), 24, max_iters=40, iter_block=7)]
ctx.close()
pickle.dump(out, open(sys.argv[1], "wb"))
"""


def test_the_plain_scatter_gives_the_same_bytes(gpu_ctx, tmp_path):
    """RATTLE_EM_PLAIN=1 in a fresh process: one atomic per entry, no sort, no merge"""
    path = tmp_path / "plain.pickle"
    env = dict(os.environ, RATTLE_EM_PLAIN="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), str(path)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = pickle.load(open(path, "rb"))
    runs, nt = runs_case()
    assert "RATTLE_EM_PLAIN" not in os.environ
    merged = [gpu_ctx.abundance(ref.lists(600, 8, 40, np.random.default_rng(0)), 40), gpu_ctx.abundance(runs, nt, max_iters=50),
              gpu_ctx.abundance(ref.lists(1025, 2, 24, np.random.default_rng(5), empty=0.1), 24, max_iters=40)]
    for i, (p, m) in enumerate(zip(plain, merged)):
        expect(p, m, f"plain against merged, list {i}")


def test_abundance_leaves_the_context_as_it_was(gpu_ctx):
    """assign_loaded_top before and after an abundance call on the same loaded reads: the same list, and kernel id 10 counted the call"""
    seqs = synth.reads(300, 7, 3, True, seed=5, exon=(40, 90))[0]
    gpu_ctx.load_reads(seqs, 10, True)
    ids = np.arange(len(seqs), dtype=np.uint32)
    rec, before = gpu_ctx.assign_loaded_top(ids[:40], ids[40:], 8)
    gpu_ctx.reset_stats()
    got = both(gpu_ctx, before, 40, "the list of assign_loaded_top")
    ms, launches, _ = gpu_ctx.kernel_stats(10)
    assert launches >= 2 * got["iterations"] + 3 and all(gpu_ctx.kernel_stats(i)[1] == 0 for i in range(10))
    assert got["n_placed"] == int((rec["target"] >= 0).sum()) > 50 and (before["count"] > 1).sum() > 0
    rec2, after = gpu_ctx.assign_loaded_top(ids[:40], ids[40:], 8)
    for f in before:
        assert before[f].tobytes() == after[f].tobytes(), f
