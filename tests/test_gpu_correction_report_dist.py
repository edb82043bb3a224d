"""The correction report of ONE `correct` job over several ranks (the ranks share the box's one GPU, the exchange goes through host
buffers, as in tests/test_gpu_dist.py): the report travels with the records rattle_hip_correction_gather merges, so the root's
merged report equals the single-rank one array for array; if one rank made its share with the switch off, the merged result has no
report -- and is otherwise the same result, without an error."""
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, os.environ["RATTLE_ROOT"])
    import torch.distributed as dist
    from rattle_amd import synth
    from rattle_amd._lib import REPORT_FIELDS, RattleError
    from rattle_amd.api import Context
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    cat, qcat, off, tid, _ = synth.reads_packed(1500, 6, 1, True, seed=5, exon=(50, 210))
    ref = None
    if rank == 0:                                  # the single-rank job, own context
        c0 = Context(0)
        cl0 = c0.cluster_unsorted_packed(cat, off)
        c0.set_correction_report(True)
        h = c0.correct_packed(cat, qcat, off, cl0, split=40, keep=True)
        ref = (h.report(), h.digest(), h.counts()[:3])
        h.free()
        c0.close()
    dist.barrier()
    ctx = Context(0)
    ctx.set_exchange_gloo()
    cl = ctx.cluster_unsorted_packed(cat, off)
    # every rank with the switch on
    ctx.set_correction_report(True)
    h = ctx.correct_packed(cat, qcat, off, cl, split=40, gather_root=0, keep=True)
    if rank == 0:
        rep = h.report()
        assert h.digest() == ref[1] and h.counts()[:3] == ref[2], "sharded correct differs"
        assert ref[2][0] > 1000 and len(rep["match"]) == ref[2][0]
        for f in REPORT_FIELDS:
            assert rep[f].dtype == np.uint32 and np.array_equal(rep[f], ref[0][f]), f
        assert all(ref[0][f].sum() > 0 for f in ("match", "substituted", "inserted", "deleted"))
        print("REPORT_EQUAL", world)
    else:
        assert h.ptr is None
    h.free()
    # the last rank with the switch off: the merged result is the same and has no report
    ctx.set_correction_report(rank != world - 1)
    h = ctx.correct_packed(cat, qcat, off, cl, split=40, gather_root=0, keep=True)
    if rank == 0:
        assert h.digest() == ref[1] and h.counts()[:3] == ref[2]
        try:
            h.report()
            print("UNEXPECTED_REPORT")
        except RattleError as e:
            assert "error -3:" in str(e) and "every rank" in str(e), str(e)
            print("NO_REPORT_OK", world)
    h.free()
    ctx.close()
    dist.destroy_process_group()
''')


@pytest.mark.parametrize("world", [2, 3])
def test_gathered_report_equals_the_single_rank_report(tmp_path, world):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, RATTLE_ROOT=ROOT, MASTER_ADDR="127.0.0.1", RATTLE_HOST_THREADS="8")
    env.pop("RATTLE_RCCL_LIB", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29760 + world), str(script)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"REPORT_EQUAL {world}" in r.stdout and f"NO_REPORT_OK {world}" in r.stdout and "UNEXPECTED_REPORT" not in r.stdout
