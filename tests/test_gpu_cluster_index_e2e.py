"""The "index" count pass end to end: `rattle cluster` and `rattle cluster --iso` with `--count-pass index` against `seed` and
`search`, every setting in a fresh child process (the library reads the setting once per process), output files compared byte for
byte; and one job over two ranks with RATTLE_PAIR_COUNT=index against the single-rank result.

An unknown value of the setting means "search", so equal files alone would not show that the new pass ran: every child runs with
RATTLE_TIMING=1 and the driver's line `count pass of the evaluations with survivors: seed A, search B, index C` is read back --
the forced form must be the only one that ran, and must have run.  Every child has its own time limit and is run once; a child
that fails ends the test there."""
import gzip
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from rattle_amd import synth

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
FORMS = ("seed", "search", "index")
LINE = re.compile(r"count pass of the evaluations with survivors: seed (\d+), search (\d+), index (\d+)")


def forms_that_ran(stderr):
    """sum of the driver's per-clustering lines: evaluations per form"""
    rows = [tuple(int(x) for x in m.groups()) for m in LINE.finditer(stderr)]
    assert rows, stderr[-2000:]
    return dict(zip(FORMS, np.sum(rows, axis=0).tolist()))


def cluster(fq, out, form, extra, env_extra=None, flag=True):
    out.mkdir()
    env = dict(os.environ, RATTLE_TIMING="1", **(env_extra or {}))
    env.pop("RATTLE_PAIR_COUNT", None)
    if not flag:
        env["RATTLE_PAIR_COUNT"] = form
    cmd = [RATTLE, "cluster", "-i", str(fq), "-o", str(out)] + extra + (["--count-pass", form] if flag else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (form, r.returncode, r.stderr[-3000:])
    ran = forms_that_ran(r.stderr)
    assert ran[form] > 0 and all(ran[f] == 0 for f in FORMS if f != form), (form, ran)
    return (out / "clusters.out").read_bytes(), ran


def mixed_reads(path):
    """3000 reads of 150 nt - 20 kb (log-uniform transcript lengths with a tail of long ones), both strands"""
    tx = synth.mixed_transcriptome(60, seed=77, lo=150, hi=20000, body_hi=6000, tail_frac=0.12)
    cat, qcat, off, _, _ = synth.reads_packed(3000, 0, 1, True, seed=78, tx=tx)
    lens = np.diff(off.astype(np.int64))
    assert lens.max() > 15000 and lens.min() < 400 and (lens > 4000).sum() > 100, (lens.min(), lens.max())
    seqs = [cat[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(lens))]
    quals = [qcat[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(lens))]
    path.write_bytes(synth.fastq_text(seqs, quals))


@pytest.mark.parametrize("iso", [False, True], ids=["gene", "iso"])
def test_toyset_clusters_do_not_depend_on_the_count_pass(tmp_path, iso):
    assert os.path.exists(RATTLE)
    fq = tmp_path / "sample.fastq"
    fq.write_bytes(gzip.open(os.path.join(GOLDEN, "toyset_rna.fastq.gz")).read())
    extra = ["--rna", "--lower-length", "0", "-t", "4"] + (["--iso"] if iso else [])
    outs = {f: cluster(fq, tmp_path / f, f, extra) for f in FORMS}
    for f in ("seed", "search"):
        assert outs["index"][0] == outs[f][0], f
    assert len(outs["index"][0]) > 1000
    # every form ran the same evaluations
    assert outs["index"][1]["index"] == outs["seed"][1]["seed"] == outs["search"][1]["search"]
    if not iso:
        from rattle_amd import hps
        want = hps.decode(open(os.path.join(GOLDEN, "toyset_rna.clusters.out"), "rb").read(), fields=2)
        assert hps.decode(outs["index"][0], fields=3) == want      # the shipped fixture (as tests/test_gpu_cli.py reads it)
    # the environment variable selects the pass as the flag does, and a small entry cap (several index builds per evaluation) changes nothing
    env_out, _ = cluster(fq, tmp_path / "env", "index", extra, env_extra={"RATTLE_INDEX_ENTRIES": "200000"}, flag=False)
    assert env_out == outs["index"][0]


@pytest.mark.parametrize("iso", [False, True], ids=["gene", "iso"])
def test_mixed_length_clusters_do_not_depend_on_the_count_pass(tmp_path, iso):
    assert os.path.exists(RATTLE)
    fq = tmp_path / "mixed.fastq"
    mixed_reads(fq)
    extra = ["--iso"] if iso else []
    outs = {f: cluster(fq, tmp_path / f, f, extra) for f in FORMS}
    for f in ("seed", "search"):
        assert outs["index"][0] == outs[f][0], f
    assert len(outs["index"][0]) > 1000


WORKER = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, os.environ["RATTLE_ROOT"])
    import torch.distributed as dist
    from rattle_amd import synth
    from rattle_amd.api import Context
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    cat, qcat, off, tid, _ = synth.reads_packed(4000, 14, 3, True, seed=21, exon=(50, 210))
    ref = None
    if rank == 0:                                  # unsharded reference, same process, own context
        c0 = Context(0)
        cl0 = c0.cluster_unsorted_packed(cat, off)
        iso0, gid0, ng0 = c0.cluster_iso_unsorted_packed(cat, off)
        ref = (cl0.as_list(), iso0.as_list(), list(gid0), ng0, [int(x) for x in cl0.counters[:3]])
        c0.close()
    dist.barrier()
    ctx = Context(0)
    ctx.set_exchange_gloo()
    cl = ctx.cluster_unsorted_packed(cat, off)
    iso, gid, ng = ctx.cluster_iso_unsorted_packed(cat, off)
    calls, nbytes = ctx.comm_stats()
    assert calls > 0 and nbytes > 0
    if rank == 0:
        assert cl.as_list() == ref[0], "sharded gene-level clusters differ"
        assert [int(x) for x in cl.counters[:3]] == ref[4], ("work counters differ", [int(x) for x in cl.counters[:3]], ref[4])
        assert iso.as_list() == ref[1] and list(gid) == ref[2] and ng == ref[3], "sharded --iso clusters differ"
        print("INDEX_DIST_OK", world, len(ref[0]), len(ref[1]), ref[4])
    ctx.close()
    dist.destroy_process_group()
''')


def test_sharded_job_with_the_index_pass_equals_single_rank(tmp_path):
    """world 2 on the one GPU (host exchange): clusters at both levels and the work counters [0..2] (pair tests, comparisons, k-mer
    matches: k = 10, so the index pass's matches are exact and add up over the ranks) equal the single-rank run's."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, RATTLE_ROOT=ROOT, MASTER_ADDR="127.0.0.1", RATTLE_HOST_THREADS="8", RATTLE_PAIR_COUNT="index", RATTLE_TIMING="1")
    env.pop("RATTLE_RCCL_LIB", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29761", str(script)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "INDEX_DIST_OK 2" in r.stdout
    ran = forms_that_ran(r.stderr)
    assert ran["index"] > 0 and ran["seed"] == 0 and ran["search"] == 0, ran
