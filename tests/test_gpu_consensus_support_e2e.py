"""The consensus support end to end: `correct` with rattle_hip_set_consensus_support on, replayed in Python with the oracle.

Input: synthetic reads of about 150 nt in four clusters, corrected with split=4, min_reads=2:
  cluster 0   4 reads: one pack, its consensus is the cluster's (level 2);
  cluster 1   8 reads: (8 - 1) / 4 + 1 = two strided packs of 4 and POA #3 (level 3) -- at split=4 a cluster of 8 reads cannot be one
              pack, so the one-pack cluster is the one of 4;
  cluster 2  12 reads: three strided packs of 4 and POA #3 (level 3);
  cluster 3   2 reads: not above min_reads, no consensus.
The replay takes the plan from rattle_hip_plan_packs and the library's own corrected reads of each pack in the order POA #2 takes
them (stable by length, descending: correct.cpp:427, oracle/orc_correct.hpp), and runs oracle.poa_msa, oracle.post_msa(mode=2), the
numpy composition of the definition in include/rattle_hip.h, POA #3 in pack order, and the same again.  Precondition, asserted: the
replay's consensus bytes equal the library's (else the replay is wrong, not the support).  Then support and depth must be equal
exactly.  The seeds were chosen on the CPU (the same replay over the oracle's own corrected reads) so that the POA #3 of the 12-read
cluster has a base column where a row has a gap inside its window; asserted here."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
from rattle_amd import _lib, hps, synth
from rattle_amd.api import Clusters, correct_command, unpack_correction

pytestmark = pytest.mark.gpu

GAP = ord("-")
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
SPLIT, MIN_READS = 4, 2
SIZES = (4, 8, 12, 2)
SEED, TX_SEED = 7, 3


def job():
    """(headers, seqs, quals, clusters in hps list form): the members of cluster c are reads of transcript c"""
    seqs, quals, tid, _ = synth.reads(160, len(SIZES), 1, False, seed=SEED, tx_seed=TX_SEED, exon=(15, 25))
    clusters = []
    for c, n in enumerate(SIZES):
        ids = [i for i in range(len(seqs)) if tid[i] == c][:n]
        assert len(ids) == n, (c, len(ids))
        clusters.append(((ids[0], 0, -1), [(i, 0, -1) for i in ids]))
    return [b"@r%d" % i for i in range(len(seqs))], seqs, quals, clusters


def packed(seqs, quals, clusters):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    cat = np.frombuffer(b"".join(seqs), np.uint8).copy()
    qcat = np.frombuffer(b"".join(quals), np.uint8).copy()
    coff = np.zeros(len(clusters) + 1, np.uint32)
    coff[1:] = np.cumsum([len(m) for _, m in clusters])
    cl = Clusters(np.array([m[0] for m, _ in clusters], np.int32), np.zeros(len(clusters), np.uint8), coff,
                  np.array([s[0] for _, m in clusters for s in m], np.int32), np.array([s[1] for _, m in clusters for s in m], np.uint8),
                  np.zeros(8, np.uint64))
    return cat, qcat, off, cl


def plan_of(off, cl):
    """rattle_hip_plan_packs: (pack_first, member ids pack after pack, cluster of each pack)"""
    lib = _lib.load()
    P = _lib.CorrectParams(0.3, 0.3, 30.0, SPLIT, MIN_READS, 0, b"")
    out = C.POINTER(_lib.PackPlan)()
    u32, i32, u8, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    rc = lib.rattle_hip_plan_packs(off.ctypes.data_as(u64), len(off) - 1, len(cl.main_id), cl.offsets.ctypes.data_as(u32), cl.member_id.ctypes.data_as(i32),
                                   cl.member_rev.ctypes.data_as(u8), C.byref(P), 1, C.byref(out))
    assert rc == 0, lib.rattle_hip_last_error()
    p = out.contents
    n = p.n_packs
    first = np.ctypeslib.as_array(p.pack_first, (n + 1,)).copy()
    member = np.ctypeslib.as_array(p.member_id, (int(first[n]),)).copy()
    cluster = np.ctypeslib.as_array(p.pack_cluster, (n,)).copy()
    lib.rattle_hip_pack_plan_free(out)
    return first, member, cluster


def compose(rows, want, sup, dep):
    """include/rattle_hip.h, level 3, per column: of the rows whose window covers K, the support of those that hold the winner at K
    and the depth of all of them -- a row's base at K or, at a gap, its last base before K.  Also the number of cells that are a gap
    inside the row's window at a column whose winner is a base."""
    orig = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
    fixed = np.frombuffer(b"".join(want["rows"]), np.uint8).reshape(orig.shape)
    win = np.frombuffer(want["winner"], np.uint8)
    k = np.arange(orig.shape[1])
    cover = (k[None, :] >= want["rfirst"][:, None]) & (k[None, :] <= want["rlast"][:, None])
    idx = np.maximum(np.cumsum(orig != GAP, 1) - 1, 0)
    sup_c = np.stack([np.asarray(s, np.int64)[i] for s, i in zip(sup, idx)])
    dep_c = np.stack([np.asarray(d, np.int64)[i] for d, i in zip(dep, idx)])
    base = win != GAP
    support = (sup_c * (cover & (fixed == win[None, :]))).sum(0)[base]
    depth = (dep_c * cover).sum(0)[base]
    return support, depth, int((cover & (fixed == GAP) & base[None, :]).sum())


def replay(oracle, plan, corrected):
    """corrected: [(read id, sequence)] in the library's order.  Returns {cluster: dict(level, consensus, support, depth, pack_support,
    pack_depth, gaps_in_window, reads: corrected reads per pack)}"""
    first, member, cluster = plan
    pack_of = {int(r): p for p in range(len(cluster)) for r in member[first[p]:first[p + 1]]}
    per_pack = {p: [] for p in range(len(cluster))}
    for rid, s in corrected:
        per_pack[pack_of[rid]].append(s)
    out = {}
    for c in sorted(set(int(x) for x in cluster)):
        rows_in, sups, deps, n_reads = [], [], [], []
        for p in np.nonzero(cluster == c)[0]:
            seqs = sorted(per_pack[int(p)], key=lambda s: -len(s))                 # stable, length descending
            rows, _ = oracle.poa_msa(seqs)
            w = oracle.post_msa(rows, None, mode=2)
            base = np.frombuffer(w["winner"], np.uint8) != GAP
            rows_in.append(w["consensus"]); sups.append(w["occ"][base].astype(np.int64)); deps.append(w["total_occ"][base].astype(np.int64))
            n_reads.append(len(seqs))
        if len(rows_in) == 1:
            out[c] = dict(level=2, consensus=rows_in[0], support=sups[0], depth=deps[0], pack_support=sups[0], pack_depth=deps[0],
                          gaps_in_window=0, reads=n_reads)
            continue
        rows, _ = oracle.poa_msa(rows_in)
        w = oracle.post_msa(rows, None, mode=2)
        support, depth, gaps = compose(rows, w, sups, deps)
        base = np.frombuffer(w["winner"], np.uint8) != GAP
        out[c] = dict(level=3, consensus=w["consensus"], support=support, depth=depth, pack_support=w["occ"][base], pack_depth=w["total_occ"][base],
                      gaps_in_window=gaps, reads=n_reads)
    return out


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """the job with the switch off and on: (handle, unpacked) each"""
    headers, seqs, quals, clusters = job()
    cat, qcat, off, cl = packed(seqs, quals, clusters)
    res = {}
    try:
        for on in (False, True):
            gpu_ctx.set_consensus_support(on)
            h = gpu_ctx.correct_packed(cat, qcat, off, cl, split=SPLIT, min_reads=MIN_READS, keep=True)
            res[on] = (h, unpack_correction(h.ptr), h.digest(), h.support())
    finally:
        gpu_ctx.set_consensus_support(False)
    yield (headers, seqs, quals, clusters), (cat, qcat, off, cl), res
    for h, _, _, _ in res.values():
        h.free()


def test_nothing_else_changes_with_the_switch(runs):
    _, _, res = runs
    (_, off_u, off_d, off_s), (_, on_u, on_d, on_s) = res[False], res[True]
    assert off_d == on_d
    for key in ("corrected", "uncorrected", "consensi", "skipped"):
        assert off_u[key] == on_u[key], key
    assert np.array_equal(off_u["counters"], on_u["counters"])
    assert off_s is None and "support" not in off_u
    assert on_s is not None and set(on_u["support"]) == {"level", "off", "support", "depth", "pack_support", "pack_depth"}
    assert len(on_u["corrected"]) >= 20 and [r[1] for r in on_u["consensi"]] == [0, 1, 2]


def test_invariants(runs):
    _, (cat, qcat, off, cl), res = runs
    h, u, _, s = res[True]
    S = h.ptr.contents.consensi
    assert np.array_equal(s["off"], np.ctypeslib.as_array(S.off, (S.n + 1,)))
    assert len(s["level"]) == S.n == 3 and list(s["level"]) == [2, 3, 3]
    assert len(s["support"]) == len(s["depth"]) == len(s["pack_support"]) == len(s["pack_depth"]) == int(s["off"][-1]) > 300
    assert np.all(s["depth"] >= 1) and np.all(s["support"] <= s["depth"])
    assert np.all(s["pack_depth"] >= 1) and np.all(s["pack_support"] <= s["pack_depth"])
    n_corrected = {c: sum(1 for r in u["corrected"] if r[1] == c) for c in range(3)}
    for i, (_, cid, n_reads, seq, _) in enumerate(u["consensi"]):
        a, b = int(s["off"][i]), int(s["off"][i + 1])
        assert b - a == len(seq)
        if s["level"][i] == 2:
            assert np.all(s["depth"][a:b] <= n_corrected[cid])
            assert np.array_equal(s["pack_support"][a:b], s["support"][a:b]) and np.array_equal(s["pack_depth"][a:b], s["depth"][a:b])
        else:
            assert np.all(s["depth"][a:b] <= n_reads) and n_reads == SIZES[cid]
            assert np.all(s["pack_depth"][a:b] <= SIZES[cid] // 4)                # rows of POA #3: the cluster's packs


def test_replay_with_the_oracle(runs, oracle):
    _, (cat, qcat, off, cl), res = runs
    _, u, _, s = res[True]
    want = replay(oracle, plan_of(off, cl), [(r[0], r[3]) for r in u["corrected"]])
    assert sorted(want) == [0, 1, 2] and [want[c]["level"] for c in (0, 1, 2)] == [2, 3, 3]
    assert want[2]["gaps_in_window"] > 0, "the POA #3 of the 12-read cluster has no gap inside a window at a base column"
    for i, (_, cid, _, seq, _) in enumerate(u["consensi"]):
        w = want[cid]
        a, b = int(s["off"][i]), int(s["off"][i + 1])
        assert seq == w["consensus"], f"cluster {cid}: the replay's consensus is not the library's"      # the precondition
        assert s["level"][i] == w["level"]
        for f in ("support", "depth", "pack_support", "pack_depth"):
            assert np.array_equal(s[f][a:b], w[f]), (cid, f)
    # at level 3 the composition is not the vote's own count: reads, not packs
    a, b = int(s["off"][2]), int(s["off"][3])
    assert s["depth"][a:b].max() > s["pack_depth"][a:b].max() and s["depth"][a:b].max() <= 12


def test_the_big_cluster_flow_gives_the_same_support(runs, gpu_ctx, monkeypatch):
    """With the stage split forced (correct_driver.hip: the packs of a cluster of three packs or more go through POA #2 first, and its
    POA #3 shares a launch of kernel D with the POA #2 of all other packs), one launch holds composed packs and packs of reads."""
    _, (cat, qcat, off, cl), res = runs
    _, _, digest, s = res[True]
    monkeypatch.setenv("RATTLE_BIG_CLUSTER_PACKS", "3")
    monkeypatch.setenv("RATTLE_BIG_MIN_PACKS", "0")
    gpu_ctx.set_consensus_support(True)
    try:
        h = gpu_ctx.correct_packed(cat, qcat, off, cl, split=SPLIT, min_reads=MIN_READS, keep=True)
    finally:
        gpu_ctx.set_consensus_support(False)
    try:
        got = h.support()
        assert h.digest() == digest and set(got) == set(s)
        for f in s:
            assert np.array_equal(got[f], s[f]), f
    finally:
        h.free()


def test_correct_command_returns_the_table(runs, gpu_ctx):
    (headers, seqs, quals, clusters), _, res = runs
    _, u, _, s = res[True]
    plain = correct_command(gpu_ctx, headers, seqs, quals, clusters, split=SPLIT, min_reads=MIN_READS)
    out = correct_command(gpu_ctx, headers, seqs, quals, clusters, split=SPLIT, min_reads=MIN_READS, support=True)
    assert not gpu_ctx.consensus_support and len(out) == len(plain) + 1 and out[:3] == plain[:3]
    check_table(out[-1].decode(), out[2].decode(), s)


def check_table(tsv, consensi_fq, s):
    lines = tsv.split("\n")
    assert lines[0].split("\t") == ["consensus", "length", "level", "reads", "min_ratio", "weak", "support", "depth"] and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    heads = consensi_fq.split("\n")[0:-1:4]
    assert len(rows) == len(heads) == len(s["level"])
    for i, (r, h) in enumerate(zip(rows, heads)):
        a, b = int(s["off"][i]), int(s["off"][i + 1])
        sup, dep = s["support"][a:b], s["depth"][a:b]
        assert "@" + r[0] == h.split()[0] and "reads=" + r[3] in h.split()
        assert int(r[1]) == b - a and int(r[2]) == s["level"][i]
        assert [int(x) for x in r[6].split(",")] == list(sup) and [int(x) for x in r[7].split(",")] == list(dep)
        assert r[4] == "%.17g" % float(np.min(sup.astype(np.float64) / dep.astype(np.float64)))
        assert int(r[5]) == int(np.sum(2 * sup.astype(np.int64) <= dep))


def test_cli(runs, tmp_path):
    (headers, seqs, quals, clusters), _, res = runs
    _, u, _, s = res[True]
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"%s\n%s\n+\n%s\n" % (h, sq, q) for h, sq, q in zip(headers, seqs, quals)))
    (tmp_path / "clusters.out").write_bytes(hps.encode(clusters))
    # refused with several devices, before any device work (the input does not even exist)
    r = subprocess.run([RATTLE, "correct", "-i", str(tmp_path / "none.fq"), "-c", str(tmp_path / "none.out"), "--support", "--devices", "0,1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--support cannot be combined with --devices" in r.stderr and "Reading" not in r.stderr
    outs = {}
    for name, extra in (("plain", []), ("support", ["--support"])):
        outs[name] = tmp_path / name
        outs[name].mkdir()
        subprocess.run([RATTLE, "correct", "-i", str(fq), "-c", str(tmp_path / "clusters.out"), "-o", str(outs[name]), "-s", str(SPLIT), "-r", str(MIN_READS)] + extra,
                       check=True, capture_output=True, timeout=300)
    for f in ("corrected.fq", "uncorrected.fq", "consensi.fq"):
        assert (outs["plain"] / f).read_bytes() == (outs["support"] / f).read_bytes(), f
    assert sorted(os.listdir(outs["support"])) == sorted(os.listdir(outs["plain"]) + ["consensus_support.tsv"])
    cons = (outs["support"] / "consensi.fq").read_text()
    assert [l for l in cons.split("\n")[1:-1:4]] == [r[3].decode() for r in u["consensi"]]
    assert set("".join(cons.split("\n")[3:-1:4])) == {"K"}                        # consensi.fq keeps its qualities
    check_table((outs["support"] / "consensus_support.tsv").read_text(), cons, s)


WORKER = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, os.environ["RATTLE_ROOT"])
    sys.path.insert(0, os.path.join(os.environ["RATTLE_ROOT"], "tests"))
    import torch.distributed as dist
    from rattle_amd import _lib
    from rattle_amd.api import Context
    import test_gpu_consensus_support_e2e as m
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    _, seqs, quals, clusters = m.job()
    cat, qcat, off, cl = m.packed(seqs, quals, clusters)
    ctx = Context(0)
    ctx.comm_init_rccl()                           # the device-buffer transport over the tests' file-backed double
    ctx.set_consensus_support(True)
    calls0, _ = ctx.comm_stats()
    try:
        ctx.correct_packed(cat, qcat, off, cl, split=m.SPLIT, min_reads=m.MIN_READS)
        print("NOT_REFUSED", rank)
    except _lib.RattleError as e:
        assert "librattle_hip error %d:" % _lib.RATTLE_ERR_STATE in str(e) and "rattle_hip_set_consensus_support" in str(e), str(e)
        assert ctx.comm_stats()[0] == calls0, "something was exchanged before the refusal"
        print("REFUSED_OK", rank)
    ctx.set_consensus_support(False)
    res = ctx.correct_packed(cat, qcat, off, cl, split=m.SPLIT, min_reads=m.MIN_READS, gather_root=0, keep=True)
    assert res.support() is None                   # the gathered result carries none
    if rank == 0:
        print("GATHERED", res.counts()[2])
    res.free()
    ctx.close()
    dist.destroy_process_group()
''')


def test_a_sharded_job_is_refused_on_every_rank(tmp_path):
    """two ranks over the file-backed double of librccl.so (tests/stubs/fake_rccl.cpp, as tests/test_gpu_dist.py sets them up) with
    the switch on: both get RATTLE_ERR_STATE before anything is exchanged, none hangs; with it off again the same contexts run the
    job, and the gathered result carries no support"""
    so = tmp_path / "libfake_rccl.so"
    r = subprocess.run(["g++", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "stubs", "fake_rccl.cpp"),
                        "-o", str(so), "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    box = tmp_path / "mailbox"
    box.mkdir()
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, RATTLE_ROOT=ROOT, MASTER_ADDR="127.0.0.1", RATTLE_HOST_THREADS="8", RATTLE_RCCL_LIB=str(so), FAKE_RCCL_DIR=str(box))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29741", str(script)], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "REFUSED_OK 0" in r.stdout and "REFUSED_OK 1" in r.stdout and "NOT_REFUSED" not in r.stdout and "GATHERED 3" in r.stdout
