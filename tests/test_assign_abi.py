"""`assign` at the edges that need no device: the three entry points exist under ABI 4 and are bound, argument errors are refused
before anything else, a host context and a context that is one rank of several are state errors (the latter before anything is
exchanged), `rattle assign` explains itself and insists on both files, the two TSV writers format a hand-written record set, and the
brute-force reduction the GPU tests compare with (tests/assign_ref.py) gives what a case worked out by hand says."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assign_ref
from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context

NAMES = ("rattle_hip_assign_loaded", "rattle_hip_assign_reads", "rattle_hip_assignment_free")
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def rattle():
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    return RATTLE


def params(**kw):
    P = _lib.AssignParams(0.2, 1000000.0, 0.4, 0, 0, 0, 0, 0)
    for f, v in kw.items():
        setattr(P, f, v)
    return P


def arrays():
    ids = np.arange(4, dtype=np.uint32)
    off = np.array([0, 20, 40], np.uint64)
    cat = np.frombuffer(b"ACGT" * 10, np.uint8).copy()
    return ids, off, cat


def u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in _lib.AssignParams._fields_] == ["t_s", "t_v", "bv_threshold", "use_hc", "is_rna", "target_batch", "read_chunk",
                                                          "count_pass"]
    assert [f for f, _ in _lib.Assignment._fields_] == ["n", "target", "rev", "bases", "hc_bases", "min_len", "score", "variance",
                                                        "second_score", "n_accepted"]
    assert [f for f, _ in _lib.ASSIGN_FIELDS] == [f for f, _ in assign_ref.FIELDS]
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in NAMES + ("rattle_assign_params", "rattle_assignment"):
        assert name in header, name


def test_argument_errors_are_refused(host_ctx):
    lib, h = host_ctx.lib, host_ctx.h
    ids, off, cat = arrays()
    P = params()
    out = C.POINTER(_lib.Assignment)()
    loaded = lib.rattle_hip_assign_loaded
    assert loaded(None, C.byref(P), u32(ids), 2, u32(ids), 2, C.byref(out)) == -2 and not out
    assert loaded(h, None, u32(ids), 2, u32(ids), 2, C.byref(out)) == -2
    assert loaded(h, C.byref(P), u32(ids), 2, u32(ids), 2, None) == -2
    assert loaded(h, C.byref(P), None, 2, u32(ids), 2, C.byref(out)) == -2
    assert loaded(h, C.byref(P), u32(ids), 2, None, 2, C.byref(out)) == -2 and not out
    for bad in (-1, 4):
        assert loaded(h, C.byref(params(count_pass=bad)), u32(ids), 2, u32(ids), 2, C.byref(out)) == -2
        assert b"count_pass" in lib.rattle_hip_last_error()
    reads = lib.rattle_hip_assign_reads
    assert reads(None, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), C.byref(out)) == -2
    assert reads(h, None, u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), C.byref(out)) == -2
    assert reads(h, u8(cat), None, 2, u8(cat), u64(off), 2, 10, C.byref(P), C.byref(out)) == -2
    assert reads(h, u8(cat), u64(off), 2, None, u64(off), 2, 10, C.byref(P), C.byref(out)) == -2
    assert reads(h, u8(cat), u64(off), 2, u8(cat), None, 2, 10, C.byref(P), C.byref(out)) == -2
    assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, None, C.byref(out)) == -2
    assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), None) == -2
    for k in (0, -3, 17):
        assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, k, C.byref(P), C.byref(out)) == -2 and not out
        assert b"kmer size" in lib.rattle_hip_last_error()
    assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(params(count_pass=9)), C.byref(out)) == -2
    lib.rattle_hip_assignment_free(None)                 # like every *_free: NULL is accepted


def test_a_host_context_is_refused_like_the_other_device_entry_points(host_ctx):
    lib, h = host_ctx.lib, host_ctx.h
    ids, off, cat = arrays()
    P = params()
    out = C.POINTER(_lib.Assignment)()
    assert lib.rattle_hip_assign_loaded(h, C.byref(P), u32(ids), 2, u32(ids), 2, C.byref(out)) == -3 and not out
    assert b"no device" in lib.rattle_hip_last_error()
    assert lib.rattle_hip_assign_reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), C.byref(out)) == -3 and not out
    assert b"no device" in lib.rattle_hip_last_error()
    cl = C.POINTER(_lib.ClusterSet)()
    CP = _lib.ClusterParams(0.2, 1e6, 0.4, 0.2, 0.05, 0, 0, 0.15, 0)
    assert lib.rattle_hip_cluster_reads(h, C.byref(CP), C.byref(cl)) == -3       # the error its other device entry points return
    with pytest.raises(_lib.RattleError):
        host_ctx.assign([b"ACGT" * 10], [b"ACGT" * 10])
    with pytest.raises(_lib.RattleError):
        host_ctx.assign_loaded([0], [1])


def test_one_rank_of_several_is_refused_before_anything_is_exchanged():
    ctx = Context(None)
    calls = []

    def fn(user, send, send_bytes, recv, recv_bytes):
        calls.append(send_bytes)
        return 1

    thunk = _lib.ALLGATHERV_FN(fn)
    try:
        assert ctx.lib.rattle_hip_set_exchange(ctx.h, 1, 2, thunk, None) == 0
        ids, off, cat = arrays()
        P = params()
        out = C.POINTER(_lib.Assignment)()
        assert ctx.lib.rattle_hip_assign_loaded(ctx.h, C.byref(P), u32(ids), 2, u32(ids), 2, C.byref(out)) == -3 and not out
        assert b"one rank of several" in ctx.lib.rattle_hip_last_error()
        assert ctx.lib.rattle_hip_assign_reads(ctx.h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), C.byref(out)) == -3
        assert b"one rank of several" in ctx.lib.rattle_hip_last_error()
        assert calls == []
    finally:
        ctx.close()


def test_the_cli_explains_itself_and_insists_on_both_files(rattle, tmp_path):
    r = subprocess.run([rattle, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "-x" in r.stderr and "assignments.tsv" in r.stderr and "target_counts.tsv" in r.stderr
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    r = subprocess.run([rattle, "assign", "-i", str(fq), "-o", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "-x" in r.stderr
    r = subprocess.run([rattle, "assign", "-x", str(fq), "-o", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "-i" in r.stderr
    r = subprocess.run([rattle, "assign", "-i", str(fq), "-x", str(fq), "--count-pass", "fast"], capture_output=True, text=True)
    assert r.returncode != 0 and "--count-pass" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.fq"]
    r = subprocess.run([rattle], capture_output=True, text=True)
    assert r.returncode != 0 and "assign" in r.stdout and "cluster" in r.stdout
    r = subprocess.run([rattle, "nonsense"], capture_output=True, text=True)
    assert r.returncode != 0 and "assign" in r.stdout


def test_the_tsv_writers():
    """Three reads on two targets: read a on t1 reverse with a runner-up, read b unassigned, read c on t0 forward and alone."""
    third = 1.0 / 3.0
    rec = {"target": np.array([1, -1, 0], np.int32), "rev": np.array([1, 0, 0], np.uint8), "bases": np.array([120, 0, 77], np.int32),
           "hc_bases": np.array([100, 0, 70], np.int32), "min_len": np.array([360, 0, 154], np.uint32),
           "score": np.array([third, -1.0, 0.5]), "variance": np.array([2.1, 0.0, 1e-300]),
           "second_score": np.array([0.25, -1.0, -1.0]), "n_accepted": np.array([3, 0, 1], np.uint32)}
    text = api.assignments_tsv([b"a", b"b", b"c"], [b"t0", b"t1"], rec)
    assert text == (b"read\ttarget\tstrand\tscore\tsecond_score\tn_accepted\tbases\thc_bases\tmin_len\tvariance\n"
                    b"a\tt1\t-\t0.33333333333333331\t0.25\t3\t120\t100\t360\t2.1000000000000001\n"
                    b"b\t*\t*\t-1\t-1\t0\t0\t0\t0\t0\n"
                    b"c\tt0\t+\t0.5\t-1\t1\t77\t70\t154\t1e-300\n")
    for line, r in zip(text.split(b"\n")[1:], range(3)):      # %.17g gives every double back
        f = line.split(b"\t")
        assert float(f[3]) == rec["score"][r] and float(f[4]) == rec["second_score"][r] and float(f[9]) == rec["variance"][r]
    counts = api.target_counts_tsv([b"t0", b"t1", b"t2"], [154, 400, 90], rec)
    assert counts == b"target\tlength\treads\tunique_reads\nt0\t154\t1\t1\nt1\t400\t1\t0\nt2\t90\t0\t0\n"
    assert api._first_token(b"@read7 runid=3 ch=1") == b"read7" and api._first_token(b">tx\tlen=3") == b"tx" and api._first_token(b"@") == b""
    un = api.unassigned_records(2)
    assert not assign_ref.same(un, assign_ref.unassigned(2))


def test_the_brute_force_reduction_on_a_case_worked_out_by_hand():
    """Three targets, four reads; the accepted comparisons (target, strand, score):
      read 0: (0,+,0.5) (1,+,0.75) (1,-,0.75) (2,+,0.6)  -> target 1 forward (the strands tie: forward first), second 0.6 -- the other
                                                             strand of target 1 does not count --, 4 accepted
      read 1: (2,-,0.4) (0,-,0.4)                          -> the targets tie: the lower index 0, reverse, second 0.4, 2 accepted
      read 2: none                                         -> unassigned
      read 3: (2,+,0.9) (2,-,0.3)                          -> target 2 forward, no other target: second -1, 2 accepted
    bases / hc_bases / min_len / variance travel with the winner.  The order of the list must not matter."""
    acc = [(0, 0, 0, 0.5, 50, 40, 100, 1.5), (0, 1, 0, 0.75, 75, 60, 100, 2.5), (0, 1, 1, 0.75, 75, 61, 100, 3.5), (0, 2, 0, 0.6, 60, 50, 100, 4.5),
           (1, 2, 1, 0.4, 44, 30, 110, 5.5), (1, 0, 1, 0.4, 40, 31, 100, 6.5),
           (3, 2, 0, 0.9, 90, 80, 100, 7.5), (3, 2, 1, 0.3, 30, 20, 100, 8.5)]
    want = {"target": [1, 0, -1, 2], "rev": [0, 1, 0, 0], "bases": [75, 40, 0, 90], "hc_bases": [60, 31, 0, 80], "min_len": [100, 100, 0, 100],
            "score": [0.75, 0.4, -1.0, 0.9], "variance": [2.5, 6.5, 0.0, 7.5], "second_score": [0.6, 0.4, -1.0, -1.0], "n_accepted": [4, 2, 0, 2]}
    want = {f: np.array(want[f], t) for f, t in assign_ref.FIELDS}
    rng = np.random.default_rng(3)
    for _ in range(6):
        got = assign_ref.reduce_best(4, [acc[i] for i in rng.permutation(len(acc))])
        assert not assign_ref.same(got, want), assign_ref.same(got, want)
    assert assign_ref.same(assign_ref.reduce_best(4, acc[:-1]), want)         # (the comparison itself sees a difference)
    assert not assign_ref.same(assign_ref.reduce_best(0, []), assign_ref.unassigned(0))
