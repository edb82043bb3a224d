"""The candidate list of `assign` at the edges that need no device: the three entry points exist under ABI 4 and are bound, their own
argument errors (k == 0, k > 8, cands == NULL) are refused before a device is needed and behind the errors the plain calls have, a host
context and a context that is one rank of several are state errors, `rattle assign` knows --secondary and refuses what it cannot take,
and the two writers format a hand-written candidate list."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assign_top_ref
from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context
from test_assign_abi import arrays, params, u8, u32, u64

NAMES = ("rattle_hip_assign_loaded_top", "rattle_hip_assign_reads_top", "rattle_hip_candidates_free")
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


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in _lib.Candidates._fields_] == ["n", "k", "count", "target", "rev", "bases", "hc_bases", "min_len", "score", "variance"]
    assert [f for f, _ in _lib.CANDIDATE_FIELDS] == [f for f, _ in assign_top_ref.FIELDS]
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in NAMES + ("rattle_candidates",):
        assert name in header, name


def test_argument_errors_are_refused_in_order(host_ctx):
    lib, h = host_ctx.lib, host_ctx.h
    ids, off, cat = arrays()
    P = params()
    out = C.POINTER(_lib.Assignment)()
    cands = C.POINTER(_lib.Candidates)()
    loaded = lib.rattle_hip_assign_loaded_top
    reads = lib.rattle_hip_assign_reads_top
    # the new errors, on a host context: RATTLE_ERR_ARG, not the state error a call with good arguments gets there
    for k in (0, 9, 0xFFFFFFFF):
        assert loaded(h, C.byref(P), u32(ids), 2, u32(ids), 2, k, C.byref(out), C.byref(cands)) == -2 and not out and not cands
        assert b"[1,8]" in lib.rattle_hip_last_error()
        assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), k, C.byref(out), C.byref(cands)) == -2 and not out
        assert b"[1,8]" in lib.rattle_hip_last_error()
    assert loaded(h, C.byref(P), u32(ids), 2, u32(ids), 2, 2, C.byref(out), None) == -2 and not out
    assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), 2, C.byref(out), None) == -2 and not out
    for k in (1, 8):
        assert loaded(h, C.byref(P), u32(ids), 2, u32(ids), 2, k, C.byref(out), C.byref(cands)) == -3
        assert b"no device" in lib.rattle_hip_last_error()
        assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), k, C.byref(out), C.byref(cands)) == -3
    # the earlier errors as in the plain calls
    assert loaded(None, C.byref(P), u32(ids), 2, u32(ids), 2, 2, C.byref(out), C.byref(cands)) == -2
    assert loaded(h, None, u32(ids), 2, u32(ids), 2, 2, C.byref(out), C.byref(cands)) == -2
    assert loaded(h, C.byref(P), u32(ids), 2, u32(ids), 2, 2, None, C.byref(cands)) == -2 and not cands
    assert loaded(h, C.byref(P), None, 2, u32(ids), 2, 2, C.byref(out), C.byref(cands)) == -2
    assert loaded(h, C.byref(P), u32(ids), 2, None, 2, 2, C.byref(out), C.byref(cands)) == -2
    assert reads(h, None, u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), 2, C.byref(out), C.byref(cands)) == -2
    assert reads(h, u8(cat), u64(off), 2, u8(cat), None, 2, 10, C.byref(P), 2, C.byref(out), C.byref(cands)) == -2
    # ... and they come first: a bad count_pass or k-mer size beside a bad k is reported, not the k
    assert loaded(h, C.byref(params(count_pass=4)), u32(ids), 2, u32(ids), 2, 0, C.byref(out), C.byref(cands)) == -2
    assert b"count_pass" in lib.rattle_hip_last_error()
    assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 17, C.byref(P), 9, C.byref(out), C.byref(cands)) == -2
    assert b"kmer size" in lib.rattle_hip_last_error()
    assert reads(h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(params(count_pass=-1)), 9, C.byref(out), None) == -2
    assert b"count_pass" in lib.rattle_hip_last_error()
    lib.rattle_hip_candidates_free(None)                 # like every *_free: NULL is accepted
    for call in (lambda: host_ctx.assign_top([b"ACGT" * 10], [b"ACGT" * 10], 2), lambda: host_ctx.assign_loaded_top([0], [1], 2),
                 lambda: host_ctx.assign_loaded_top([0], [1], 0)):
        with pytest.raises(_lib.RattleError):
            call()


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
        cands = C.POINTER(_lib.Candidates)()
        assert ctx.lib.rattle_hip_assign_loaded_top(ctx.h, C.byref(P), u32(ids), 2, u32(ids), 2, 3, C.byref(out), C.byref(cands)) == -3
        assert b"one rank of several" in ctx.lib.rattle_hip_last_error() and not out and not cands
        assert ctx.lib.rattle_hip_assign_reads_top(ctx.h, u8(cat), u64(off), 2, u8(cat), u64(off), 2, 10, C.byref(P), 3, C.byref(out),
                                                   C.byref(cands)) == -3
        assert b"one rank of several" in ctx.lib.rattle_hip_last_error()
        assert ctx.lib.rattle_hip_assign_loaded_top(ctx.h, C.byref(P), u32(ids), 2, u32(ids), 2, 9, C.byref(out), C.byref(cands)) == -2
        assert calls == []
    finally:
        ctx.close()


def test_the_cli_knows_the_flag_and_refuses_what_it_cannot_take(rattle, tmp_path):
    r = subprocess.run([rattle, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--secondary" in r.stderr and "candidates.tsv" in r.stderr
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    for bad in (["--secondary", "0"], ["--secondary", "8"], ["--secondary", "x"], ["--secondary", "-1"], ["--secondary", "2", "--devices", "0,1"]):
        r = subprocess.run([rattle, "assign", "-i", str(fq), "-x", str(fq), "-o", str(tmp_path)] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and ("--secondary" in r.stderr or "--devices" in r.stderr), bad
    assert sorted(os.listdir(tmp_path)) == ["a.fq"]


def test_the_writers():
    """Three reads on three targets, K = 3: read a has three candidates, read b none, read c one."""
    third = 1.0 / 3.0
    c = assign_top_ref.unused(3, 3)
    c["count"][:] = [3, 0, 1]
    c["target"][0] = [1, 0, 2]; c["rev"][0] = [1, 0, 0]; c["score"][0] = [0.5, third, 0.25]; c["bases"][0] = [120, 80, 60]
    c["hc_bases"][0] = [100, 70, 50]; c["min_len"][0] = [240, 240, 240]; c["variance"][0] = [2.1, 0.0, 1e-300]
    c["target"][2, 0] = 2; c["score"][2, 0] = 0.75; c["bases"][2, 0] = 75; c["hc_bases"][2, 0] = 70; c["min_len"][2, 0] = 100; c["variance"][2, 0] = 3.0
    text = api.candidates_tsv([b"a", b"b", b"c"], [b"t0", b"t1", b"t2"], c)
    assert text == (b"read\trank\ttarget\tstrand\tscore\tbases\thc_bases\tmin_len\tvariance\n"
                    b"a\t0\tt1\t-\t0.5\t120\t100\t240\t2.1000000000000001\n"
                    b"a\t1\tt0\t+\t0.33333333333333331\t80\t70\t240\t0\n"
                    b"a\t2\tt2\t+\t0.25\t60\t50\t240\t1e-300\n"
                    b"c\t0\tt2\t+\t0.75\t75\t70\t100\t3\n")
    un = api.unused_candidates(2, 4)
    assert not assign_top_ref.same(un, assign_top_ref.unused(2, 4))
    # the ranked PAF: rank 0 and rank 1 aligned; read a's rank 1 has status 2 (over the cell cap), read c has no rank 1
    def aln(status, score):
        a = {f: np.zeros(3, np.dtype(t)) for f, t in _lib.ALIGN_FIELDS}
        a["status"][:] = status; a["score"][:] = score
        a["q_end"][:] = 10; a["t_start"][:] = 5; a["t_end"][:] = 16; a["matches"][:] = 9; a["mismatches"][:] = 1; a["t_gap"][:] = 1
        return a
    alns = [aln([0, 3, 0], [41, 0, 41]), aln([2, 3, 3], [0, 0, 0])]
    names, tn = [b"a", b"b", b"c"], [b"t0", b"t1", b"t2"]
    paf = api.paf_ranked_text(names, [10, 10, 10], tn, [30, 31, 32], c, alns)
    assert paf == (b"a\t10\t0\t10\t-\tt1\t31\t5\t16\t9\t11\t255\tAS:i:41\tNM:i:2\tnx:i:1\tni:i:0\tnd:i:1\ttp:A:P\trk:i:0\n"
                   b"c\t10\t0\t10\t+\tt2\t32\t5\t16\t9\t11\t255\tAS:i:41\tNM:i:2\tnx:i:1\tni:i:0\tnd:i:1\ttp:A:P\trk:i:0\n")
    alns[1] = aln([0, 3, 3], [30, 0, 0])
    cg = [(np.array([0, 1, 1, 2], np.uint64), np.array([(10 << 4) | 7, (10 << 4) | 7], np.uint32)),
          (np.array([0, 2, 2, 2], np.uint64), np.array([(4 << 4) | 7, (1 << 4) | 2], np.uint32))]
    paf = api.paf_ranked_text(names, [10, 10, 10], tn, [30, 31, 32], c, alns, cg).split(b"\n")
    assert paf[0].endswith(b"\tnd:i:1\ttp:A:P\trk:i:0\tcg:Z:10=") and paf[2].endswith(b"\ttp:A:P\trk:i:0\tcg:Z:10=") and paf[3] == b""
    assert paf[1] == b"a\t10\t0\t10\t+\tt0\t30\t5\t16\t9\t11\t255\tAS:i:30\tNM:i:2\tnx:i:1\tni:i:0\tnd:i:1\ttp:A:S\trk:i:1\tcg:Z:4=1D"
    # the P lines without the two tags are paf_text's lines for the record that is slot 0
    rec = api.unassigned_records(3)
    rec["target"][:] = c["target"][:, 0]; rec["rev"][:] = c["rev"][:, 0]
    plain = api.paf_text(names, [10, 10, 10], tn, [30, 31, 32], rec, alns[0], cg[0])
    assert b"".join(l.replace(b"\ttp:A:P\trk:i:0", b"") + b"\n" for l in paf if b"tp:A:P" in l) == plain
