"""`align_cigars` at the edges that need no device: the two entry points exist under ABI 4 and are bound, the struct field lists are the
header's and those of align_pairs did not move, every argument error is refused before anything else and in align_pairs' order, a host
context and a context that is one rank of several are state errors (the latter with nothing exchanged), `_free(NULL)` is accepted,
`rattle assign -h` names `--cigar` and cg:Z:, `--cigar` without `--paf` fails and writes nothing, and the PAF writer appends the tag
of a hand-written ops set -- and writes what it wrote before without one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_ref
import cigar_ref
from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context

NAMES = ("rattle_hip_align_cigars", "rattle_hip_cigars_free")
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def call(lib, h, tcat=b"ACGTACGTAC" * 2, toff=(0, 10, 20), rcat=b"ACGTACGTUU" * 2, roff=(0, 10, 20), target=(0, 1), rev=(0, 1), null=()):
    """rattle_hip_align_cigars on two targets and two reads of 10 bases; `null`: the arguments handed over as NULL"""
    tcat, rcat = np.frombuffer(tcat, np.uint8).copy(), np.frombuffer(rcat, np.uint8).copy()
    toff, roff = np.array(toff, np.uint64), np.array(roff, np.uint64)
    target, rev = np.array(target, np.int32), np.array(rev, np.uint8)
    params = _lib.AlignParams(0, 0)
    res = C.POINTER(_lib.Alignment)()
    cg = C.POINTER(_lib.Cigars)()
    rc = lib.rattle_hip_align_cigars(
        h, None if "tcat" in null else ptr(tcat, C.c_uint8), None if "toff" in null else ptr(toff, C.c_uint64), len(toff) - 1,
        None if "rcat" in null else ptr(rcat, C.c_uint8), None if "roff" in null else ptr(roff, C.c_uint64), len(roff) - 1,
        None if "target" in null else ptr(target, C.c_int32), None if "rev" in null else ptr(rev, C.c_uint8),
        None if "params" in null else C.byref(params), None if "out" in null else C.byref(res), None if "cigars" in null else C.byref(cg))
    assert not res and not cg
    return rc, lib.rattle_hip_last_error()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in _lib.Cigars._fields_] == ["n", "offset", "ops"]
    assert _lib.SIGNATURES["rattle_hip_align_cigars"][1][:-1] == _lib.SIGNATURES["rattle_hip_align_pairs"][1]
    # nothing was added to the structs of align_pairs
    assert [f for f, _ in _lib.AlignParams._fields_] == ["max_cells", "pair_chunk"]
    assert [f for f, _ in _lib.Alignment._fields_] == ["n", "status", "score", "q_start", "q_end", "t_start", "t_end", "matches", "mismatches",
                                                       "q_gap", "t_gap"]
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in NAMES + ("rattle_cigars", "7 pair_cigar", "len << 4 | op"):
        assert name in header, name
    assert (api.K_ALIGN, api.K_CIGAR) == (6, 7)


def test_argument_errors_are_refused_before_the_context_is_looked_at(host_ctx):
    """on a host context: RATTLE_ERR_ARG (-2), not the RATTLE_ERR_STATE (-3) the same context gets for a clean call"""
    lib, h = host_ctx.lib, host_ctx.h
    assert call(lib, None)[0] == -2
    for name in ("tcat", "toff", "rcat", "roff", "target", "rev", "params", "out", "cigars"):
        assert call(lib, h, null=(name,))[0] == -2, name
    rc, msg = call(lib, h, target=(0, 2))
    assert rc == -2 and b"target" in msg and b"align_cigars" in msg       # an index >= n_targets
    rc, msg = call(lib, h, rev=(0, 2))
    assert rc == -2 and b"rev" in msg
    rc, msg = call(lib, h, target=(0, 2), rev=(0, 2), rcat=b"ACGTACGTAC" + b"NCGTACGTAC")
    assert rc == -2 and b"target" in msg                                  # align_pairs' order: the index, then the strand, then the letters
    rc, msg = call(lib, h, rev=(0, 2), rcat=b"ACGTACGTAC" + b"NCGTACGTAC")
    assert rc == -2 and b"rev" in msg
    for bad in (b"ACGTNCGTAC", b"ACGTaCGTAC", b"ACGT\0CGTAC", b"ACGT-CGTAC"):
        rc, msg = call(lib, h, rcat=b"ACGTACGTAC" + bad)
        assert rc == -2 and b"read 1" in msg, bad
        rc, msg = call(lib, h, tcat=bad + b"ACGTACGTAC")
        assert rc == -2 and b"target 0" in msg, bad
        # ... but not in a sequence that is not submitted: the call gets as far as the context
        assert call(lib, h, rcat=b"ACGTACGTAC" + bad, target=(0, -1))[0] == -3
        assert call(lib, h, tcat=bad + b"ACGTACGTAC", target=(1, 1))[0] == -3
    assert call(lib, h, target=(-1, -1), rev=(7, 7))[0] == -3             # (rev of a read that is not submitted is not read)
    lib.rattle_hip_cigars_free(None)                                      # like every *_free: NULL is accepted


def test_a_host_context_is_refused(host_ctx):
    rc, msg = call(host_ctx.lib, host_ctx.h)
    assert rc == -3 and b"no device" in msg
    with pytest.raises(_lib.RattleError):
        host_ctx.align_cigars([b"ACGT" * 5], [b"ACGT" * 5], [0], [0])
    with pytest.raises(ValueError):
        host_ctx.align_cigars([b"ACGT" * 5], [b"ACGT" * 5], [0, 0], [0])


def test_one_rank_of_several_is_refused_before_anything_is_exchanged():
    ctx = Context(None)
    calls = []

    def fn(user, send, send_bytes, recv, recv_bytes):
        calls.append(send_bytes)
        return 1

    thunk = _lib.ALLGATHERV_FN(fn)
    try:
        assert ctx.lib.rattle_hip_set_exchange(ctx.h, 1, 2, thunk, None) == 0
        rc, msg = call(ctx.lib, ctx.h)
        assert rc == -3 and b"one rank of several" in msg and b"align_cigars" in msg
        assert calls == []
    finally:
        ctx.close()


def test_the_cli_names_the_flag_and_refuses_it_without_paf(tmp_path):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    r = subprocess.run([RATTLE, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--cigar" in r.stderr and "cg:Z:" in r.stderr and "--paf" in r.stderr
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(fq), "-o", str(tmp_path), "--cigar"], capture_output=True, text=True)
    assert r.returncode != 0 and "--cigar needs --paf" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.fq"]


def test_the_cigar_string_and_the_paf_writer():
    """The reads of test_align_abi's writer test: a forward on t1 and c reverse on t0 have lines; the ops of b, d, e (none) are skipped."""
    assert api.cigar_bytes(np.array([12 << 4 | 7, 1 << 4 | 8, 3 << 4 | 1, 2 << 4 | 2, 300 << 4 | 7], np.uint32)) == b"12=1X3I2D300="
    assert api.cigar_bytes([]) == b"" and api.cigar_bytes(cigar_ref.encode([("=", 5), ("D", 70)])) == b"5=70D"
    asg = {"target": np.array([1, -1, 0, 0, 1], np.int32), "rev": np.array([0, 0, 1, 0, 0], np.uint8)}
    aln = {"status": [0, 3, 0, 1, 2], "score": [452, 0, 77, 0, 0], "q_start": [3, 0, 0, 0, 0], "q_end": [103, 0, 20, 0, 0],
           "t_start": [40, 0, 5, 0, 0], "t_end": [141, 0, 24, 0, 0], "matches": [96, 0, 18, 0, 0], "mismatches": [3, 0, 1, 0, 0],
           "q_gap": [1, 0, 1, 0, 0], "t_gap": [2, 0, 0, 0, 0]}
    aln = {f: np.array(aln[f], t) for f, t in align_ref.FIELDS}
    a_ops = [("=", 50), ("X", 3), ("I", 1), ("=", 20), ("D", 2), ("=", 26)]
    c_ops = [("=", 10), ("X", 1), ("I", 1), ("=", 8)]
    ops = np.concatenate([cigar_ref.encode(a_ops), cigar_ref.encode(c_ops)])
    offsets = np.array([0, 6, 6, 10, 10, 10], np.uint64)
    args = ([b"a", b"b", b"c", b"d", b"e"], [110, 50, 20, 30, 900], [b"t0", b"t1"], [60, 300], asg, aln)
    old = (b"a\t110\t3\t103\t+\tt1\t300\t40\t141\t96\t102\t255\tAS:i:452\tNM:i:6\tnx:i:3\tni:i:1\tnd:i:2\n"
           b"c\t20\t0\t20\t-\tt0\t60\t5\t24\t18\t20\t255\tAS:i:77\tNM:i:2\tnx:i:1\tni:i:1\tnd:i:0\n")
    assert api.paf_text(*args) == old and api.paf_text(*args, cigars=None) == old
    assert api.paf_text(*args, cigars=(offsets, ops)) == (
        b"a\t110\t3\t103\t+\tt1\t300\t40\t141\t96\t102\t255\tAS:i:452\tNM:i:6\tnx:i:3\tni:i:1\tnd:i:2\tcg:Z:50=3X1I20=2D26=\n"
        b"c\t20\t0\t20\t-\tt0\t60\t5\t24\t18\t20\t255\tAS:i:77\tNM:i:2\tnx:i:1\tni:i:1\tnd:i:0\tcg:Z:10=1X1I8=\n")
