"""`align_pairs_scored` and `align_cigars_scored` at the edges that need no device: the two entry points exist under ABI 4 and are bound,
the scoring struct is the header's, every refusal of align_pairs comes first and in its order, then -- still before the device is looked
at -- a NULL scoring, a magnitude outside 1..64, gap_extend > gap_open and a pair whose score might not fit; `scoring=None` reaches
the old symbols; and `rattle assign` refuses `--paf-scoring` without `--paf` and on anything but four integers within the limits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context

NAMES = ("rattle_hip_align_pairs_scored", "rattle_hip_align_cigars_scored")
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def call(lib, h, which, tcat=b"ACGTACGTAC" * 2, toff=(0, 10, 20), rcat=b"ACGTACGTUU" * 2, roff=(0, 10, 20), target=(0, 1), rev=(0, 1),
         scoring=(5, 4, 8, 6), null=()):
    """one of the two entry points on two targets and two reads of 10 bases; `null`: the arguments handed over as NULL"""
    tcat, rcat = np.frombuffer(tcat, np.uint8).copy(), np.frombuffer(rcat, np.uint8).copy()
    toff, roff = np.array(toff, np.uint64), np.array(roff, np.uint64)
    target, rev = np.array(target, np.int32), np.array(rev, np.uint8)
    params, S = _lib.AlignParams(0, 0), _lib.AlignScoring(*scoring)
    res, cg = C.POINTER(_lib.Alignment)(), C.POINTER(_lib.Cigars)()
    args = [h, None if "tcat" in null else ptr(tcat, C.c_uint8), None if "toff" in null else ptr(toff, C.c_uint64), len(toff) - 1,
            None if "rcat" in null else ptr(rcat, C.c_uint8), None if "roff" in null else ptr(roff, C.c_uint64), len(roff) - 1,
            None if "target" in null else ptr(target, C.c_int32), None if "rev" in null else ptr(rev, C.c_uint8),
            None if "params" in null else C.byref(params), None if "scoring" in null else C.byref(S), None if "out" in null else C.byref(res)]
    if which == "cigars":
        args.append(None if "cigars" in null else C.byref(cg))
    rc = getattr(lib, NAMES[which == "cigars"])(*args)
    assert not res and not cg
    return rc, lib.rattle_hip_last_error()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [(f, t) for f, t in _lib.AlignScoring._fields_] == [(f, C.c_uint32) for f in ("match", "mismatch", "gap_open", "gap_extend")]
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in NAMES + ("rattle_align_scoring", "uint32_t match, mismatch, gap_open, gap_extend", "OPEN WINS A TIE"):
        assert name in header, name
    assert (api.K_ALIGN, api.K_CIGAR, api.K_ALIGN_AFFINE, api.K_CIGAR_AFFINE) == (6, 7, 8, 9)
    # the scored calls return the structs of the old ones
    assert _lib.SIGNATURES[NAMES[0]][1][-1] is _lib.SIGNATURES["rattle_hip_align_pairs"][1][-1]
    assert _lib.SIGNATURES[NAMES[1]][1][-2:] == _lib.SIGNATURES["rattle_hip_align_cigars"][1][-2:]


@pytest.mark.parametrize("which", ["pairs", "cigars"])
def test_the_refusals_of_align_pairs_come_first(host_ctx, which):
    """RATTLE_ERR_ARG (-2) for each, also with a scoring that would be refused itself"""
    lib, h = host_ctx.lib, host_ctx.h
    assert call(lib, None, which)[0] == -2
    for name in ("tcat", "toff", "rcat", "roff", "target", "rev", "params", "out") + (("cigars",) if which == "cigars" else ()):
        rc, msg = call(lib, h, which, null=(name,))
        assert rc == -2 and msg == b"null argument", name
    bad_scoring = (0, 4, 8, 6)
    rc, msg = call(lib, h, which, target=(0, 2), scoring=bad_scoring)
    assert rc == -2 and b"target" in msg                                  # an index >= n_targets
    rc, msg = call(lib, h, which, rev=(0, 2), scoring=bad_scoring)
    assert rc == -2 and b"rev" in msg
    for bad in (b"ACGTNCGTAC", b"ACGT\0CGTAC"):
        rc, msg = call(lib, h, which, rcat=b"ACGTACGTAC" + bad, scoring=bad_scoring)
        assert rc == -2 and b"read 1" in msg, bad
        rc, msg = call(lib, h, which, tcat=bad + b"ACGTACGTAC", null=("scoring",))
        assert rc == -2 and b"target 0" in msg, bad


@pytest.mark.parametrize("which", ["pairs", "cigars"])
def test_the_scoring_is_refused_before_the_device_is_looked_at(host_ctx, which):
    """on a host context: RATTLE_ERR_ARG (-2), not the RATTLE_ERR_STATE (-3) the same context gets for a scoring within the limits"""
    lib, h = host_ctx.lib, host_ctx.h
    rc, msg = call(lib, h, which, null=("scoring",))
    assert rc == -2 and b"null scoring" in msg
    for bad in ((0, 4, 8, 6), (65, 4, 8, 6), (5, 0, 8, 6), (5, 65, 8, 6), (5, 4, 0, 0), (5, 4, 65, 6), (5, 4, 8, 0), (5, 4, 6, 8), (5, 4, 64, 65),
                (2 ** 32 - 1, 4, 8, 6)):
        rc, msg = call(lib, h, which, scoring=bad)
        assert rc == -2 and b"[1, 64]" in msg and b"gap_extend <= gap_open" in msg, bad
    for ok in ((5, 4, 8, 6), (5, 4, 8, 8), (1, 1, 1, 1), (64, 64, 64, 64), (64, 1, 64, 1), (2, 4, 4, 2)):
        rc, msg = call(lib, h, which, scoring=ok)
        assert rc == -3 and b"no device" in msg, ok
    assert call(lib, h, which, target=(-1, -1), rev=(7, 7))[0] == -3      # (nothing submitted: the call gets as far as the context)


@pytest.mark.parametrize("which", ["pairs", "cigars"])
def test_a_score_that_might_not_fit_is_refused(host_ctx, which):
    """match * min(Lq, Lt) > 2^31 - 1: with match 64 a pair of two sequences of 2^25 bases (2^31), not one of 2^25 - 1 on 2^25, and
    not when the long read is not submitted"""
    lib, h = host_ctx.lib, host_ctx.h
    n = 1 << 25
    seq = np.full(n, ord("A"), np.uint8).tobytes()
    kw = dict(tcat=seq, toff=(0, n), rev=(0, 0), scoring=(64, 4, 8, 6))
    rc, msg = call(lib, h, which, rcat=seq + b"ACGT", roff=(0, n, n + 4), target=(0, 0), **kw)
    assert rc == -2 and b"read 0" in msg and b"2^31 - 1" in msg
    assert call(lib, h, which, rcat=seq + b"ACGT", roff=(0, n - 1, n + 4), target=(0, 0), **kw)[0] == -3
    assert call(lib, h, which, rcat=seq + b"ACGT", roff=(0, n, n + 4), target=(-1, 0), **kw)[0] == -3
    assert call(lib, h, which, rcat=seq + b"ACGT", roff=(0, n, n + 4), target=(0, 0), **{**kw, "scoring": (63, 4, 8, 6)})[0] == -3


def test_one_rank_of_several_is_refused_before_anything_is_exchanged():
    ctx = Context(None)
    calls = []

    def fn(user, send, send_bytes, recv, recv_bytes):
        calls.append(send_bytes)
        return 1

    thunk = _lib.ALLGATHERV_FN(fn)
    try:
        assert ctx.lib.rattle_hip_set_exchange(ctx.h, 1, 2, thunk, None) == 0
        for which in ("pairs", "cigars"):
            rc, msg = call(ctx.lib, ctx.h, which, scoring=(0, 0, 0, 0))  # (an error of align_pairs: before the scoring's)
            assert rc == -3 and b"one rank of several" in msg
        assert calls == []
    finally:
        ctx.close()


class Spy:
    """a library that records which symbols are called, and refuses every call"""

    def __init__(self, lib):
        self.lib, self.called = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("rattle_hip_align"):
            return fn

        def spy(*args):
            self.called.append((name, len(args)))
            return fn(*args)
        return spy


def test_scoring_none_reaches_the_old_symbols(host_ctx):
    real, spy = host_ctx.lib, Spy(host_ctx.lib)
    host_ctx.lib = spy
    try:
        args = ([b"ACGT" * 5], [b"ACGT" * 5], [0], [0])
        for fn, kw, name, n in ((host_ctx.align_pairs, {}, "rattle_hip_align_pairs", 11),
                                (host_ctx.align_pairs, {"scoring": None}, "rattle_hip_align_pairs", 11),
                                (host_ctx.align_cigars, {}, "rattle_hip_align_cigars", 12),
                                (host_ctx.align_pairs, {"scoring": (5, 4, 8, 8)}, "rattle_hip_align_pairs_scored", 12),
                                (host_ctx.align_cigars, {"scoring": (5, 4, 8, 6)}, "rattle_hip_align_cigars_scored", 13)):
            del spy.called[:]
            with pytest.raises(_lib.RattleError):                         # (a host context: the call is made and refused)
                fn(*args, **kw)
            assert spy.called == [(name, n)], (name, spy.called)
        with pytest.raises(ValueError):
            host_ctx.align_pairs(*args, scoring=(5, 4, 8))
        with pytest.raises(_lib.RattleError, match="gap_extend <= gap_open"):
            host_ctx.align_cigars(*args, scoring=(5, 4, 6, 8))
    finally:
        host_ctx.lib = real


def run_cli(tmp_path, *flags):
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    return subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(fq), "-o", str(tmp_path), *flags], capture_output=True, text=True)


def test_the_cli_refuses_the_flag_without_paf_and_malformed_values(tmp_path):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    r = subprocess.run([RATTLE, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--paf-scoring m,x,o,e" in r.stderr and "Default: linear gaps, 5,4,8,8" in r.stderr and "1..64" in r.stderr
    r = run_cli(tmp_path, "--paf-scoring", "5,4,8,6")
    assert r.returncode != 0 and "--paf-scoring needs --paf" in r.stderr
    r = run_cli(tmp_path, "--cigar", "--paf-scoring", "5,4,8,6")
    assert r.returncode != 0 and "needs --paf" in r.stderr
    for bad in ("5,4,8", "5,4,8,6,1", "5,4,8,", ",4,8,6", "5,4,8,x", "5,4,8,6.0", "5, 4,8,6", "0,4,8,6", "65,4,8,6", "5,0,8,6", "5,65,8,6",
                "5,4,65,6", "5,4,8,0", "5,4,6,8", "5;4;8;6", "5,4,8,+6", "5,4,8,100", "99999999999,4,8,6", "affine"):
        r = run_cli(tmp_path, "--paf", "--paf-scoring", bad)
        assert r.returncode != 0 and "--paf-scoring takes four integers" in r.stderr and "1..64" in r.stderr and "e <= o" in r.stderr, bad
    assert sorted(os.listdir(tmp_path)) == ["a.fq"]                       # every refusal comes before anything is written
