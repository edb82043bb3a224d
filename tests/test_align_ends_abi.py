"""`align_pairs_mode` and `align_cigars_mode` at the edges that need no device: the two entry points exist under ABI 4 and are bound, the
two modes are the header's; every refusal of the call the scoring selects comes first; then -- still before the device is looked at -- a
mode that is neither of the two and, in read mode, a read whose left border would reach 2^29; Python's `mode=` reaches the new symbols
and leaves "local" on the old ones; and `rattle assign` refuses `--paf-end-to-end` without `--paf`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context

NAMES = ("rattle_hip_align_pairs_mode", "rattle_hip_align_cigars_mode")
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
LOCAL, READ = 0, 1


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def call(lib, h, which, tcat=b"ACGTACGTAC" * 2, toff=(0, 10, 20), rcat=b"ACGTACGTUU" * 2, roff=(0, 10, 20), target=(0, 1), rev=(0, 1),
         scoring=(5, 4, 8, 6), mode=READ, null=()):
    """one of the two entry points on two targets and two reads of 10 bases; scoring None and `null`: arguments handed over as NULL"""
    tcat, rcat = np.frombuffer(tcat, np.uint8).copy(), np.frombuffer(rcat, np.uint8).copy()
    toff, roff = np.array(toff, np.uint64), np.array(roff, np.uint64)
    target, rev = np.array(target, np.int32), np.array(rev, np.uint8)
    params, S = _lib.AlignParams(0, 0), _lib.AlignScoring(*(scoring or (0, 0, 0, 0)))
    res, cg = C.POINTER(_lib.Alignment)(), C.POINTER(_lib.Cigars)()
    args = [h, None if "tcat" in null else ptr(tcat, C.c_uint8), None if "toff" in null else ptr(toff, C.c_uint64), len(toff) - 1,
            None if "rcat" in null else ptr(rcat, C.c_uint8), None if "roff" in null else ptr(roff, C.c_uint64), len(roff) - 1,
            None if "target" in null else ptr(target, C.c_int32), None if "rev" in null else ptr(rev, C.c_uint8),
            None if "params" in null else C.byref(params), None if scoring is None else C.byref(S), int(mode),
            None if "out" in null else C.byref(res)]
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
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in NAMES + ("#define RATTLE_ALIGN_LOCAL 0", "#define RATTLE_ALIGN_READ  1", "no zero floor", "H[i][0] = U[i][0] = -(o + (i-1) e)"):
        assert name in header, name
    assert api.ALIGN_MODES == {"local": LOCAL, "read": READ}
    # the scored calls' arguments with an int behind the scoring
    for new, old in zip(NAMES, ("rattle_hip_align_pairs_scored", "rattle_hip_align_cigars_scored")):
        a, b = _lib.SIGNATURES[new][1], _lib.SIGNATURES[old][1]
        assert a[:11] == b[:11] and a[11] is C.c_int and a[12:] == b[11:]


@pytest.mark.parametrize("which", ["pairs", "cigars"])
def test_the_refusals_of_the_four_calls_come_first(host_ctx, which):
    """RATTLE_ERR_ARG (-2) for each, also with a mode that would be refused itself"""
    lib, h = host_ctx.lib, host_ctx.h
    assert call(lib, None, which)[0] == -2
    for name in ("tcat", "toff", "rcat", "roff", "target", "rev", "params", "out") + (("cigars",) if which == "cigars" else ()):
        rc, msg = call(lib, h, which, null=(name,))
        assert rc == -2 and msg == b"null argument", name
    rc, msg = call(lib, h, which, target=(0, 2), mode=7)
    assert rc == -2 and b"target" in msg
    rc, msg = call(lib, h, which, rev=(0, 2), mode=7)
    assert rc == -2 and b"rev" in msg
    rc, msg = call(lib, h, which, rcat=b"ACGTACGTACACGTNCGTAC", mode=7)
    assert rc == -2 and b"read 1" in msg
    rc, msg = call(lib, h, which, scoring=(5, 4, 6, 8), mode=7)
    assert rc == -2 and b"gap_extend <= gap_open" in msg


@pytest.mark.parametrize("which", ["pairs", "cigars"])
def test_an_unknown_mode_is_refused_before_the_device_is_looked_at(host_ctx, which):
    """on a host context: RATTLE_ERR_ARG (-2), not the RATTLE_ERR_STATE (-3) the same context gets for the two modes"""
    lib, h = host_ctx.lib, host_ctx.h
    for scoring in (None, (5, 4, 8, 6)):
        for bad in (7, 2, -1):
            rc, msg = call(lib, h, which, scoring=scoring, mode=bad)
            assert rc == -2 and b"mode" in msg and b"RATTLE_ALIGN_READ" in msg, (scoring, bad)
        for ok in (LOCAL, READ):
            rc, msg = call(lib, h, which, scoring=scoring, mode=ok)
            assert rc == -3 and b"no device" in msg, (scoring, ok)
    assert call(lib, h, which, target=(-1, -1), rev=(7, 7))[0] == -3      # (nothing submitted: the call gets as far as the context)


@pytest.mark.parametrize("which", ["pairs", "cigars"])
def test_a_border_that_would_reach_2_29_is_refused(host_ctx, which):
    """gap_open + gap_extend * (Lq - 1) >= 2^29: with 64,64 a read of 2^23 bases, not one of 2^23 - 1, not in local mode and not when the
    long read is not submitted.  (The letters are checked first, so the read has to exist: 8 MiB of A, the smallest the order allows.)"""
    lib, h = host_ctx.lib, host_ctx.h
    n = 1 << 23
    seq = np.full(n, ord("A"), np.uint8).tobytes() + b"ACGT"
    kw = dict(tcat=b"ACGT", toff=(0, 4), rcat=seq, rev=(0, 0), scoring=(1, 1, 64, 64))
    rc, msg = call(lib, h, which, roff=(0, n, n + 4), target=(0, 0), **kw)
    assert rc == -2 and b"read 0" in msg and b"2^29" in msg
    assert call(lib, h, which, roff=(0, n - 1, n + 4), target=(0, 0), **kw)[0] == -3
    assert call(lib, h, which, roff=(0, n, n + 4), target=(0, 0), mode=LOCAL, **kw)[0] == -3
    assert call(lib, h, which, roff=(0, n, n + 4), target=(-1, 0), **kw)[0] == -3
    assert call(lib, h, which, roff=(0, n, n + 4), target=(0, 0), **{**kw, "scoring": (1, 1, 64, 63)})[0] == -3
    assert call(lib, h, which, roff=(0, 0, n + 4), target=(0, -1), **kw)[0] == -3              # an empty read has no border


def test_the_linear_form_has_the_bound_of_8_8(host_ctx):
    """scoring NULL is 5,4,8,8: a read of 2^26 bases"""
    lib, h = host_ctx.lib, host_ctx.h
    n = 1 << 26
    seq = np.full(n, ord("C"), np.uint8).tobytes()
    kw = dict(tcat=b"ACGT", toff=(0, 4), rcat=seq, rev=(0,), target=(0,), scoring=None)
    rc, msg = call(lib, h, "pairs", roff=(0, n), **kw)
    assert rc == -2 and b"read 0" in msg and b"2^29" in msg
    assert call(lib, h, "pairs", roff=(0, n - 1), **kw)[0] == -3


def test_one_rank_of_several_is_refused_before_the_mode_is_looked_at():
    ctx = Context(None)
    calls = []

    def fn(user, send, send_bytes, recv, recv_bytes):
        calls.append(send_bytes)
        return 1

    thunk = _lib.ALLGATHERV_FN(fn)
    try:
        assert ctx.lib.rattle_hip_set_exchange(ctx.h, 1, 2, thunk, None) == 0
        for which in ("pairs", "cigars"):
            rc, msg = call(ctx.lib, ctx.h, which, mode=7)
            assert rc == -3 and b"one rank of several" in msg
        assert calls == []
    finally:
        ctx.close()


class Spy:
    """a library that records which align symbols are called"""

    def __init__(self, lib):
        self.lib, self.called = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("rattle_hip_align"):
            return fn

        def spy(*args):
            self.called.append((name, len(args), args[11] if name.endswith("_mode") else None))
            return fn(*args)
        return spy


def test_mode_reaches_the_new_symbols_and_local_the_old(host_ctx):
    real, spy = host_ctx.lib, Spy(host_ctx.lib)
    host_ctx.lib = spy
    try:
        args = ([b"ACGT" * 5], [b"ACGT" * 5], [0], [0])
        for fn, kw, want in ((host_ctx.align_pairs, {"mode": "local"}, ("rattle_hip_align_pairs", 11, None)),
                             (host_ctx.align_cigars, {"mode": "local", "scoring": (5, 4, 8, 6)}, ("rattle_hip_align_cigars_scored", 13, None)),
                             (host_ctx.align_pairs, {"mode": "read"}, ("rattle_hip_align_pairs_mode", 13, READ)),
                             (host_ctx.align_pairs, {"mode": "read", "scoring": (5, 4, 8, 6)}, ("rattle_hip_align_pairs_mode", 13, READ)),
                             (host_ctx.align_cigars, {"mode": "read"}, ("rattle_hip_align_cigars_mode", 14, READ)),
                             (host_ctx.align_cigars, {"mode": 0, "scoring": (2, 4, 4, 2)}, ("rattle_hip_align_cigars_mode", 14, LOCAL))):
            del spy.called[:]
            with pytest.raises(_lib.RattleError):                         # (a host context: the call is made and refused)
                fn(*args, **kw)
            assert spy.called == [want], (kw, spy.called)
        with pytest.raises(ValueError):
            host_ctx.align_pairs(*args, mode="global")
        with pytest.raises(_lib.RattleError, match="mode 7"):
            host_ctx.align_pairs(*args, mode=7)
    finally:
        host_ctx.lib = real


def run_cli(tmp_path, *flags):
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    return subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(fq), "-o", str(tmp_path), *flags], capture_output=True, text=True)


def test_the_cli_refuses_the_flag_without_paf(tmp_path):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    r = subprocess.run([RATTLE, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--paf-end-to-end" in r.stderr and "semi-global" in r.stderr
    for flags in (("--paf-end-to-end",), ("--paf-end-to-end", "--secondary", "2"), ("--cigar", "--paf-end-to-end")):
        r = run_cli(tmp_path, *flags)
        assert r.returncode != 0 and "needs --paf" in r.stderr, flags
    r = run_cli(tmp_path, "--paf-end-to-end")
    assert "--paf-end-to-end needs --paf" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.fq"]                       # every refusal comes before anything is written
