"""`align_pileup` at the edges that need no device: the two symbols exist under ABI 4 and are bound; pileup == NULL and every refusal of
`align_cigars_mode` come back as RATTLE_ERR_ARG in that call's order, cigars == NULL being allowed; a context without a device is
RATTLE_ERR_STATE; `rattle_hip_pileup_free(NULL)` is harmless; kernel id 11 is a kernel id and 12 is not; Python's `align_pileup`
reaches the symbol with and without the CIGARs; and `rattle assign` refuses `--pileup` without `--paf`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context

NAMES = ("rattle_hip_align_pileup", "rattle_hip_pileup_free")
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
LOCAL, READ = 0, 1


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def call(lib, h, which="pileup", tcat=b"ACGTACGTAC" * 2, toff=(0, 10, 20), rcat=b"ACGTACGTUU" * 2, roff=(0, 10, 20), target=(0, 1), rev=(0, 1),
         scoring=(5, 4, 8, 6), mode=READ, null=()):
    """align_pileup (or, which == "cigars", align_cigars_mode) on two targets and two reads of 10 bases; scoring None and `null`:
    arguments handed over as NULL"""
    tcat, rcat = np.frombuffer(tcat, np.uint8).copy(), np.frombuffer(rcat, np.uint8).copy()
    toff, roff = np.array(toff, np.uint64), np.array(roff, np.uint64)
    target, rev = np.array(target, np.int32), np.array(rev, np.uint8)
    params, S = _lib.AlignParams(0, 0), _lib.AlignScoring(*(scoring or (0, 0, 0, 0)))
    res, cg, pu = C.POINTER(_lib.Alignment)(), C.POINTER(_lib.Cigars)(), C.POINTER(_lib.Pileup)()
    args = [h, None if "tcat" in null else ptr(tcat, C.c_uint8), None if "toff" in null else ptr(toff, C.c_uint64), len(toff) - 1,
            None if "rcat" in null else ptr(rcat, C.c_uint8), None if "roff" in null else ptr(roff, C.c_uint64), len(roff) - 1,
            None if "target" in null else ptr(target, C.c_int32), None if "rev" in null else ptr(rev, C.c_uint8),
            None if "params" in null else C.byref(params), None if scoring is None else C.byref(S), int(mode),
            None if "out" in null else C.byref(res), None if "cigars" in null else C.byref(cg)]
    if which == "pileup":
        rc = lib.rattle_hip_align_pileup(*args, None if "pileup" in null else C.byref(pu))
    else:
        rc = lib.rattle_hip_align_cigars_mode(*args)
    assert not res and not cg and not pu
    return rc, lib.rattle_hip_last_error()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in NAMES + ("rattle_pileup;", "uint32_t *a, *c, *g, *t, *del, *ins, *starts, *ends;", "NEITHER THE FIRST NOR THE LAST", "11 pair_pileup"):
        assert name in header, name
    # align_cigars_mode's arguments with one more result behind them
    a, b = _lib.SIGNATURES[NAMES[0]][1], _lib.SIGNATURES["rattle_hip_align_cigars_mode"][1]
    assert a[:-1] == b and a[-1]._type_._type_ is _lib.Pileup
    assert [f for f, _ in _lib.Pileup._fields_] == ["n"] + list(_lib.PILEUP_FIELDS)
    assert _lib.PILEUP_FIELDS == ("a", "c", "g", "t", "del", "ins", "starts", "ends")


def test_free_of_null_is_harmless():
    _lib.load().rattle_hip_pileup_free(None)


def test_the_refusals_are_those_of_align_cigars_mode_in_its_order(host_ctx):
    """RATTLE_ERR_ARG (-2) for each, with the message align_cigars_mode gives up to the call's name"""
    lib, h = host_ctx.lib, host_ctx.h
    assert call(lib, None)[0] == -2
    for name in ("tcat", "toff", "rcat", "roff", "target", "rev", "params", "out", "pileup"):
        rc, msg = call(lib, h, null=(name,))
        assert rc == -2 and msg == b"null argument", name
    # pileup == NULL is looked at first, as cigars == NULL is there: with a second fault the answer is still "null argument"
    assert call(lib, h, null=("pileup",), target=(0, 2)) == (-2, b"null argument")
    # cigars == NULL is no fault here: the call gets as far as the context
    rc, msg = call(lib, h, null=("cigars",))
    assert rc == -3 and b"no device" in msg
    faults = (dict(target=(0, 2), mode=7), dict(rev=(0, 2), mode=7), dict(rcat=b"ACGTACGTACACGTNCGTAC", mode=7),
              dict(tcat=b"ACGTACGTACACGTNCGTAC", mode=7), dict(scoring=(5, 4, 6, 8), mode=7), dict(scoring=(5, 4, 8, 6), mode=7),
              dict(scoring=None, mode=2), dict(target=(0, 2), rev=(0, 2)), dict(rev=(0, 2), rcat=b"ACGTACGTACACGTNCGTAC"),
              dict(rcat=b"ACGTACGTACACGTNCGTAC", scoring=(65, 4, 8, 6)))
    for kw in faults:
        rc, msg = call(lib, h, **kw)
        rc2, msg2 = call(lib, h, "cigars", **kw)
        assert rc == rc2 == -2, kw
        assert msg.split(b": ", 1)[1] == msg2.split(b": ", 1)[1] and msg.startswith(b"align_pileup: "), (kw, msg, msg2)
    n = 1 << 23                                                           # a left border that would reach 2^29 (tests/test_align_ends_abi.py)
    seq = np.full(n, ord("A"), np.uint8).tobytes() + b"ACGT"
    rc, msg = call(lib, h, tcat=b"ACGT", toff=(0, 4), rcat=seq, roff=(0, n, n + 4), target=(0, 0), rev=(0, 0), scoring=(1, 1, 64, 64))
    assert rc == -2 and b"read 0" in msg and b"2^29" in msg


def test_a_context_without_a_device_is_a_state_error(host_ctx):
    lib, h = host_ctx.lib, host_ctx.h
    for scoring in (None, (5, 4, 8, 6)):
        for mode in (LOCAL, READ):
            rc, msg = call(lib, h, scoring=scoring, mode=mode)
            assert rc == -3 and b"no device" in msg, (scoring, mode)
    assert call(lib, h, target=(-1, -1), rev=(7, 7))[0] == -3             # (nothing submitted: the call gets as far as the context)


def test_one_rank_of_several_is_refused():
    ctx = Context(None)
    thunk = _lib.ALLGATHERV_FN(lambda user, send, send_bytes, recv, recv_bytes: 1)
    try:
        assert ctx.lib.rattle_hip_set_exchange(ctx.h, 1, 2, thunk, None) == 0
        rc, msg = call(ctx.lib, ctx.h, mode=7)
        assert rc == -3 and b"one rank of several" in msg
    finally:
        ctx.close()


def test_kernel_id_11_is_a_kernel_id(host_ctx):
    assert host_ctx.kernel_stats(11)[1:] == (0, 0)
    with pytest.raises(_lib.RattleError, match="bad kernel id"):
        host_ctx.kernel_stats(12)


class Spy:
    """a library that records which align symbols are called, and whether the CIGARs were asked for"""

    def __init__(self, lib):
        self.lib, self.called = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("rattle_hip_align"):
            return fn

        def spy(*args):
            self.called.append((name, len(args), args[11], args[13] is not None))
            return fn(*args)
        return spy


def test_python_reaches_the_symbol_with_and_without_the_cigars(host_ctx):
    real, spy = host_ctx.lib, Spy(host_ctx.lib)
    host_ctx.lib = spy
    try:
        args = ([b"ACGT" * 5], [b"ACGT" * 5], [0], [0])
        for kw, mode, cg in (({}, LOCAL, False), ({"cigars": True}, LOCAL, True), ({"mode": "read", "scoring": (5, 4, 8, 6)}, READ, False),
                             ({"mode": "read", "cigars": True}, READ, True)):
            del spy.called[:]
            with pytest.raises(_lib.RattleError):                         # (a host context: the call is made and refused)
                host_ctx.align_pileup(*args, **kw)
            assert spy.called == [(NAMES[0], 15, mode, cg)], (kw, spy.called)
        with pytest.raises(ValueError):
            host_ctx.align_pileup(*args, mode="global")
    finally:
        host_ctx.lib = real


def test_pileup_tsv_has_a_line_per_covered_position():
    table = {f: np.zeros(7, np.uint32) for f in _lib.PILEUP_FIELDS}
    table["a"][1] = 2; table["del"][1] = 1; table["ins"][1] = 1; table["starts"][1] = 3
    table["t"][5] = 4; table["ends"][5] = 4
    table["ins"][6] = 9                                                   # (no depth: no line)
    text = api.pileup_tsv([b"x1", b"x2"], [b"CAG", b"GGUC"], table)
    assert text == (b"target\tpos\tref\tdepth\tA\tC\tG\tT\tdel\tins\tstarts\tends\n"
                    b"x1\t1\tA\t3\t2\t0\t0\t0\t1\t1\t3\t0\n"
                    b"x2\t2\tU\t4\t0\t0\t0\t4\t0\t0\t0\t4\n")


def test_the_cli_refuses_the_flag_without_paf(tmp_path):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    r = subprocess.run([RATTLE, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--pileup" in r.stderr and "pileup.tsv" in r.stderr
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    for flags in (("--pileup",), ("--pileup", "--secondary", "2"), ("--cigar", "--pileup")):
        r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(fq), "-o", str(tmp_path), *flags], capture_output=True, text=True)
        assert r.returncode != 0 and "needs --paf" in r.stderr, flags
    assert sorted(os.listdir(tmp_path)) == ["a.fq"]                       # every refusal comes before anything is written
