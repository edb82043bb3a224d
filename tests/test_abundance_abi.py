"""`abundance` at the edges that need no device: the entry points exist under ABI 4 and are bound, the argument errors come in the order
the header promises and before the context is looked at, a context that is one rank of several is refused, `rattle assign` knows the
flags and refuses the bad combinations before it writes anything, and api.abundance_tsv formats a hand-made record."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rattle_amd import _lib, api
from rattle_amd.api import Context

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


class Call:
    """one call of rattle_hip_abundance on a two-read, k = 2 list; every keyword breaks one thing"""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def __call__(self, k=2, count=(2, 1), target=(0, 1, 1, -1), nt=2, ratio=0.95, tol=1e-3, max_iters=1000, params=True, cands=True, out=True,
                 ctx=True, arrays=True):
        self.keep = (np.array(count, np.uint32), np.array(target, np.int32), np.array([0.9, 0.9, 0.8, -1.0]))
        Cd = _lib.Candidates()
        Cd.n, Cd.k = 2, k
        if arrays:
            Cd.count = self.keep[0].ctypes.data_as(C.POINTER(C.c_uint32))
            Cd.target = self.keep[1].ctypes.data_as(C.POINTER(C.c_int32))
            Cd.score = self.keep[2].ctypes.data_as(C.POINTER(C.c_double))
        P = _lib.AbundanceParams(ratio, tol, max_iters, 0)
        res = C.POINTER(_lib.Abundance)()
        rc = self.lib.rattle_hip_abundance(self.h if ctx else None, C.byref(Cd) if cands else None, nt, C.byref(P) if params else None,
                                           C.byref(res) if out else None)
        assert not res
        return rc, self.lib.rattle_hip_last_error()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in ("rattle_hip_abundance", "rattle_hip_abundance_free"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in _lib.AbundanceParams._fields_] == ["ratio", "tol", "max_iters", "iter_block"]
    assert [f for f, _ in _lib.Abundance._fields_] == ["n_targets", "n_reads", "k", "iterations", "converged", "n_placed", "units", "est_reads",
                                                       "cpm", "compatible_reads", "delta", "posterior"]
    header = open(os.path.join(ROOT, "include", "rattle_hip.h")).read()
    for name in ("rattle_hip_abundance", "rattle_hip_abundance_free", "rattle_abundance_params", "rattle_abundance"):
        assert name in header, name
    lib.rattle_hip_abundance_free(None)                  # like every *_free: NULL is accepted


def test_the_argument_errors_come_in_the_stated_order(host_ctx):
    call = Call(host_ctx.lib, host_ctx.h)
    # everything right: only the host context is in the way, and it is looked at last
    rc, msg = call()
    assert rc == -3 and b"no device" in msg
    rc, msg = call(params=False)                         # NULL params: the defaults
    assert rc == -3 and b"no device" in msg
    bad = {"null": dict(cands=False), "k": dict(k=9, count=(9, 9)), "count": dict(count=(3, 1)), "target": dict(target=(0, 2, 1, -1)),
           "ratio": dict(ratio=0.0), "tol": dict(tol=-1.0), "iters": dict(max_iters=0)}
    word = {"null": b"null", "k": b"[1,8]", "count": b"exceeds k", "target": b"names target", "ratio": b"ratio", "tol": b"tol", "iters": b"max_iters"}
    order = list(bad)
    for i, first in enumerate(order):
        rc, msg = call(**bad[first])
        assert rc == -2 and word[first] in msg, (first, msg)
        for later in order[i + 1:]:                     # two mistakes at once: the earlier one of the list is the one reported
            if first == "null":
                continue
            kw = dict(bad[later])
            kw.update(bad[first])
            rc, msg = call(**kw)
            assert rc == -2 and word[first] in msg, (first, later, msg)
    for kw in (dict(ctx=False), dict(out=False), dict(arrays=False)):
        rc, msg = call(ratio=2.0, **kw)
        assert rc == -2 and b"null" in msg
    for kw in (dict(k=0, count=(0, 0)), dict(target=(0, -1, 1, -1)), dict(ratio=1.5), dict(ratio=-0.5), dict(ratio=float("nan")),
               dict(tol=float("nan")), dict(tol=float(2 ** 20)), dict(nt=0)):
        assert call(**kw)[0] == -2, kw
    for kw in (dict(ratio=1.0), dict(tol=0.0), dict(tol=float(2 ** 20 - 1)), dict(max_iters=1), dict(count=(0, 0), nt=0)):
        assert call(**kw)[0] == -3, kw                   # the limits themselves are inside
    with pytest.raises(_lib.RattleError):
        host_ctx.abundance({"count": [1], "target": [[0]], "score": [[0.5]]}, 1)
    with pytest.raises(ValueError):
        host_ctx.abundance({"count": [1, 1], "target": [[0]], "score": [[0.5]]}, 1)


def test_one_rank_of_several_is_refused_behind_the_arguments():
    ctx = Context(None)
    calls = []

    def fn(user, send, send_bytes, recv, recv_bytes):
        calls.append(send_bytes)
        return 1

    thunk = _lib.ALLGATHERV_FN(fn)
    try:
        assert ctx.lib.rattle_hip_set_exchange(ctx.h, 1, 2, thunk, None) == 0
        call = Call(ctx.lib, ctx.h)
        rc, msg = call()
        assert rc == -3 and b"one rank of several" in msg
        rc, msg = call(max_iters=0)
        assert rc == -2 and b"max_iters" in msg
        assert calls == []
    finally:
        ctx.close()


def test_the_cli_knows_the_flags_and_refuses_the_bad_combinations(rattle, tmp_path):
    r = subprocess.run([rattle, "assign", "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("--abundance", "--abundance-ratio", "--abundance-tol", "--abundance-iters", "abundance.tsv", "est_reads", "cpm"):
        assert word in r.stderr, word
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r0\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    base = [rattle, "assign", "-i", str(fq), "-x", str(fq), "-o", str(out)]
    for extra, word in ((["--abundance-ratio", "0.9"], "--abundance-ratio needs --abundance"), (["--abundance-tol", "0.1"], "--abundance-tol needs --abundance"),
                        (["--abundance-iters", "5"], "--abundance-iters needs --abundance"),
                        (["--abundance", "--abundance-ratio", "0"], "--abundance-ratio"), (["--abundance", "--abundance-ratio", "1.01"], "--abundance-ratio"),
                        (["--abundance", "--abundance-ratio", "x"], "--abundance-ratio"), (["--abundance", "--abundance-tol", "-1"], "--abundance-tol"),
                        (["--abundance", "--abundance-tol", "1048576"], "--abundance-tol"), (["--abundance", "--abundance-tol", "1e"], "--abundance-tol"),
                        (["--abundance", "--abundance-iters", "0"], "--abundance-iters"), (["--abundance", "--abundance-iters", "2.5"], "--abundance-iters"),
                        (["--abundance", "--abundance-iters", "-3"], "--abundance-iters"), (["--abundance", "--devices", "0,1"], "--devices")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
        assert os.listdir(out) == [], extra


def test_abundance_tsv_on_a_hand_made_record():
    """Three reads on three targets: a on t1 with a runner-up, b unassigned, c on t0 alone; the estimates are made up"""
    third = 1.0 / 3.0
    rec = {"target": np.array([1, -1, 0], np.int32), "second_score": np.array([0.25, -1.0, -1.0])}
    ab = {"compatible_reads": np.array([2, 1, 0], np.uint32), "est_reads": np.array([1.0 + third, 2.0 * third, 0.0]),
          "cpm": np.array([2e6 * third, 1e6 * third, 0.0])}
    text = api.abundance_tsv([b"t0", b"t1", b"t2"], [154, 400, 90], rec, ab)
    assert text == (b"target\tlength\treads\tunique_reads\tcompatible_reads\test_reads\tcpm\n"
                    b"t0\t154\t1\t1\t2\t1.3333333333333333\t666666.66666666663\n"
                    b"t1\t400\t1\t0\t1\t0.66666666666666663\t333333.33333333331\n"
                    b"t2\t90\t0\t0\t0\t0\t0\n")
    counts = api.target_counts_tsv([b"t0", b"t1", b"t2"], [154, 400, 90], rec).split(b"\n")
    for line, count in zip(text.split(b"\n")[1:4], counts[1:4]):      # the first four columns are target_counts.tsv's
        f = line.split(b"\t")
        assert b"\t".join(f[:4]) == count
    for line, t in zip(text.split(b"\n")[1:4], range(3)):               # %.17g gives every double back
        f = line.split(b"\t")
        assert float(f[5]) == ab["est_reads"][t] and float(f[6]) == ab["cpm"][t]
