"""What the ranks of one job send each other is read by one bounds-checked reader (rattle_amd/csrc/wire.h), and a damaged piece is an
error return, not a read or write out of bounds.

A. tests/stubs/wire_check.cpp, a stand-alone program over wire.h alone, built here with -fsanitize=address,undefined: the four
   payloads written, read back and compared, then damaged in every way the formats can be (see the program's head).
B. Through the library, on host-only contexts: a correction gathered over a callback transport from a piece that is intact, then
   truncated and inflated.  The transport plays a world of two with one live rank (the other one's piece is what it was handed
   before), so both ranks run one after the other in this process.
The same for `cluster_subsets`, which needs a device, is tests/test_gpu_dist_malformed.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rattle_amd import _lib
from rattle_amd._lib import Correction


@pytest.fixture(scope="module")
def wire_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wire") / "wire_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "stubs", "wire_check.cpp")])
    return str(exe)


def test_the_four_payloads_round_trip_and_every_damaged_piece_is_rejected_cleanly(wire_check):
    r = subprocess.run([wire_check], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WIRE_CHECK_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


class LoneRankTransport:
    """A rattle_allgatherv_fn for `rank` of a world of two in which only this rank runs: the other rank's piece is `peer_piece`.  The
    library gathers the sizes first and the payload second, so the calls come in pairs; `sent` is the payload this rank put in."""

    def __init__(self, rank: int, peer_piece: bytes = b""):
        self.rank, self.peer_piece, self.sent, self.calls = rank, peer_piece, None, 0
        self.fn = _lib.ALLGATHERV_FN(self._call)           # (kept alive with the object)

    def _call(self, user, send, send_bytes, recv, recv_bytes):
        try:
            mine = C.string_at(send, send_bytes)
            sizes = self.calls % 2 == 0
            self.calls += 1
            if sizes:
                assert send_bytes == 8
                parts = [mine, mine]
                parts[1 - self.rank] = struct.pack("<Q", len(self.peer_piece))
            else:
                self.sent = mine
                parts = [mine, mine]
                parts[1 - self.rank] = self.peer_piece
            assert [int(recv_bytes[0]), int(recv_bytes[1])] == [len(parts[0]), len(parts[1])]
            flat = parts[0] + parts[1]
            if flat:
                C.memmove(recv, flat, len(flat))
            return 0
        except Exception as e:  # never unwind through the C frame
            print(f"exchange callback failed: {e!r}")
            return 1

    def attach(self, ctx):
        _lib.check(ctx.lib.rattle_hip_set_exchange(ctx.h, self.rank, 2, self.fn, None))


@pytest.fixture(scope="module")
def gather_job():
    """test_dist_cpu's job in a world of two: each rank's share, the piece rank 1 sends to the root, the unsharded result's digest"""
    from rattle_amd.api import Context, correction_digest
    from test_dist_cpu import _plan, make_job, stub_correction
    off, coff, mid, mrev, seqs = make_job()
    plan = _plan(off, coff, mid, mrev, 2)
    shares = [stub_correction(plan, seqs, r) for r in (0, 1)]
    whole, keep = stub_correction(_plan(off, coff, mid, mrev, 1), seqs, 0)
    ctx = Context(None)
    T = LoneRankTransport(1)
    T.attach(ctx)
    merged = C.POINTER(Correction)()
    rc = ctx.lib.rattle_hip_correction_gather(ctx.h, C.byref(shares[1][0]), 0, C.byref(merged))
    assert rc == 0, ctx.lib.rattle_hip_last_error()
    assert not merged and T.calls == 2 and len(T.sent) > 1000 and len(T.sent) % 8 == 0
    ctx.close()
    return dict(shares=shares, piece=T.sent, want=correction_digest(whole), plan=plan)


def _gather_on_root(job, piece, ctx=None):
    from rattle_amd.api import Context
    ctx = ctx or Context(None)
    T = LoneRankTransport(0, piece)
    T.attach(ctx)
    merged = C.POINTER(Correction)()
    rc = ctx.lib.rattle_hip_correction_gather(ctx.h, C.byref(job["shares"][0][0]), 0, C.byref(merged))
    err = ctx.lib.rattle_hip_last_error().decode()
    assert T.sent == b"", "the root's own share never travels"
    return ctx, rc, merged, err


def test_a_gathered_correction_equals_the_unsharded_one(gather_job):
    from rattle_amd.api import correction_digest
    ctx, rc, merged, err = _gather_on_root(gather_job, gather_job["piece"])
    assert rc == 0, err
    R = merged.contents
    assert correction_digest(R) == gather_job["want"], "merged result differs from the unsharded one"
    pk = np.ctypeslib.as_array(R.corrected_pack, (R.corrected.n,))
    assert np.all(np.diff(pk.astype(np.int64)) >= 0), "corrected reads not in pack order"
    assert int(R.counters[0]) == sum(int(c) for c in gather_job["plan"]["cost"]) and R.skipped.n == 2
    ctx.lib.rattle_hip_correction_free(merged)
    ctx.close()


def _inflated(piece):
    n, = struct.unpack_from("<Q", piece, 0)
    return struct.pack("<Q", n + 1) + piece[8:]


@pytest.mark.parametrize("damage", [lambda p: p[:-1], lambda p: p[:-8], _inflated, lambda p: struct.pack("<Q", 2 ** 63) + p[8:], lambda p: b""],
                         ids=["one byte short", "last eight bytes gone", "first set's n inflated", "first set's n = 2^63", "empty"])
def test_a_damaged_piece_is_an_error_of_the_gather_that_names_its_rank(gather_job, damage):
    from rattle_amd.api import correction_digest
    ctx, rc, merged, err = _gather_on_root(gather_job, damage(gather_job["piece"]))
    assert rc == _lib.RATTLE_ERR_HIP and not merged, (rc, err)
    assert "correction gather" in err and "rank 1" in err, err
    # the context is as good as before
    ctx, rc, merged, err = _gather_on_root(gather_job, gather_job["piece"], ctx)
    assert rc == 0 and correction_digest(merged.contents) == gather_job["want"], err
    ctx.lib.rattle_hip_correction_free(merged)
    ctx.close()
