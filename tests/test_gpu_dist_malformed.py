"""`cluster_subsets` as rank 0 of 2 on one device, over a callback transport that hands it the other rank's piece (tests/test_wire.py:
LoneRankTransport): with the piece as rank 1 sent it the four sets equal a single-rank call's, and with the piece damaged the call
returns RATTLE_ERR_HIP, leaves no set behind, and the context goes on working.  The damage is in host bytes and the expected outcome
is an error return: nothing here can fault the device.  (The formats themselves, byte by byte: tests/stubs/wire_check.cpp.)"""
import ctypes as C
import struct

import numpy as np
import pytest

from rattle_amd import _lib, synth
from rattle_amd._lib import ClusterParams, ClusterSet
from test_wire import LoneRankTransport

pytestmark = pytest.mark.gpu

SIZES = (14, 12, 10, 8)          # LPT by n^2 over two ranks: 196 -> rank 0, 144 and 100 -> rank 1, 64 -> rank 0


def subsets_call(ctx, subsets):
    """rattle_hip_cluster_subsets as api.Context.cluster_subsets calls it, but the return code and the raw outs come back"""
    P = ClusterParams(0.2, 1000000.0, 0.4, 0.2, 0.05, 0, 0, 0.15, 0)
    n = len(subsets)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in subsets])
    ids = np.concatenate([np.asarray(x, np.uint32) for x in subsets])
    outs = (C.POINTER(ClusterSet) * n)()
    rc = ctx.lib.rattle_hip_cluster_subsets(ctx.h, C.byref(P), ids.ctypes.data_as(C.POINTER(C.c_uint32)), offs.ctypes.data_as(C.POINTER(C.c_uint64)), n, outs, 0)
    err = ctx.lib.rattle_hip_last_error().decode()
    if rc != 0:
        return rc, [bool(outs[i]) for i in range(n)], err
    return rc, [ctx._take_clusters(outs[i]) for i in range(n)], err


def as_lists(sets):
    return [(s.as_list(), [int(x) for x in s.counters[:3]]) for s in sets]


def records(piece):
    """[start, end) of every cluster set in a piece: 12 bytes of header, 64 of counters, the five arrays, padded to 4 bytes"""
    out, at = [], 0
    while at < len(piece):
        _, nc, nm = struct.unpack_from("<III", piece, at)
        end = at + 76 + 4 * nc + 4 * (nc + 1) + 4 * nm + (nc + nm + 3) // 4 * 4
        out.append((at, end))
        at = end
    assert at == len(piece)
    return out


@pytest.fixture(scope="module")
def job():
    from rattle_amd.api import Context
    seqs, _, _, _ = synth.reads(sum(SIZES), 4, 1, True, seed=11, exon=(30, 45))          # eight exons: about 300 nt
    seqs = sorted(seqs, key=lambda s: -len(s))
    bounds = np.cumsum((0,) + SIZES)
    subsets = [np.arange(bounds[i], bounds[i + 1], dtype=np.uint32) for i in range(len(SIZES))]
    ctx = Context(0)
    ctx.load_reads(seqs, 10, True)
    rc, single, err = subsets_call(ctx, subsets)
    assert rc == 0, err
    # rank 1 alone: its piece goes into the transport, and as nothing comes back from rank 0 its own call ends in an error
    T = LoneRankTransport(1)
    T.attach(ctx)
    rc, left, err = subsets_call(ctx, subsets)
    assert rc == _lib.RATTLE_ERR_HIP and not any(left) and "rank 0" in err, (rc, err)
    piece = T.sent
    assert [struct.unpack_from("<I", piece, a)[0] for a, _ in records(piece)] == [1, 2], "rank 1 owns subsets 1 and 2 and sends the larger first"
    yield dict(ctx=ctx, subsets=subsets, single=as_lists(single), piece=piece)
    ctx.close()


def as_rank0(job, piece):
    T = LoneRankTransport(0, piece)
    T.attach(job["ctx"])
    try:
        return subsets_call(job["ctx"], job["subsets"])
    finally:
        _lib.check(job["ctx"].lib.rattle_hip_set_exchange(job["ctx"].h, 0, 1, _lib.ALLGATHERV_FN(), None))


def test_with_the_piece_intact_the_sets_equal_a_single_rank_call(job):
    rc, sets, err = as_rank0(job, job["piece"])
    assert rc == 0, err
    got = as_lists(sets)
    assert [g[0] for g in got] == [s[0] for s in job["single"]]
    assert got == job["single"], "the work counters of a subset do not depend on the rank that clustered it"


def _poke(piece, at, value):
    return piece[:at] + struct.pack("<I", value) + piece[at + 4:]


DAMAGE = {
    "one byte short": lambda p: p[:-1],
    "the second record removed": lambda p: p[:records(p)[1][0]],
    "a subset of rank 0": lambda p: _poke(p, 0, 3),
    "subset == n_subsets": lambda p: _poke(p, 0, len(SIZES)),
    "n_clusters inflated": lambda p: _poke(p, 4, struct.unpack_from("<I", p, 4)[0] + 1),
}


@pytest.mark.parametrize("damage", list(DAMAGE), ids=[k.replace(" ", "_") for k in DAMAGE])
def test_a_damaged_piece_is_an_error_and_leaves_nothing_behind(job, damage):
    piece = DAMAGE[damage](job["piece"])
    assert piece != job["piece"]
    rc, left, err = as_rank0(job, piece)
    assert rc == _lib.RATTLE_ERR_HIP and not any(left), (rc, left, err)
    assert "cluster_subsets exchange" in err and "rank 1" in err, err
    rc, sets, err = subsets_call(job["ctx"], job["subsets"])          # the same context, one rank again
    assert rc == 0 and as_lists(sets) == job["single"], err
