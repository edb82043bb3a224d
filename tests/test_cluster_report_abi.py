"""The cluster report at the edges that need no device: the three entry points exist under ABI 4, the switch is accepted on a host
context, and a cluster set without joins behind it -- one a caller built itself -- is a state error with a message that says what
to do, not a read behind the struct; NULL arguments are argument errors and every *_free takes NULL."""
import ctypes as C

import numpy as np
import pytest

from rattle_amd import _lib
from rattle_amd._lib import ClusterReport, ClusterSet
from rattle_amd.api import Context, cluster_report

NAMES = ("rattle_hip_set_cluster_report", "rattle_hip_cluster_report", "rattle_hip_cluster_report_free")


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in ClusterReport._fields_] == ["n", "level", "pass", "bv_threshold", "into", "absorbed", "rev", "bases", "hc_bases",
                                                      "min_len", "score", "variance"]
    # the evidence of the test hook comes after everything the earlier mirror knew
    assert [f for f, _ in _lib.DebugEval._fields_][-4:] == ["oversize_pairs", "hit_bases", "hit_hc_bases", "hit_variance"]


def test_the_switch_is_accepted_on_a_host_context_and_a_null_context_is_not(host_ctx):
    lib = host_ctx.lib
    assert lib.rattle_hip_set_cluster_report(host_ctx.h, 1) == 0
    assert lib.rattle_hip_set_cluster_report(host_ctx.h, 0) == 0
    host_ctx.set_cluster_report(True)
    assert host_ctx.cluster_report
    host_ctx.set_cluster_report(False)
    assert not host_ctx.cluster_report
    assert lib.rattle_hip_set_cluster_report(None, 1) == -2


def foreign_set():
    """a cluster set the caller built: two clusters over three reads"""
    keep = [np.array([0, 2], np.int32), np.zeros(2, np.uint8), np.array([0, 2, 3], np.uint32), np.array([0, 1, 2], np.int32),
            np.zeros(3, np.uint8)]
    cs = ClusterSet(2, *[a.ctypes.data_as(C.POINTER(t)) for a, t in zip(keep, (C.c_int32, C.c_uint8, C.c_uint32, C.c_int32, C.c_uint8))])
    return cs, keep


def test_a_foreign_cluster_set_is_a_state_error_not_a_crash():
    lib = _lib.load()
    cs, keep = foreign_set()
    out = C.POINTER(ClusterReport)()
    assert lib.rattle_hip_cluster_report(C.byref(cs), C.byref(out)) == -3 and not out
    assert b"rattle_hip_set_cluster_report" in lib.rattle_hip_last_error()
    assert cluster_report(lib, C.pointer(cs)) is None
    # a heap copy of it, as far from the library's own objects as a caller's allocation is
    buf = (C.c_uint8 * C.sizeof(ClusterSet))()
    C.memmove(buf, C.byref(cs), C.sizeof(ClusterSet))
    assert lib.rattle_hip_cluster_report(C.cast(buf, C.POINTER(ClusterSet)), C.byref(out)) == -3 and not out


def test_null_arguments():
    lib = _lib.load()
    cs, keep = foreign_set()
    out = C.POINTER(ClusterReport)()
    assert lib.rattle_hip_cluster_report(None, C.byref(out)) == -2 and not out
    assert lib.rattle_hip_cluster_report(C.byref(cs), None) == -2
    lib.rattle_hip_cluster_report_free(None)            # like every *_free: NULL is accepted
    lib.rattle_hip_cluster_set_free(None)
