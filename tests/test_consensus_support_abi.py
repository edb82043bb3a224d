"""The consensus support at the edges that need no device: the entry points exist under ABI 4, the switch is accepted on a host
context, a correction without a support -- one made with the switch off (here: by the stub that stands in for the kernels, and its
copy from the gather), or an object the library did not make -- is a state error with a message that says what to do, and the
free functions take NULL."""
import ctypes as C

import pytest

from rattle_amd import _lib
from rattle_amd._lib import ConsensusSupport, Correction
from rattle_amd.api import Context, consensus_support, unpack_correction
from test_dist_cpu import _plan, make_job, stub_correction


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in ("rattle_hip_set_consensus_support", "rattle_hip_consensus_support", "rattle_hip_consensus_support_free",
                 "rattle_hip_debug_consensus_support", "rattle_hip_debug_consensus_support_free"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in ConsensusSupport._fields_] == ["n", "level", "off", "support", "depth", "pack_support", "pack_depth"]


def test_the_switch_is_accepted_on_a_host_context_and_a_null_context_is_not(host_ctx):
    lib = host_ctx.lib
    assert lib.rattle_hip_set_consensus_support(host_ctx.h, 1) == 0
    assert lib.rattle_hip_set_consensus_support(host_ctx.h, 0) == 0
    host_ctx.set_consensus_support(True)
    assert host_ctx.consensus_support
    host_ctx.set_consensus_support(False)
    assert not host_ctx.consensus_support
    assert lib.rattle_hip_set_consensus_support(None, 1) == -2


def test_a_correction_without_a_support_is_a_state_error(host_ctx):
    """a struct the caller built is not the library's object; its copy from the gather is, but carries no support either -- also
    when the gathering context has the switch on"""
    lib = host_ctx.lib
    off, coff, mid, mrev, seqs = make_job()
    local, keep = stub_correction(_plan(off, coff, mid, mrev, 1), seqs, 0)
    out = C.POINTER(ConsensusSupport)()
    assert lib.rattle_hip_consensus_support(C.byref(local), C.byref(out)) == -3 and not out
    assert b"rattle_hip_set_consensus_support" in lib.rattle_hip_last_error()
    assert consensus_support(lib, C.pointer(local)) is None and "support" not in unpack_correction(local)
    host_ctx.set_consensus_support(True)
    try:
        merged = C.POINTER(Correction)()
        assert lib.rattle_hip_correction_gather(host_ctx.h, C.byref(local), 0, C.byref(merged)) == 0, lib.rattle_hip_last_error()
        assert merged.contents.consensi.n == local.consensi.n
        assert lib.rattle_hip_consensus_support(merged, C.byref(out)) == -3 and not out
        assert b"rattle_hip_set_consensus_support" in lib.rattle_hip_last_error()
        assert "support" not in unpack_correction(merged)
        lib.rattle_hip_correction_free(merged)
    finally:
        host_ctx.set_consensus_support(False)


def test_null_arguments_and_free_of_null():
    lib = _lib.load()
    out = C.POINTER(ConsensusSupport)()
    assert lib.rattle_hip_consensus_support(None, C.byref(out)) == -2 and not out
    assert lib.rattle_hip_consensus_support(None, None) == -2
    lib.rattle_hip_consensus_support_free(None)
    lib.rattle_hip_debug_consensus_support_free(None)


def test_the_debug_hook_needs_a_device(host_ctx):
    """on a host context the hook validates its input and then refuses: nothing is launched"""
    import numpy as np
    lib = host_ctx.lib
    first = np.zeros(1, np.uint32); off = np.zeros(1, np.uint64)
    M = _lib.DebugSupportMsa(0, first.ctypes.data_as(C.POINTER(C.c_uint32)), None, off.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None, None)
    P = _lib.CorrectParams()
    out = C.POINTER(_lib.DebugSupport)()
    assert lib.rattle_hip_debug_consensus_support(host_ctx.h, C.byref(P), C.byref(M), C.byref(out)) == -3 and not out
    sup = np.ones(1, np.uint32)
    M.sup = sup.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.rattle_hip_debug_consensus_support(host_ctx.h, C.byref(P), C.byref(M), C.byref(out)) == -2      # sup without dep
