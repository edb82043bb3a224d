"""The correction report at the edges that need no device: the entry points exist under ABI 4, the switch is accepted on a host
context, and a correction without a report -- one merged from shares made with the switch off, or an object the library did not
make -- is a state error with a message that says what to do; a NULL correction is an argument error."""
import ctypes as C

import pytest

from rattle_amd import _lib
from rattle_amd._lib import Correction, CorrectionReport
from rattle_amd.api import Context, unpack_correction
from test_dist_cpu import _plan, make_job, stub_correction


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def test_the_symbols_exist_under_abi_4():
    lib = _lib.load()
    for name in ("rattle_hip_set_correction_report", "rattle_hip_correction_report", "rattle_hip_correction_report_free"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rattle_hip_abi_version() == 4
    assert [f for f, _ in CorrectionReport._fields_] == ["n", "in_len", "out_len", "trim_front", "trim_back", "match", "substituted",
                                                          "mismatch_kept", "inserted", "deleted", "gap_kept"]


def test_the_switch_is_accepted_on_a_host_context_and_a_null_context_is_not(host_ctx):
    lib = host_ctx.lib
    assert lib.rattle_hip_set_correction_report(host_ctx.h, 1) == 0
    assert lib.rattle_hip_set_correction_report(host_ctx.h, 0) == 0
    host_ctx.set_correction_report(True)
    host_ctx.set_correction_report(False)
    assert lib.rattle_hip_set_correction_report(None, 1) == -2


def test_a_correction_without_a_report_is_a_state_error(host_ctx):
    """a share made without the switch (here: by the stub that stands in for the kernels), merged on a host context that has the
    switch on: neither the share nor the merged object has a report"""
    lib = host_ctx.lib
    off, coff, mid, mrev, seqs = make_job()
    local, keep = stub_correction(_plan(off, coff, mid, mrev, 1), seqs, 0)
    out = C.POINTER(CorrectionReport)()
    assert lib.rattle_hip_correction_report(C.byref(local), C.byref(out)) == -3 and not out
    assert b"rattle_hip_set_correction_report" in lib.rattle_hip_last_error()
    assert "report" not in unpack_correction(local) and len(unpack_correction(local)["corrected"]) == local.corrected.n
    host_ctx.set_correction_report(True)
    try:
        merged = C.POINTER(Correction)()
        assert lib.rattle_hip_correction_gather(host_ctx.h, C.byref(local), 0, C.byref(merged)) == 0, lib.rattle_hip_last_error()
        assert merged.contents.corrected.n == local.corrected.n > 0
        assert lib.rattle_hip_correction_report(merged, C.byref(out)) == -3 and not out
        assert "report" not in unpack_correction(merged)
        assert b"rattle_hip_set_correction_report" in lib.rattle_hip_last_error()
        lib.rattle_hip_correction_free(merged)
    finally:
        host_ctx.set_correction_report(False)


def test_a_null_correction_is_an_argument_error():
    lib = _lib.load()
    out = C.POINTER(CorrectionReport)()
    assert lib.rattle_hip_correction_report(None, C.byref(out)) == -2 and not out
    assert lib.rattle_hip_correction_report(None, None) == -2
    lib.rattle_hip_correction_report_free(None)          # like every *_free: NULL is accepted
