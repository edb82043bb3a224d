"""The "index" count pass at the library's edges that need no device: rattle_hip_debug_evaluate accepts count_pass = 3 (on a host
context the call passes the argument check and stops at the missing device), still refuses values outside 0 .. 3, and the CLI
refuses an unknown --count-pass."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from rattle_amd import _lib

RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
ERR_ARG, ERR_STATE = -2, -3


@pytest.fixture(scope="module")
def host_ctx():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rattle_hip_ctx_create_host(C.byref(h)) == 0
    yield lib, h
    lib.rattle_hip_ctx_destroy(h)


def evaluate(lib, h, count_pass):
    P = _lib.ClusterParams(0.2, 1e6, 0.0, 0.0, 0.0, 0, 0, 0.0, 0)
    out = C.POINTER(_lib.DebugEval)()
    rc = lib.rattle_hip_debug_evaluate(h, C.byref(P), count_pass, None, 0, C.byref(out))
    assert not out                                              # nothing is handed out on an error
    return rc, lib.rattle_hip_last_error().decode()


@pytest.mark.parametrize("count_pass", [0, 1, 2, 3])
def test_known_count_passes_reach_the_device_check(host_ctx, count_pass):
    rc, msg = evaluate(*host_ctx, count_pass)
    assert rc == ERR_STATE and "no device" in msg, (rc, msg)


@pytest.mark.parametrize("count_pass", [-1, 4, 7])
def test_unknown_count_passes_are_argument_errors(host_ctx, count_pass):
    rc, msg = evaluate(*host_ctx, count_pass)
    assert rc == ERR_ARG and "count_pass" in msg and "index" in msg, (rc, msg)


def test_abi_version_is_unchanged(host_ctx):
    assert host_ctx[0].rattle_hip_abi_version() == 4


def test_cli_refuses_an_unknown_count_pass(tmp_path):
    assert os.path.exists(RATTLE)
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    r = subprocess.run([RATTLE, "cluster", "-i", str(fq), "-o", str(tmp_path), "--count-pass", "bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--count-pass" in r.stderr and "usage" in r.stderr and "bogus" in r.stderr and "index" in r.stderr
    assert not (tmp_path / "clusters.out").exists()
    # the known values are documented by --help
    h = subprocess.run([RATTLE, "cluster", "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--count-pass auto|seed|search|index" in h.stderr
