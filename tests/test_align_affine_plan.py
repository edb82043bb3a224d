"""The host plan of the three-state kernel F (csrc/cigar_plan.h with 32-byte records and two strip words per column) on its own:
tests/stubs/cigar_plan_affine_check.cpp, a stand-alone program over that header alone, built here with -fsanitize=address,undefined.
Counts written out by hand, the saturating products, and the old signature's plan unchanged."""
import os
import subprocess

from conftest import ROOT


def test_the_affine_plan_under_the_sanitizers(tmp_path):
    exe = tmp_path / "cigar_plan_affine_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "stubs", "cigar_plan_affine_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok 12"), (r.stdout, r.stderr)
