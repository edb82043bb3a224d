"""The host plan of kernel F (csrc/cigar_plan.h: which pairs of kernel E's chunk go on, their code records, strip and ops words, the
sub-chunks under the cap on code bytes) on its own: tests/stubs/cigar_plan_check.cpp, a stand-alone program over that header alone, built
here with -fsanitize=address,undefined."""
import os
import subprocess

from conftest import ROOT


def test_the_plan_under_the_sanitizers(tmp_path):
    exe = tmp_path / "cigar_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "stubs", "cigar_plan_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok 414"), (r.stdout, r.stderr)
