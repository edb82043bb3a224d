"""Records the answers of the reference's own translation units (oracle/_ref/libref.so, built from the reference sources by
`make -C oracle ref`) to the calls of tests/test_oracle_cluster.py into tests/golden/ref_units.json.gz, which those tests use where
oracle/_ref cannot be built.  Run it again after changing the calls of those tests.  usage: python tools/record_ref_units.py"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "ref_units.json.gz")
    env = dict(os.environ, RATTLE_RECORD_REF=out)
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_cluster.py"),
                              "-k", "reference_units or var_edge or fasta_cpp"], env=env, cwd=ROOT))
