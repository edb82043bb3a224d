"""`rattle assign --secondary 2` on the golden direct-RNA transcriptome and the first 500 records of its reads: alone, with --paf --cigar,
and with --paf-scoring 5,4,8,6 on top.  Every file is byte for byte the Python path's (api.assign_command / assign_paf_command with
secondary=2), assignments.tsv and target_counts.tsv are byte for byte those of the run without the flag, and what the flag cannot take
is refused with a non-zero exit."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT, read_fastq_gz
from rattle_amd import api

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
N_READS = 500
MODES = (("plain", []), ("secondary", ["--secondary", "2"]), ("paf", ["--secondary", "2", "--paf", "--cigar"]),
         ("scored", ["--secondary=2", "--paf", "--cigar", "--paf-scoring", "5,4,8,6"]))


@pytest.fixture(scope="module")
def runs(tmp_path_factory, toyset):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_assign_secondary")
    reads = toyset[:N_READS]
    fq = tmp / "reads.fastq"
    fq.write_bytes(b"".join(b"%s\n%s\n+\n%s\n" % r for r in reads))
    tx = os.path.join(GOLDEN, "toyset_rna.transcriptome.fq.gz")
    out = {}
    for name, extra in MODES:
        out[name] = tmp / name
        out[name].mkdir()
        r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", tx, "-o", str(out[name]), "--rna"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return reads, read_fastq_gz(tx), out, (str(fq), tx, tmp)


def test_the_files_are_the_python_paths(gpu_ctx, runs):
    reads, targets, out, _ = runs
    args = ([r[0] for r in reads], [r[1] for r in reads], [t[0] for t in targets], [t[1] for t in targets])
    tsv, counts, table = api.assign_command(gpu_ctx, *args, is_rna=True, secondary=2)
    assert sorted(os.listdir(out["plain"])) == ["assignments.tsv", "target_counts.tsv"]
    assert sorted(os.listdir(out["secondary"])) == ["assignments.tsv", "candidates.tsv", "target_counts.tsv"]
    for name in ("secondary", "paf", "scored"):
        assert (out[name] / "assignments.tsv").read_bytes() == tsv == (out["plain"] / "assignments.tsv").read_bytes(), name
        assert (out[name] / "target_counts.tsv").read_bytes() == counts == (out["plain"] / "target_counts.tsv").read_bytes(), name
        assert (out[name] / "candidates.tsv").read_bytes() == table, name
    rows = [l.split(b"\t") for l in table.split(b"\n")[1:-1]]
    # what the golden reads must give for this test to see the flag at work: most reads placed, and a rank beyond 0 at least once (no
    # read of these 500 has three accepting transcripts: rank 2 is tests/test_gpu_assign_paf_ranked.py's)
    assert len(rows) >= 300 and {b"0", b"1"} <= {r[1] for r in rows} <= {b"0", b"1", b"2"}
    assert (tsv, counts) == api.assign_command(gpu_ctx, *args, is_rna=True)
    for name, scoring in (("paf", None), ("scored", (5, 4, 8, 6))):
        assert sorted(os.listdir(out[name])) == ["alignments.paf", "assignments.tsv", "candidates.tsv", "target_counts.tsv"]
        want = api.assign_paf_command(gpu_ctx, *args, is_rna=True, cigar=True, scoring=scoring, secondary=2)
        got = (out[name] / "alignments.paf").read_bytes()
        assert want == (tsv, counts, got, table), name
        assert got.count(b"\ttp:A:P\trk:i:0\tcg:Z:") >= 100 and got.count(b"\ttp:A:S\trk:i:1\tcg:Z:") >= 1
    assert (out["paf"] / "alignments.paf").read_bytes() != (out["scored"] / "alignments.paf").read_bytes()


def test_what_the_flag_cannot_take_is_refused(runs):
    fq, tx, tmp = runs[3]
    out = tmp / "refused"
    out.mkdir()
    for bad in (["--secondary", "0"], ["--secondary", "8"], ["--secondary", "x"], ["--secondary", "2", "--devices", "0,1"]):
        r = subprocess.run([RATTLE, "assign", "-i", fq, "-x", tx, "-o", str(out), "--rna"] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and "Error" in r.stderr, bad
    assert os.listdir(out) == []
