"""`rattle assign --paf` on three dozen synthetic reads and five transcripts, both strands, one read with an N and one that nothing
accepts: three files appear, the two tables are byte for byte those of a run without the flag (which still lists exactly two files),
and alignments.paf is api.paf_text fed from the plain-Python contract (tests/align_ref.py) as well as api.assign_paf_command on the same
input."""
import os
import subprocess

import numpy as np
import pytest

import align_ref
from conftest import ROOT
from rattle_amd import api

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")


def build_input():
    """5 transcripts of 120 - 220 bases; 36 reads: pieces of 80 - 100 % of a transcript with 5 % errors, every second one
    reverse-complemented; read 7 carries an N, read 20 is random.  About 1e6 cells for the reference."""
    rng = np.random.default_rng(41)
    targets = [align_ref.rnd(rng, n) for n in (120, 150, 180, 200, 220)]
    reads = []
    for i in range(36):
        t = targets[i % 5]
        lq = int(rng.integers(len(t) * 4 // 5, len(t) + 1))
        a = int(rng.integers(0, len(t) - lq + 1))
        q = align_ref.mutate(rng, t[a:a + lq], 0.05)
        reads.append(align_ref.revcomp(q) if i % 2 else q)
    reads[7] = reads[7][:40] + b"N" + reads[7][41:]
    reads[20] = align_ref.rnd(rng, 150)
    return targets, reads


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_assign_paf")
    targets, reads = build_input()
    fq, tx = tmp / "reads.fastq", tmp / "tx.fastq"
    fq.write_bytes(b"".join(b"@read%d strand=%d\n%s\n+\n%s\n" % (i, i % 2, s, b"I" * len(s)) for i, s in enumerate(reads)))
    tx.write_bytes(b"".join(b"@tx%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(targets)))
    out = {}
    for name, extra in (("plain", []), ("paf", ["--paf"]), ("capped", ["--paf", "--paf-max-cells", "25000"])):
        out[name] = tmp / name
        out[name].mkdir()
        r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(tx), "-o", str(out[name])] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name + ".stderr"] = r.stderr
    return targets, reads, out


def test_three_files_and_the_two_old_ones_unchanged(runs):
    _, _, out = runs
    assert sorted(os.listdir(out["plain"])) == ["assignments.tsv", "target_counts.tsv"]
    assert sorted(os.listdir(out["paf"])) == ["alignments.paf", "assignments.tsv", "target_counts.tsv"]
    for f in ("assignments.tsv", "target_counts.tsv"):
        assert (out["paf"] / f).read_bytes() == (out["plain"] / f).read_bytes(), f
        assert (out["capped"] / f).read_bytes() == (out["plain"] / f).read_bytes(), f


def test_the_paf_is_the_contracts_and_the_librarys(gpu_ctx, runs):
    targets, reads, out = runs
    rh = [b"@read%d strand=%d" % (i, i % 2) for i in range(len(reads))]
    th = [b"@tx%d" % i for i in range(len(targets))]
    tsv, counts, paf = api.assign_paf_command(gpu_ctx, rh, reads, th, targets)
    assert tsv == (out["plain"] / "assignments.tsv").read_bytes() and counts == (out["plain"] / "target_counts.tsv").read_bytes()
    assert (tsv, counts) == api.assign_command(gpu_ctx, rh, reads, th, targets)
    got = (out["paf"] / "alignments.paf").read_bytes()
    assert got == paf
    # the placement from the table, the alignment from the plain-Python contract
    rows = [l.split("\t") for l in tsv.decode().split("\n")[1:-1]]
    asg = {"target": np.array([int(r[1][2:]) if r[1] != "*" else -1 for r in rows], np.int32),
           "rev": np.array([r[2] == "-" for r in rows], np.uint8)}
    assert asg["target"][7] == -1 and asg["target"][20] == -1 and (asg["target"] >= 0).sum() >= 30
    assert (asg["rev"][asg["target"] >= 0] == 1).sum() >= 10 and (asg["rev"][asg["target"] >= 0] == 0).sum() >= 10
    want = align_ref.records(targets, reads, asg["target"], asg["rev"])
    rn, tn = [b"read%d" % i for i in range(len(reads))], [b"tx%d" % i for i in range(len(targets))]
    assert got == api.paf_text(rn, [len(s) for s in reads], tn, [len(s) for s in targets], asg, want)
    lines = got.decode().split("\n")[:-1]
    assert len(lines) == (want["status"] == 0).sum() == (asg["target"] >= 0).sum()
    assert not any(l.startswith(("read7\t", "read20\t")) for l in lines)
    # --paf-max-cells: the reads over it have no line, their count goes to stderr
    capped = align_ref.records(targets, reads, asg["target"], asg["rev"], max_cells=25000)
    n_skipped = int((capped["status"] == 2).sum())
    assert 0 < n_skipped < len(lines)
    assert (out["capped"] / "alignments.paf").read_bytes() == api.paf_text(rn, [len(s) for s in reads], tn, [len(s) for s in targets], asg, capped)
    assert f"{n_skipped}  reads over --paf-max-cells" in out["capped.stderr"] and "--paf-max-cells" not in out["paf.stderr"]
