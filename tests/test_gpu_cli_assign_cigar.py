"""`rattle assign --paf --cigar` on the input of test_gpu_cli_assign_paf.py (rebuilt here): the two tables are byte for byte those of a
plain run, alignments.paf with its cg:Z: tags stripped is byte for byte that of a `--paf` run, every tag is the string of the plain-Python
contract (tests/cigar_ref.py), the file is what api.assign_paf_command(..., cigar=True) returns, and with --paf-max-cells the skipped
reads have no line."""
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref
import cigar_ref
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
    tmp = tmp_path_factory.mktemp("cli_assign_cigar")
    targets, reads = build_input()
    fq, tx = tmp / "reads.fastq", tmp / "tx.fastq"
    fq.write_bytes(b"".join(b"@read%d strand=%d\n%s\n+\n%s\n" % (i, i % 2, s, b"I" * len(s)) for i, s in enumerate(reads)))
    tx.write_bytes(b"".join(b"@tx%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(targets)))
    out = {}
    for name, extra in (("plain", []), ("paf", ["--paf"]), ("cigar", ["--paf", "--cigar"]),
                        ("capped", ["--paf", "--cigar", "--paf-max-cells", "25000"]), ("capped_paf", ["--paf", "--paf-max-cells", "25000"])):
        out[name] = tmp / name
        out[name].mkdir()
        r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(tx), "-o", str(out[name])] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name + ".stderr"] = r.stderr
    return targets, reads, out


TAG = re.compile(rb"\tcg:Z:([0-9=XID]+)\n")


def test_the_tables_and_the_untagged_paf_are_unchanged(runs):
    _, _, out = runs
    assert sorted(os.listdir(out["cigar"])) == ["alignments.paf", "assignments.tsv", "target_counts.tsv"]
    for f in ("assignments.tsv", "target_counts.tsv"):
        assert (out["cigar"] / f).read_bytes() == (out["plain"] / f).read_bytes(), f
        assert (out["capped"] / f).read_bytes() == (out["plain"] / f).read_bytes(), f
    for with_tag, without in (("cigar", "paf"), ("capped", "capped_paf")):
        got, old = (out[with_tag] / "alignments.paf").read_bytes(), (out[without] / "alignments.paf").read_bytes()
        assert b"cg:Z:" not in old and old.count(b"\n") > 0
        assert len(TAG.findall(got)) == got.count(b"\n") == old.count(b"\n")      # every line, at its end
        assert TAG.sub(b"\n", got) == old


def test_every_tag_is_the_contracts_and_the_file_the_librarys(gpu_ctx, runs):
    targets, reads, out = runs
    rh = [b"@read%d strand=%d" % (i, i % 2) for i in range(len(reads))]
    th = [b"@tx%d" % i for i in range(len(targets))]
    tsv, counts, paf = api.assign_paf_command(gpu_ctx, rh, reads, th, targets, cigar=True)
    assert tsv == (out["plain"] / "assignments.tsv").read_bytes() and counts == (out["plain"] / "target_counts.tsv").read_bytes()
    got = (out["cigar"] / "alignments.paf").read_bytes()
    assert got == paf
    assert api.assign_paf_command(gpu_ctx, rh, reads, th, targets)[2] == (out["paf"] / "alignments.paf").read_bytes()
    # the placement from the table, the strings from the plain-Python contract
    rows = [l.split("\t") for l in tsv.decode().split("\n")[1:-1]]
    tor = [int(r[1][2:]) if r[1] != "*" else -1 for r in rows]
    rev = [int(r[2] == "-") for r in rows]
    want = cigar_ref.cigars(targets, reads, tor, rev)
    lines = got.split(b"\n")[:-1]
    tags = {l.split(b"\t")[0]: l.split(b"\t")[-1] for l in lines}
    assert len(tags) == len(lines) == sum(1 for s in want if s) >= 30
    for i, s in enumerate(want):
        assert tags.get(b"read%d" % i, b"cg:Z:")[5:] == s, i
    assert any(b"X" in s for s in want) and any(b"I" in s for s in want) and any(b"D" in s for s in want)
    # --paf-max-cells: the reads over it have no line, their count goes to stderr as before
    capped = cigar_ref.cigars(targets, reads, tor, rev, max_cells=25000)
    n_skipped = sum(1 for a, b in zip(want, capped) if a and not b)
    assert 0 < n_skipped < len(lines)
    clines = (out["capped"] / "alignments.paf").read_bytes().split(b"\n")[:-1]
    assert [l.split(b"\t")[0] for l in clines] == [b"read%d" % i for i, s in enumerate(capped) if s]
    assert all(l.split(b"\t")[-1][5:] == capped[int(l.split(b"\t")[0][4:])] for l in clines)
    assert f"{n_skipped}  reads over --paf-max-cells" in out["capped.stderr"]
    assert (out["capped"] / "alignments.paf").read_bytes() == api.assign_paf_command(gpu_ctx, rh, reads, th, targets, cigar=True, max_cells=25000)[2]
