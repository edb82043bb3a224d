"""`rattle assign --paf --paf-end-to-end` on the golden direct-RNA transcriptome and the first 500 records of its reads: with --cigar, with
--paf-scoring 5,4,8,6 and --paf-max-cells on top, and with --secondary 2.  Every line covers the whole read (q_start 0, q_end Lq, the
CIGAR's read columns sum to Lq), every file is byte for byte the Python path's (api.assign_paf_command with end_to_end=True), the tables
are byte for byte those of the run without the flag, whose alignments.paf is the Python path's with end_to_end=False; and the flag
without --paf is refused."""
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT, read_fastq_gz
from rattle_amd import api

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
N_READS = 500
MAX_CELLS = 20_000_000                              # (the first read, 4385 bases on 4351, stays below it)
MODES = (("local", ["--paf", "--cigar"]), ("ends", ["--paf", "--cigar", "--paf-end-to-end"]),
         ("scored", ["--paf", "--paf-end-to-end", "--cigar", "--paf-scoring", "5,4,8,6", "--paf-max-cells", str(MAX_CELLS)]),
         ("plain", ["--paf", "--paf-end-to-end"]), ("ranked", ["--paf", "--cigar", "--secondary", "2", "--paf-end-to-end"]))


@pytest.fixture(scope="module")
def runs(tmp_path_factory, toyset):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_assign_ends")
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


def whole_read(paf: bytes, cigar: bool):
    """every line: q_start 0, q_end = the read's length, and the CIGAR's =, X and I sum to it, its =, X and D to the transcript span"""
    lines = paf.split(b"\n")[:-1]
    for l in lines:
        f = l.split(b"\t")
        lq, qs, qe, ts, te = int(f[1]), int(f[2]), int(f[3]), int(f[7]), int(f[8])
        assert (qs, qe) == (0, lq), l[:80]
        if cigar:
            assert f[-1].startswith(b"cg:Z:")
            n = {o: 0 for o in b"=XID"}
            for k, o in re.findall(rb"(\d+)([=XID])", f[-1][5:]):
                n[o[0]] += int(k)
            assert n[ord("=")] + n[ord("X")] + n[ord("I")] == lq and n[ord("=")] + n[ord("X")] + n[ord("D")] == te - ts, l[:80]
    return len(lines)


def test_every_line_is_the_whole_read_and_the_python_paths(gpu_ctx, runs):
    reads, targets, out, _ = runs
    args = ([r[0] for r in reads], [r[1] for r in reads], [t[0] for t in targets], [t[1] for t in targets])
    tsv, counts = api.assign_command(gpu_ctx, *args, is_rna=True)
    for name, kw in (("local", dict(cigar=True)), ("ends", dict(cigar=True, end_to_end=True)),
                     ("scored", dict(cigar=True, end_to_end=True, scoring=(5, 4, 8, 6), max_cells=MAX_CELLS)), ("plain", dict(end_to_end=True))):
        assert sorted(os.listdir(out[name])) == ["alignments.paf", "assignments.tsv", "target_counts.tsv"]
        got = tuple((out[name] / f).read_bytes() for f in ("assignments.tsv", "target_counts.tsv", "alignments.paf"))
        assert got[:2] == (tsv, counts), name                             # the tables do not know the flag
        assert got == api.assign_paf_command(gpu_ctx, *args, is_rna=True, **kw), name
    # without the flag: today's file, which api.assign_paf_command(..., end_to_end=False) is as well
    local = (out["local"] / "alignments.paf").read_bytes()
    assert local == api.assign_paf_command(gpu_ctx, *args, is_rna=True, cigar=True, end_to_end=False)[2]
    ends = (out["ends"] / "alignments.paf").read_bytes()
    assert whole_read(ends, True) >= 300 and 1 <= whole_read((out["scored"] / "alignments.paf").read_bytes(), True) <= whole_read(ends, True)
    assert whole_read((out["plain"] / "alignments.paf").read_bytes(), False) == whole_read(ends, True)
    # every placed read has a line (status 0 for every pair), a read that aligned locally among them, and the golden reads have clipped ends
    assert ends.count(b"\n") >= local.count(b"\n") and ends != local
    assert any(int(l.split(b"\t")[2]) > 0 for l in local.split(b"\n")[:-1])


def test_every_rank_is_aligned_in_read_mode(gpu_ctx, runs):
    reads, targets, out, _ = runs
    args = ([r[0] for r in reads], [r[1] for r in reads], [t[0] for t in targets], [t[1] for t in targets])
    assert sorted(os.listdir(out["ranked"])) == ["alignments.paf", "assignments.tsv", "candidates.tsv", "target_counts.tsv"]
    got = tuple((out["ranked"] / f).read_bytes() for f in ("assignments.tsv", "target_counts.tsv", "alignments.paf", "candidates.tsv"))
    assert got == api.assign_paf_command(gpu_ctx, *args, is_rna=True, cigar=True, secondary=2, end_to_end=True)
    assert got[:2] == tuple((out["local"] / f).read_bytes() for f in ("assignments.tsv", "target_counts.tsv"))
    assert got[3] == api.assign_command(gpu_ctx, *args, is_rna=True, secondary=2)[2]
    paf = got[2]
    assert whole_read(paf, True) >= 300 and paf.count(b"\ttp:A:S\trk:i:1\tcg:Z:") >= 1
    # rank 0 of the ranked file is the file without --secondary, tags apart
    rank0 = [l.replace(b"\ttp:A:P\trk:i:0", b"") for l in paf.split(b"\n")[:-1] if b"\trk:i:0\t" in l]
    assert b"".join(l + b"\n" for l in rank0) == (out["ends"] / "alignments.paf").read_bytes()


def test_the_flag_without_paf_is_refused(runs):
    fq, tx, tmp = runs[3]
    out = tmp / "refused"
    out.mkdir()
    for bad in (["--paf-end-to-end"], ["--paf-end-to-end", "--secondary", "2"]):
        r = subprocess.run([RATTLE, "assign", "-i", fq, "-x", tx, "-o", str(out), "--rna"] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and "--paf-end-to-end needs --paf" in r.stderr, bad
    assert os.listdir(out) == []
