"""`rattle assign --paf --pileup` on the input of test_gpu_cli_assign_paf.py (rebuilt here): pileup.tsv is byte for byte
api.pileup_tsv of the Python call, with and without --cigar; every other file is byte for byte that of the run without the flag; with
--secondary 2 the file is the one without it (rank 0 alone is counted); with --paf-end-to-end and --paf-scoring 5,4,8,6 it is the table
of the plain-Python contract (tests/pileup_ref.py over tests/align_model.py); stderr names the positions covered and the largest depth;
and the flag without --paf is refused."""
import os
import subprocess

import numpy as np
import pytest

import align_model as M
import align_ref
import pileup_ref as P
from conftest import ROOT
from rattle_amd import api

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
RUNS = (("paf", ["--paf"]), ("cigar", ["--paf", "--cigar"]), ("pileup", ["--paf", "--pileup"]), ("pileup_cigar", ["--paf", "--cigar", "--pileup"]),
        ("ranked", ["--paf", "--cigar", "--secondary", "2"]), ("ranked_pileup", ["--paf", "--cigar", "--secondary", "2", "--pileup"]),
        ("ends", ["--paf", "--paf-end-to-end", "--paf-scoring", "5,4,8,6"]),
        ("ends_pileup", ["--paf", "--paf-end-to-end", "--paf-scoring", "5,4,8,6", "--pileup", "--paf-max-cells", "25000"]))
TABLES = ("assignments.tsv", "target_counts.tsv")


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
    tmp = tmp_path_factory.mktemp("cli_assign_pileup")
    targets, reads = build_input()
    fq, tx = tmp / "reads.fastq", tmp / "tx.fastq"
    fq.write_bytes(b"".join(b"@read%d strand=%d\n%s\n+\n%s\n" % (i, i % 2, s, b"I" * len(s)) for i, s in enumerate(reads)))
    tx.write_bytes(b"".join(b"@tx%d len=%d\n%s\n+\n%s\n" % (i, len(s), s, b"I" * len(s)) for i, s in enumerate(targets)))
    out = {}
    for name, extra in RUNS:
        out[name] = tmp / name
        out[name].mkdir()
        r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", str(tx), "-o", str(out[name])] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name + ".stderr"] = r.stderr
    rh = [b"@read%d strand=%d" % (i, i % 2) for i in range(len(reads))]
    th = [b"@tx%d len=%d" % (i, len(s)) for i, s in enumerate(targets)]
    return targets, reads, out, (rh, reads, th, targets), (str(fq), str(tx), tmp)


def test_every_other_file_is_that_of_the_run_without_the_flag(runs):
    _, _, out, _, _ = runs
    for with_flag, without, files in (("pileup", "paf", TABLES + ("alignments.paf",)), ("pileup_cigar", "cigar", TABLES + ("alignments.paf",)),
                                      ("ranked_pileup", "ranked", TABLES + ("alignments.paf", "candidates.tsv"))):
        assert sorted(os.listdir(out[without])) == sorted(files)
        assert sorted(os.listdir(out[with_flag])) == sorted(files + ("pileup.tsv",))
        for f in files:
            assert (out[with_flag] / f).read_bytes() == (out[without] / f).read_bytes(), (with_flag, f)
        assert "pileup:" not in out[without + ".stderr"]
    assert b"cg:Z:" in (out["pileup_cigar"] / "alignments.paf").read_bytes() and b"cg:Z:" not in (out["pileup"] / "alignments.paf").read_bytes()
    for f in TABLES:
        assert (out["ends_pileup"] / f).read_bytes() == (out["ends"] / f).read_bytes()


def test_the_file_is_the_python_paths(gpu_ctx, runs):
    _, _, out, args, _ = runs
    got = (out["pileup"] / "pileup.tsv").read_bytes()
    tsv, counts, paf, text = api.assign_paf_command(gpu_ctx, *args, pileup=True)
    assert (tsv, counts, paf) == tuple((out["paf"] / f).read_bytes() for f in TABLES + ("alignments.paf",))
    assert got == text
    # --cigar changes nothing in it, nor does --secondary: rank 0 alone is counted
    assert (out["pileup_cigar"] / "pileup.tsv").read_bytes() == got == (out["ranked_pileup"] / "pileup.tsv").read_bytes()
    assert api.assign_paf_command(gpu_ctx, *args, pileup=True, cigar=True)[3] == got
    ranked = api.assign_paf_command(gpu_ctx, *args, pileup=True, cigar=True, secondary=2)
    assert len(ranked) == 5 and ranked[4] == got and ranked[:4] == api.assign_paf_command(gpu_ctx, *args, cigar=True, secondary=2)
    # the layout: a header, then tab-separated lines of 12 fields whose depth is the sum of five of them and never 0, in file order
    lines = got.decode().split("\n")
    assert lines[0].split("\t") == ["target", "pos", "ref", "depth", "A", "C", "G", "T", "del", "ins", "starts", "ends"] and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert len(rows) > 500 and all(len(r) == 12 for r in rows)
    targets = args[3]
    for r in rows:
        x, pos, n = int(r[0][2:]), int(r[1]), [int(v) for v in r[3:]]
        assert r[2] == chr(targets[x][pos]) and n[0] == sum(n[1:6]) > 0
    keys = [(int(r[0][2:]), int(r[1])) for r in rows]
    assert keys == sorted(set(keys))
    # stderr: positions covered and the largest depth
    assert f"pileup: {len(rows)} transcript positions covered, largest depth {max(int(r[3]) for r in rows)}" in out["pileup.stderr"]
    # the sums of the header: one start and one end per line of alignments.paf, matches + mismatches in the letters, nd:i: in del
    paf_lines = [l.split(b"\t") for l in paf.split(b"\n")[:-1]]
    assert sum(int(r[10]) for r in rows) == sum(int(r[11]) for r in rows) == len(paf_lines) >= 30
    assert sum(int(v) for r in rows for v in r[4:8]) == sum(int(l[9]) + int(l[14][5:]) for l in paf_lines)
    assert sum(int(r[8]) for r in rows) == sum(int(l[16][5:]) for l in paf_lines)


def test_end_to_end_and_scored_it_is_the_models_table(gpu_ctx, runs):
    targets, reads, out, args, _ = runs
    rows = [l.split("\t") for l in (out["ends"] / "assignments.tsv").read_bytes().decode().split("\n")[1:-1]]
    tor = [int(r[1][2:]) if r[1] != "*" else -1 for r in rows]
    rev = [int(r[2] == "-") for r in rows]
    clean = [s if i != 7 else b"" for i, s in enumerate(reads)]           # (read 7, with its N, is not placed: tor[7] is -1)
    assert tor[7] == -1 and sum(t >= 0 for t in tor) >= 30
    case = (targets, clean, tor, rev)
    rec, _, planes = P.model("cli_sample", case, P.ENGINE, M.READ, 25000)
    assert (rec["status"] == 2).any() and (rec["status"] == 0).sum() >= 10      # --paf-max-cells leaves some out of the table too
    want = api.pileup_tsv([b"tx%d" % i for i in range(len(targets))], targets, dict(zip(P.FIELDS, (np.array(p, np.uint32) for p in planes))))
    got = (out["ends_pileup"] / "pileup.tsv").read_bytes()
    assert got == want
    assert got == api.assign_paf_command(gpu_ctx, *args, pileup=True, end_to_end=True, scoring=(5, 4, 8, 6), max_cells=25000)[3]
    assert got != (out["pileup"] / "pileup.tsv").read_bytes()


def test_the_flag_without_paf_is_refused(runs):
    fq, tx, tmp = runs[4]
    out = tmp / "refused"
    out.mkdir()
    for bad in (["--pileup"], ["--pileup", "--secondary", "2"], ["--pileup", "--abundance"]):
        r = subprocess.run([RATTLE, "assign", "-i", fq, "-x", tx, "-o", str(out)] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and "--pileup needs --paf" in r.stderr, bad
    assert os.listdir(out) == []
