"""`rattle assign` on the golden direct-RNA transcriptome and the first 1500 records of its reads: assignments.tsv and
target_counts.tsv are byte for byte what api.assign_command returns, the counts are those of the assignments, a fixed sample of 150
reads is the oracle's brute force field by field (tests/assign_ref.py), the result does not depend on --target-batch / --read-chunk /
--count-pass, and a job over several devices is refused."""
import os
import subprocess

import numpy as np
import pytest

import assign_ref
from conftest import GOLDEN, ROOT, read_fastq_gz
from rattle_amd import api
from test_gpu_cluster_eval import Ref

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
N_READS, N_SAMPLE = 1500, 150
COLUMNS = ["read", "target", "strand", "score", "second_score", "n_accepted", "bases", "hc_bases", "min_len", "variance"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, toyset):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_assign")
    reads = toyset[:N_READS]
    fq = tmp / "reads.fastq"
    fq.write_bytes(b"".join(b"%s\n%s\n+\n%s\n" % r for r in reads))
    tx = os.path.join(GOLDEN, "toyset_rna.transcriptome.fq.gz")
    out = {}
    for name, extra in (("plain", []), ("other", ["--target-batch", "50", "--read-chunk", "400", "--count-pass", "index"])):
        out[name] = tmp / name
        out[name].mkdir()
        subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", tx, "-o", str(out[name]), "--rna"] + extra, check=True, capture_output=True)
    return fq, reads, read_fastq_gz(tx), out


def test_the_files_are_the_librarys_and_agree_with_each_other(gpu_ctx, runs):
    fq, reads, targets, out = runs
    assert sorted(os.listdir(out["plain"])) == ["assignments.tsv", "target_counts.tsv"]
    text, counts = (out["plain"] / "assignments.tsv").read_bytes(), (out["plain"] / "target_counts.tsv").read_bytes()
    want = api.assign_command(gpu_ctx, [r[0] for r in reads], [r[1] for r in reads], [t[0] for t in targets], [t[1] for t in targets],
                              is_rna=True)
    assert text == want[0] and counts == want[1]
    for f in ("assignments.tsv", "target_counts.tsv"):                # batches, chunks and the count pass change nothing
        assert (out["other"] / f).read_bytes() == (out["plain"] / f).read_bytes(), f
    lines = text.decode().split("\n")
    assert lines[0].split("\t") == COLUMNS and lines[-1] == "" and len(lines) == N_READS + 2
    rows = [l.split("\t") for l in lines[1:-1]]
    assert [r[0] for r in rows] == [api._first_token(r[0]).decode() for r in reads]
    placed = [r for r in rows if r[1] != "*"]
    assert len(placed) >= 100 and all(r[2] == "+" for r in placed) and all(r[2] == "*" and r[5] == "0" for r in rows if r[1] == "*")
    clines = counts.decode().split("\n")
    assert clines[0].split("\t") == ["target", "length", "reads", "unique_reads"] and len(clines) == len(targets) + 2
    for c, t in zip(clines[1:-1], targets):
        name, length, n, uniq = c.split("\t")
        assert name == api._first_token(t[0]).decode() and int(length) == len(t[1])
        mine = [r for r in placed if r[1] == name]
        assert int(n) == len(mine) and int(uniq) == sum(float(r[4]) < 0 for r in mine)
    assert sum(int(c.split("\t")[2]) for c in clines[1:-1]) == len(placed)


def test_a_sample_of_the_reads_against_the_oracle(oracle, runs):
    fq, reads, targets, out = runs
    sample = np.sort(np.random.default_rng(150).choice(N_READS, N_SAMPLE, replace=False))
    seqs = [t[1] for t in targets] + [reads[i][1] for i in sample]
    nt = len(targets)
    want = assign_ref.brute_force(Ref(oracle, seqs, 10, False), np.arange(nt), np.arange(nt, len(seqs)), 0.4)
    rows = [l.split("\t") for l in (out["plain"] / "assignments.tsv").read_text().split("\n")[1:-1]]
    names = [api._first_token(t[0]).decode() for t in targets]
    assert (want["target"] >= 0).sum() >= 10
    for q, i in enumerate(sample):
        t = int(want["target"][q])
        exp = [names[t] if t >= 0 else "*", "*" if t < 0 else "-" if want["rev"][q] else "+", "%.17g" % want["score"][q],
               "%.17g" % want["second_score"][q], str(want["n_accepted"][q]), str(want["bases"][q]), str(want["hc_bases"][q]),
               str(want["min_len"][q]), "%.17g" % want["variance"][q]]
        assert rows[i][1:] == exp, (int(i), rows[i], exp)


def test_several_devices_are_refused(runs, tmp_path):
    fq, _, _, _ = runs
    r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", os.path.join(GOLDEN, "toyset_rna.transcriptome.fq.gz"), "-o", str(tmp_path),
                        "--devices", "0,1"], capture_output=True, text=True)
    assert r.returncode != 0 and "--devices" in r.stderr
    assert os.listdir(tmp_path) == []
