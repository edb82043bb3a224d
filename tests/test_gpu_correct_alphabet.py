"""Whole `correct` on reads written with U and clustered on both strands, against the oracle and the oracle CLI, byte for byte.

`correct` takes A, C, G, T and U and reverse-complements the members marked `rev` with the reference's complement, where U -> A and
A -> T.  Reads written with U and clustered without `--rna` therefore give packs whose forward members hold U where the reversed ones hold
T: POA #1 aligns T against U (a mismatch, as in the reference), kernel D votes with real counts in its T and its U slot, the corrected
reads and the consensi hold both letters, and so POA #2 and POA #3 see mixed packs too."""
import os
import subprocess

import pytest

from rattle_amd import hps, synth
from rattle_amd.api import correct_command
from test_gpu_cli import ORACLE, RATTLE

pytestmark = pytest.mark.gpu

SPLIT, MIN_READS = 25, 5


@pytest.fixture(scope="module")
def built(oracle):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    assert os.path.exists(ORACLE)


@pytest.fixture(scope="module")
def job():
    """120 reads of two transcripts on both strands, T written as U, longest first; one cluster per transcript, a member's `rev` flag its
    strand against the first member's"""
    seqs, quals, tid, strand = synth.reads(120, 2, 1, True, seed=3)
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))
    seqs = [seqs[i].replace(b"T", b"U") for i in order]
    quals = [quals[i] for i in order]
    tid, strand = [int(tid[i]) for i in order], [int(strand[i]) for i in order]
    clusters = []
    for g in sorted(set(tid), key=tid.index):
        ids = [i for i in range(len(seqs)) if tid[i] == g]
        mem = [(i, strand[i] ^ strand[ids[0]], -1) for i in ids]
        clusters.append((mem[0], mem))
    headers = [b"@u%d" % i for i in range(len(seqs))]
    return headers, seqs, quals, clusters


@pytest.fixture(scope="module")
def want(oracle, job):
    headers, seqs, quals, clusters = job
    return oracle.correct(headers, seqs, quals, hps.encode(clusters), split=SPLIT)


def _seqs_of(fastq):
    return fastq.split(b"\n")[1::4]


def test_the_job_is_what_it_claims(job, want):
    """on the oracle's output: both consensi hold T and U, more than half of the corrected reads hold both, and every queued pack has
    members of both strands"""
    headers, seqs, quals, clusters = job
    assert not any(b"T" in s for s in seqs) and all(b"U" in s for s in seqs)
    assert sorted((len(mem), sum(r for _, r, _ in mem)) for _, mem in clusters) == [(35, 22), (85, 43)]
    for _, mem in clusters:
        nf = (len(mem) - 1) // SPLIT + 1                           # correct.cpp:331-360: strided sub-packs, queued if > min_reads
        for j in range(nf):
            pack = mem[j::nf]
            assert len(pack) > MIN_READS and {r for _, r, _ in pack} == {0, 1}, (j, pack)
    cons = _seqs_of(want[2])
    assert len(cons) == 2 and all(c.count(b"T") >= 10 and c.count(b"U") >= 100 for c in cons), [(c.count(b"T"), c.count(b"U")) for c in cons]
    cor = _seqs_of(want[0])
    assert len(cor) > 100 and 2 * sum(b"T" in s and b"U" in s for s in cor) > len(cor)


@pytest.mark.parametrize("mode", [None, "dense"])
def test_correct_on_u_reads_of_both_strands_matches_oracle(gpu_ctx, job, want, monkeypatch, mode):
    headers, seqs, quals, clusters = job
    if mode:
        monkeypatch.setenv("RATTLE_POA_MODE", mode)
    got = correct_command(gpu_ctx, headers, seqs, quals, clusters, split=SPLIT)
    assert got[0] == want[0], "corrected.fq differs"
    assert got[1] == want[1], "uncorrected.fq differs"
    assert got[2] == want[2], "consensi.fq differs"
    assert int(got[3][0]) == int(want[3][0])                       # DP cells, exact


def test_cluster_and_correct_cli_on_u_reads_match_oracle_cli(built, job, tmp_path):
    """the same reads as a FASTQ through `rattle cluster` without --rna (both strands) and `rattle correct`: nothing on the way refuses
    or rewrites U; clusters.out and the three FASTQ files are the oracle CLI's"""
    _, seqs, quals, _ = job
    fq = tmp_path / "u.fastq"
    fq.write_bytes(synth.fastq_text(seqs, quals))
    a = tmp_path / "a"; b = tmp_path / "b"
    a.mkdir(); b.mkdir()
    for tool, out in ((RATTLE, a), (ORACLE, b)):
        subprocess.run([tool, "cluster", "-i", str(fq), "-o", str(out)], check=True, capture_output=True)
    assert (a / "clusters.out").read_bytes() == (b / "clusters.out").read_bytes()
    clusters = hps.decode((a / "clusters.out").read_bytes(), fields=3)
    assert any(len(mem) > MIN_READS and {s[1] for s in mem} == {0, 1} for _, mem in clusters)      # a cluster to correct, on both strands
    for tool, out in ((RATTLE, a), (ORACLE, b)):
        subprocess.run([tool, "correct", "-i", str(fq), "-c", str(out / "clusters.out"), "-o", str(out), "-s", str(SPLIT)], check=True, capture_output=True)
    for f in ("corrected.fq", "uncorrected.fq", "consensi.fq"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    cons = _seqs_of((a / "consensi.fq").read_bytes())
    assert cons and any(b"T" in c and b"U" in c for c in cons)
    assert b"U" in (a / "corrected.fq").read_bytes()
