"""Three branches of the CLI that no other test runs: `rattle polish` on transcript-level consensi (the `gene_map` branch, against
the oracle CLI), `rattle polish -l s1,s2 --summary` (polish_summary.tsv and the sums in the rewritten headers, derived from the
test's own input), and the names that `cluster --report` / `correct --report` take from FASTA headers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from rattle_amd import hps, synth

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
ORACLE = os.path.join(ROOT, "oracle", "oracle_cli")
N = 40


@pytest.fixture(scope="module")
def consensi(oracle):
    """near-duplicate sequences that DO cluster, as in test_gpu_cli.test_polish_cli_merges_similar_consensi"""
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    assert os.path.exists(ORACLE)
    seqs, _, _, _ = synth.reads(N, 3, 1, True, seed=23, sub=0.01, ins=0.005, dele=0.005)
    return seqs


def label_counts(i):
    return i % 5 + 1, (7 * i) % 4


def header(i, transcript, labels):
    name = b"@transcript_cluster_%d gene_cluster_%d" % (i, i // 4) if transcript else b"@gene_cluster_%d" % i
    lab = b"s1:%d,s2:%d," % label_counts(i) if labels else b""
    return name + b" reads=%d labels=%s" % (6 + i, lab)


def fastq(seqs, transcript, labels):
    return b"".join(b"%s\n%s\n+\n%s\n" % (header(i, transcript, labels), s, b"K" * len(s)) for i, s in enumerate(seqs))


def test_polish_transcript_level_consensi_match_oracle_cli(consensi, tmp_path):
    (tmp_path / "c.fq").write_bytes(fastq(consensi, True, False))
    a = tmp_path / "a"; b = tmp_path / "b"
    a.mkdir(); b.mkdir()
    subprocess.run([RATTLE, "polish", "-i", str(tmp_path / "c.fq"), "-o", str(a)], check=True, capture_output=True)
    subprocess.run([ORACLE, "polish", "-i", str(tmp_path / "c.fq"), "-o", str(b)], check=True, capture_output=True)
    got = (a / "transcriptome.fq").read_bytes()
    assert got == (b / "transcriptome.fq").read_bytes()
    heads = got.split(b"\n")[0:-1:4]
    assert 1 <= len(heads) < N and all(h.startswith(b"@transcript_cluster_") for h in heads)
    assert all(re.fullmatch(rb"@transcript_cluster_\d+ gene_cluster_\d+ generated_from_transcript_clusters=\d+ total_reads=\d+ labels=", h) for h in heads)
    assert any(int(re.search(rb"generated_from_transcript_clusters=(\d+)", h).group(1)) > 1 for h in heads)
    assert sorted(os.listdir(a)) == ["transcriptome.fq"]


@pytest.mark.parametrize("transcript", [True, False], ids=["transcript", "gene"])
def test_polish_summary_and_label_sums(consensi, tmp_path, transcript):
    (tmp_path / "c.fq").write_bytes(fastq(consensi, transcript, True))
    subprocess.run([RATTLE, "polish", "-i", str(tmp_path / "c.fq"), "-o", str(tmp_path), "-l", "s1,s2", "--summary"], check=True, capture_output=True)
    text = (tmp_path / "polish_summary.tsv").read_text()
    assert text.endswith("\n")
    lines = text.split("\n")[:-1]
    assert len(lines) == N
    members = {}                                                   # new cluster -> the inputs it was made from
    for l in lines:
        if transcript:
            m = re.fullmatch(r"transcript_cluster_(\d+), gene_cluster_(\d+), new_cluster_(\d+)", l)
            assert m and int(m.group(2)) == int(m.group(1)) // 4, l
        else:
            m = re.fullmatch(r"gene_cluster_(\d+), new_cluster_(\d+)", l)
            assert m, l
        members.setdefault(int(m.groups()[-1]), []).append(int(m.group(1)))
    assert sorted(i for v in members.values() for i in v) == list(range(N))
    heads = (tmp_path / "transcriptome.fq").read_text().split("\n")[0:-1:4]
    assert sorted(members) == list(range(len(heads))) and 1 <= len(heads) < N
    gene_map = {}                                                  # the reference's rule for a new record's gene (main.cpp:690-755)
    for c, h in enumerate(heads):
        if transcript:
            gene = -1
            for i in members[c]:                                       # the summary lists a cluster's inputs in member order
                if i // 4 not in gene_map:
                    gene = i // 4 if gene == -1 else gene
                    gene_map[i // 4] = gene
                else:
                    gene = gene_map[i // 4]
            m = re.fullmatch(r"@transcript_cluster_(\d+) gene_cluster_(\d+) generated_from_transcript_clusters=(\d+) total_reads=(\d+) labels=s1:(\d+),s2:(\d+),", h)
            assert m and int(m.group(2)) == gene, h
        else:
            m = re.fullmatch(r"@cluster_(\d+) generated_from_consensi_clusters=(\d+) total_reads=(\d+) labels=s1:(\d+),s2:(\d+),", h)
            assert m, h
        made_from, total, s1, s2 = (int(x) for x in m.groups()[-4:])
        assert int(m.group(1)) == c
        assert made_from == len(members[c]), h
        assert total == sum(6 + i for i in members[c]), h
        assert (s1, s2) == (sum(label_counts(i)[0] for i in members[c]), sum(label_counts(i)[1] for i in members[c])), h
    assert any(len(v) > 1 for v in members.values())


def test_report_names_from_fasta_headers(consensi, tmp_path):
    """the FASTA input of test_gpu_cli.test_fasta_input_matches_oracle_cli: headers `>f<i> some text`"""
    seqs, _, _, _ = synth.reads(260, 3, 1, True, seed=37)
    lines = []
    for i, s in enumerate(seqs[:160]):
        if i == 4:
            s = s[:30] + b"N" + s[31:]
        if i == 7:
            s = s[:90]
        if i % 3 == 0:
            s = s.lower()
        lines.append(b">f%d some text\n" % i)
        lines += [s[p:p + 70] + b"\n" for p in range(0, len(s), 70)]
    fa = tmp_path / "x.fasta"
    fa.write_bytes(b"".join(lines))
    subprocess.run([RATTLE, "cluster", "-i", str(fa), "-o", str(tmp_path), "--report"], check=True, capture_output=True)
    clusters = hps.decode((tmp_path / "clusters.out").read_bytes(), fields=3)
    cluster_of = {"f%d" % m[0]: c for c, (_, ms) in enumerate(clusters) for m in ms}
    assert len(cluster_of) == 158 and "f4" not in cluster_of and "f7" not in cluster_of
    rows = [l.split("\t") for l in (tmp_path / "cluster_report.tsv").read_text().split("\n")[1:-1]]
    assert len(rows) == len(cluster_of) - len(clusters) > 100
    for r in rows:
        assert re.fullmatch(r"f\d+", r[3]) and re.fullmatch(r"f\d+", r[4]), r
        assert cluster_of[r[3]] == cluster_of[r[4]], r             # a join: both ends up in one cluster of clusters.out
    assert len({r[3] for r in rows}) == len(rows)                  # every read is absorbed once

    subprocess.run([RATTLE, "correct", "-i", str(fa), "-c", str(tmp_path / "clusters.out"), "-o", str(tmp_path), "-s", "60", "--report"],
                   check=True, capture_output=True)
    cor = (tmp_path / "corrected.fq").read_text().split("\n")
    heads = cor[0:-1:4]
    rows = [l.split("\t") for l in (tmp_path / "correction_report.tsv").read_text().split("\n")[1:-1]]
    assert len(rows) == len(heads) > 100
    for r, h in zip(rows, heads):
        assert re.fullmatch(r"f\d+", r[0]), r
        assert h == ">%s some text,gene_cluster_%s" % (r[0], r[1]), (r, h)
        assert cluster_of[r[0]] == int(r[1]), r
