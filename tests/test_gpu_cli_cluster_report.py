"""`rattle cluster --report`: cluster_report.tsv beside clusters.out has one line per join, in the library's order and with the
library's numbers (doubles printed with %.17g: compared exactly), with and without --iso; it does not depend on the seed batch
(RATTLE_SEED_BATCH=7: other rounds, other levels, the same joins); clusters.out does not change by a byte; without the flag no
file is written; and the flag refuses a job over several devices."""
import os
import subprocess

import pytest

from conftest import ROOT
from rattle_amd import synth
from rattle_amd.api import cluster_command

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
COLUMNS = ["level", "pass", "bv_threshold", "absorbed", "into", "strand", "bases", "hc_bases", "min_len", "score", "variance"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_cluster_report")
    seqs, quals, _, _ = synth.reads(300, 7, 3, True, seed=5, exon=(65, 115))
    fq = tmp / "sample.fastq"
    fq.write_bytes(synth.fastq_text(seqs, quals))
    out = {}
    for name, extra, env in (("plain", [], {}), ("report", ["--report"], {}), ("batch7", ["--report"], {"RATTLE_SEED_BATCH": "7"}),
                             ("iso_plain", ["--iso"], {}), ("iso_report", ["--iso", "--report"], {}),
                             ("iso_batch7", ["--iso", "--report"], {"RATTLE_SEED_BATCH": "7"})):
        out[name] = tmp / name
        out[name].mkdir()
        subprocess.run([RATTLE, "cluster", "-i", str(fq), "-o", str(out[name])] + extra, check=True, capture_output=True,
                       env=dict(os.environ, **env))
    return fq, seqs, out


def rows_of(path):
    lines = path.read_text().split("\n")
    assert lines[0].split("\t") == COLUMNS and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert all(len(r) == len(COLUMNS) for r in rows)
    return rows


def n_clusters(path):
    from rattle_amd import hps
    return len(hps.decode(path.read_bytes(), fields=3))


@pytest.mark.parametrize("iso", [False, True], ids=["gene", "iso"])
def test_the_report_is_the_librarys(gpu_ctx, runs, iso):
    fq, seqs, out = runs
    pre = "iso_" if iso else ""
    want = (out[pre + "plain"] / "clusters.out").read_bytes()
    assert len(want) > 100 and (out[pre + "report"] / "clusters.out").read_bytes() == want
    assert (out[pre + "batch7"] / "clusters.out").read_bytes() == want
    assert os.listdir(out[pre + "plain"]) == ["clusters.out"]
    assert sorted(os.listdir(out[pre + "report"])) == ["cluster_report.tsv", "clusters.out"]
    rows = rows_of(out[pre + "report"] / "cluster_report.tsv")
    clusters, _, rep = cluster_command(gpu_ctx, seqs, list(range(len(seqs))), iso=iso, report=True)
    assert not gpu_ctx.cluster_report
    n = len(seqs)
    assert n_clusters(out[pre + "report"] / "clusters.out") == len(clusters)
    if iso:
        genes = len({c[0][2] for c in clusters})
        assert len(rows) == len(rep["into"]) == (n - genes) + (n - len(clusters))
        assert [r[0] for r in rows] == ["0"] * (n - genes) + ["1"] * (n - len(clusters))
    else:
        assert len(rows) == len(rep["into"]) == n - len(clusters) and set(r[0] for r in rows) == {"0"}
    assert any(int(r[1]) >= 1 for r in rows)
    for q, r in enumerate(rows):
        got = (int(r[0]), int(r[1]), float(r[2]), r[3], r[4], r[5], int(r[6]), int(r[7]), int(r[8]), float(r[9]), float(r[10]))
        lib = (int(rep["level"][q]), int(rep["pass"][q]), float(rep["bv_threshold"][q]), "r%d" % rep["absorbed"][q], "r%d" % rep["into"][q],
               "-" if rep["rev"][q] else "+", int(rep["bases"][q]), int(rep["hc_bases"][q]), int(rep["min_len"][q]), float(rep["score"][q]),
               float(rep["variance"][q]))
        assert got == lib, (q, got, lib)
        assert r[9] == "%.17g" % rep["score"][q] and r[10] == "%.17g" % rep["variance"][q] and r[2] == "%.17g" % rep["bv_threshold"][q]
    # the seed batch changes the rounds and the level a join is found at, not the joins
    assert (out[pre + "batch7"] / "cluster_report.tsv").read_bytes() == (out[pre + "report"] / "cluster_report.tsv").read_bytes()


def test_report_refuses_several_devices(runs, tmp_path):
    fq, _, _ = runs
    r = subprocess.run([RATTLE, "cluster", "-i", str(fq), "-o", str(tmp_path), "--report", "--devices", "0,0"], capture_output=True, text=True)
    assert r.returncode != 0 and "--report cannot be combined with --devices" in r.stderr
    assert os.listdir(tmp_path) == []


def test_help_names_the_flag():
    r = subprocess.run([RATTLE, "cluster", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--report" in r.stderr and "cluster_report.tsv" in r.stderr
