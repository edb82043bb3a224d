"""`rattle correct --report` on the toyset fixture: correction_report.tsv has one line per record of corrected.fq, in that file's
order, and no other output file changes by a byte -- on one device and as one job over two ranks."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
COLUMNS = ["read", "cluster", "in_len", "out_len", "trim_front", "trim_back", "match", "substituted", "mismatch_kept", "inserted", "deleted", "gap_kept"]
FILES = ("corrected.fq", "uncorrected.fq", "consensi.fq")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_report")
    fq = tmp / "sample.fastq"
    fq.write_bytes(gzip.open(os.path.join(GOLDEN, "toyset_rna.fastq.gz")).read())
    out = {}
    for name, extra in (("plain", []), ("report", ["--report"]), ("sharded", ["--report", "--devices", "0,0", "--host-exchange"])):
        out[name] = tmp / name
        out[name].mkdir()
        subprocess.run([RATTLE, "correct", "-i", str(fq), "-c", os.path.join(GOLDEN, "toyset_rna.clusters.out"), "-o", str(out[name])] + extra,
                       check=True, capture_output=True)
    return fq, out


def test_the_other_outputs_do_not_change(runs):
    _, out = runs
    for f in FILES:
        want = (out["plain"] / f).read_bytes()
        assert len(want) > 1000 and (out["report"] / f).read_bytes() == want and (out["sharded"] / f).read_bytes() == want, f
    assert not (out["plain"] / "correction_report.tsv").exists()
    assert sorted(os.listdir(out["report"])) == sorted(os.listdir(out["plain"]) + ["correction_report.tsv"])


def test_the_report_follows_corrected_fq(runs):
    fq, out = runs
    lines = (out["report"] / "correction_report.tsv").read_text().split("\n")
    assert lines[0].split("\t") == COLUMNS and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    cor = (out["report"] / "corrected.fq").read_text().split("\n")
    heads, seqs = cor[0:-1:4], cor[1:-1:4]
    assert len(rows) == len(heads) > 7000 and all(len(r) == len(COLUMNS) for r in rows)
    # the id is the first token of the read's input header; corrected.fq appends ",gene_cluster_<cluster>" to that header
    in_len = {}
    text = fq.read_text().split("\n")
    for h, s in zip(text[0:-1:4], text[1:-1:4]):
        in_len[h.split()[0][1:]] = len(s)
    assert len(in_len) == 8306
    for r, h, s in zip(rows, heads, seqs):
        assert h.startswith("@" + r[0]) and h.endswith(",gene_cluster_" + r[1]), (r, h)
        n = [int(x) for x in r[2:]]
        assert n[1] == len(s) and n[0] == in_len[r[0]], (r, h)
        assert n[1] == n[4] + n[5] + n[6] + n[7] + n[9] and n[0] == n[2] + n[3] + n[4] + n[5] + n[6] + n[8] + n[9], r
    assert (out["sharded"] / "correction_report.tsv").read_bytes() == (out["report"] / "correction_report.tsv").read_bytes()
