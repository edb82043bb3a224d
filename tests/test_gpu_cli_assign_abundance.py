"""`rattle assign --abundance`: the family reads of tests/test_gpu_assign.py through Context.assign_top(8) and Context.abundance against
the rule on the returned list, and the CLI on the golden direct-RNA transcriptome and the first 500 records of its reads, alone and with
--secondary 2 --paf --cigar: abundance.tsv is byte for byte the Python path's, every other file byte for byte that of the run without
the flag.  --abundance-ratio is 0.5 in these runs: at the default 0.95 no read of these 500 has a second compatible transcript (the
best runner-up reaches 0.83 of its winner), at 0.5 ten reads have one and none lies within 0.03 of the bar (worked out with
assign_ref.accepted_comparisons on the oracle) -- the test asserts that it sees shared reads."""
import os
import subprocess

import numpy as np
import pytest

import abundance_ref as ref
from conftest import GOLDEN, ROOT, read_fastq_gz
from rattle_amd import api
from test_gpu_assign import FAMILY_SEED, family_case

pytestmark = pytest.mark.gpu
RATTLE = os.path.join(ROOT, "rattle_amd", "csrc", "rattle")
N_READS = 500
RATIO = 0.5
AB = ["--abundance", "--abundance-ratio", str(RATIO)]
MODES = (("plain", []), ("abundance", AB), ("ranked", ["--secondary", "2", "--paf", "--cigar"]), ("ranked_abundance", AB + ["--secondary", "2", "--paf", "--cigar"]))


def test_the_family_reads(gpu_ctx):
    seqs, T, R = family_case(10, True, FAMILY_SEED[10])
    rec, cands = gpu_ctx.assign_top([seqs[i] for i in T], [seqs[i] for i in R], 8)
    shared = ref.compatible(cands, 0.95).sum(1)
    assert (cands["count"] > 1).sum() >= 20 and (shared > 1).sum() >= 5 and (cands["count"] == 0).sum() >= 20, np.bincount(shared)
    for ratio in (0.95, 0.6):
        got = gpu_ctx.abundance(cands, len(T), ratio=ratio)
        bad = ref.same(got, ref.vector(cands, len(T), ratio=ratio))
        assert bad is None, (ratio, bad)
        assert got["n_placed"] == int((rec["target"] >= 0).sum()) and int(got["units"].sum()) == got["n_placed"] * ref.ONE
    winners = np.bincount(rec["target"][rec["target"] >= 0], minlength=len(T))
    assert (got["est_reads"] != winners).any()


@pytest.fixture(scope="module")
def runs(tmp_path_factory, toyset):
    if not os.path.exists(RATTLE):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.dirname(RATTLE)])
    tmp = tmp_path_factory.mktemp("cli_assign_abundance")
    reads = toyset[:N_READS]
    fq = tmp / "reads.fastq"
    fq.write_bytes(b"".join(b"%s\n%s\n+\n%s\n" % r for r in reads))
    tx = os.path.join(GOLDEN, "toyset_rna.transcriptome.fq.gz")
    out, err = {}, {}
    for name, extra in MODES:
        out[name] = tmp / name
        out[name].mkdir()
        r = subprocess.run([RATTLE, "assign", "-i", str(fq), "-x", tx, "-o", str(out[name]), "--rna"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        err[name] = r.stderr
    return reads, read_fastq_gz(tx), out, err


def test_the_golden_run(gpu_ctx, runs):
    reads, targets, out, err = runs
    args = ([r[0] for r in reads], [r[1] for r in reads], [t[0] for t in targets], [t[1] for t in targets])
    tsv, counts, table = api.assign_command(gpu_ctx, *args, is_rna=True, abundance=True, abundance_ratio=RATIO)
    assert (tsv, counts) == api.assign_command(gpu_ctx, *args, is_rna=True)
    assert sorted(os.listdir(out["plain"])) == ["assignments.tsv", "target_counts.tsv"]
    assert sorted(os.listdir(out["abundance"])) == ["abundance.tsv", "assignments.tsv", "target_counts.tsv"]
    assert sorted(os.listdir(out["ranked"])) == ["alignments.paf", "assignments.tsv", "candidates.tsv", "target_counts.tsv"]
    assert sorted(os.listdir(out["ranked_abundance"])) == ["abundance.tsv", "alignments.paf", "assignments.tsv", "candidates.tsv", "target_counts.tsv"]
    for name in ("abundance", "ranked_abundance"):
        assert (out[name] / "abundance.tsv").read_bytes() == table, name
        assert "abundance: " in err[name] and " iterations" in err[name] and "not converged" not in err[name]
    for name, base in (("abundance", "plain"), ("ranked_abundance", "ranked")):
        for f in os.listdir(out[base]):
            assert (out[name] / f).read_bytes() == (out[base] / f).read_bytes(), (name, f)
    assert (out["plain"] / "assignments.tsv").read_bytes() == tsv and (out["plain"] / "target_counts.tsv").read_bytes() == counts
    want = api.assign_paf_command(gpu_ctx, *args, is_rna=True, cigar=True, secondary=2, abundance=True, abundance_ratio=RATIO)
    assert want == (tsv, counts, (out["ranked"] / "alignments.paf").read_bytes(), (out["ranked"] / "candidates.tsv").read_bytes(), table)
    # the precondition: reads with two compatible slots, so that est_reads is not the winner-takes-all column
    rows = [l.split(b"\t") for l in table.split(b"\n")[1:-1]]
    assert len(rows) == len(targets) and table.split(b"\n")[0] == b"target\tlength\treads\tunique_reads\tcompatible_reads\test_reads\tcpm"
    assert [b"\t".join(r[:4]) for r in rows] == counts.split(b"\n")[1:-1]
    moved = [r for r in rows if float(r[5]) != float(r[2])]
    assert len(moved) >= 2, "no read of the golden run is shared at this ratio"
    assert sum(int(r[4]) for r in rows) > sum(int(r[2]) for r in rows) >= 300
    placed = sum(int(r[2]) for r in rows)
    assert abs(sum(float(r[5]) for r in rows) - placed) < 1e-6 and abs(sum(float(r[6]) for r in rows) - 1e6) < 1e-3
    # ... and the Python path's numbers are the rule's on its own list
    rec, cands = gpu_ctx.assign_top(args[3], args[1], 8, is_rna=True)
    assert (ref.compatible(cands, RATIO).sum(1) >= 2).sum() >= 1 and (ref.compatible(cands, 0.95).sum(1) >= 2).sum() == 0
    model = ref.vector(cands, len(targets), ratio=RATIO)
    assert api.abundance_tsv([api._first_token(h) for h in args[2]], [len(s) for s in args[3]], rec, model) == table
