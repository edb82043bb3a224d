"""The ranked PAF of `assign --paf --secondary` from the Python path (api.assign_paf_command(secondary=2)) on 60 reads of a family of
16 isoforms, K = 3: every (read, rank) line is the line of a direct align_cigars call on that one (read, target, strand), the plain
Python references agree on a sample of the pairs, the tp:A:P lines without the two tags are the PAF written without secondary, the
candidate table is the candidate list, and the cell cap drops ranks one by one.  Once with the linear default, once with 5,4,8,6."""
import re

import numpy as np
import pytest

import align_affine_ref
import align_ref
import assign_ref
import assign_top_ref
import cigar_ref
from rattle_amd import api, synth
from test_gpu_assign import noisy
from test_gpu_cluster_eval import Ref, revcomp

pytestmark = pytest.mark.gpu
K = 3
TAGS = re.compile(rb"\ttp:A:([PS])\trk:i:(\d)")
CG = re.compile(rb"\tcg:Z:[0-9=XID]+")
_case = {}


def case():
    """4 genes x 4 isoforms of short exons as the targets, 60 noisy reads of them on both strands, one of them with another letter"""
    if not _case:
        rng = np.random.default_rng(5)
        targets = [t.tobytes() for t in synth.transcriptome(4, 4, seed=6, exon=(20, 40))[0]]
        assert len(targets) == 16 and len(set(targets)) == 16
        reads = [noisy(rng, targets[int(rng.integers(0, 16))]) for _ in range(60)]
        reads = [revcomp(s) if i % 3 == 0 else s for i, s in enumerate(reads)]
        reads[7] = reads[7][:20] + b"N" + reads[7][21:]                      # not submitted: no candidate, no line
        _case.update(targets=targets, reads=reads, th=[b">tx%d len=%d" % (i, len(t)) for i, t in enumerate(targets)],
                     rh=[b"@read%d ch=%d" % (i, i % 5) for i in range(60)])
    return _case


def args(c):
    return c["rh"], c["reads"], c["th"], c["targets"]


@pytest.fixture(scope="module")
def cands(gpu_ctx, oracle):
    """the candidate list of the case, checked against the oracle; reads in file order (the unclean one without candidates)"""
    c = case()
    sent = [i for i, s in enumerate(c["reads"]) if not s.translate(None, b"ACGTU")]
    assert len(sent) == 59
    rec, part = gpu_ctx.assign_top(c["targets"], [c["reads"][i] for i in sent], K)
    seqs = c["targets"] + [c["reads"][i] for i in sent]
    acc = assign_ref.accepted_comparisons(Ref(oracle, seqs, 10, True), np.arange(16), np.arange(16, 16 + 59), 0.4, 0.2, 1000000.0)
    assert not assign_top_ref.same(part, assign_top_ref.reduce_top(59, acc, K))
    full = api.unused_candidates(60, K)
    for f in full:
        full[f][sent] = part[f]
    assert (full["count"] == 3).sum() >= 15 and (full["count"] == 0).sum() >= 1 and (full["rev"][:, 1] == 1).sum() >= 5
    return full


def split_lines(paf):
    """{(read, rank): line without the two tags}, and the keys in file order"""
    out, order = {}, []
    for line in paf.split(b"\n")[:-1]:
        m = TAGS.search(line)
        assert m and (m.group(1) == b"P") == (m.group(2) == b"0"), line
        key = (int(line.split(b"\t")[0][4:]), int(m.group(2)))
        assert key not in out
        out[key] = TAGS.sub(b"", line)
        order.append(key)
    return out, order


@pytest.mark.parametrize("scoring", [None, (5, 4, 8, 6)], ids=["linear", "5-4-8-6"])
def test_every_line_is_the_direct_call_on_its_pair(gpu_ctx, cands, scoring):
    c = case()
    tsv, counts, paf, table = api.assign_paf_command(gpu_ctx, *args(c), cigar=True, scoring=scoring, secondary=K - 1)
    rn, tn = [b"read%d" % i for i in range(60)], [b"tx%d" % i for i in range(16)]
    assert table == api.candidates_tsv(rn, tn, cands) and table.count(b"\n") == 1 + int(cands["count"].sum())
    lines, order = split_lines(paf)
    assert order == sorted(order) and len(order) >= 120
    one = api.unassigned_records(1)
    sample = 0
    for r in range(60):
        for j in range(K):
            if j >= cands["count"][r]:
                assert (r, j) not in lines
                continue
            t, rev = int(cands["target"][r, j]), int(cands["rev"][r, j])
            q, x = c["reads"][r], c["targets"][t]
            aln, offsets, ops = gpu_ctx.align_cigars([x], [q], [0], [rev], scoring=scoring)
            one["target"][0], one["rev"][0] = 0, rev
            direct = api.paf_text([rn[r]], [len(q)], [tn[t]], [len(x)], one, aln, (offsets, ops))
            assert aln["status"][0] == 0 and lines[(r, j)] + b"\n" == direct, (r, j)
            plain = gpu_ctx.align_pairs([x], [q], [0], [rev], scoring=scoring)
            assert not align_ref.same(plain, aln)
            if r % 6 == 1 and sample < 10:                            # the plain Python references on a sample of the pairs
                sample += 1
                got = tuple(int(aln[f][0]) for f, _ in align_ref.FIELDS)
                if scoring is None:
                    want, wops = cigar_ref.pair(q, x, rev)
                    assert align_ref.align(q, x, rev) == want
                else:
                    want, wops = align_affine_ref.pair(q, x, rev, scoring)
                assert got == tuple(want) and api.cigar_bytes(ops) == cigar_ref.text(wops), (r, j)
    assert sample == 10
    # without --cigar: the same lines without the tag
    no_cg = api.assign_paf_command(gpu_ctx, *args(c), scoring=scoring, secondary=K - 1)
    assert no_cg[2] == CG.sub(b"", paf) and no_cg[3] == table and CG.search(paf)
    # the tp:A:P lines without the two tags are the PAF of the run without secondary; the two tables do not move
    old = api.assign_paf_command(gpu_ctx, *args(c), cigar=True, scoring=scoring)
    assert len(old) == 3 and (tsv, counts) == old[:2]
    assert b"".join(lines[k] + b"\n" for k in order if k[1] == 0) == old[2] and old[2].count(b"\n") >= 50
    assert api.assign_command(gpu_ctx, *args(c), secondary=K - 1) == (tsv, counts, table)
    assert api.assign_command(gpu_ctx, *args(c)) == (tsv, counts)


def test_the_cell_cap_counts_pairs(gpu_ctx, cands):
    """max_cells between the cells of a read's rank 0 and rank 1: the one within the cap is written, the other is not"""
    c = case()
    cells = lambda r, j: len(c["reads"][r]) * len(c["targets"][int(cands["target"][r, j])])
    two = [r for r in range(60) if cands["count"][r] >= 2]
    up = [r for r in two if cells(r, 1) > cells(r, 0)]
    down = [r for r in two if cells(r, 1) < cells(r, 0)]
    assert up and down
    for r, keep, drop in ((up[0], 0, 1), (down[0], 1, 0)):
        cap = cells(r, keep)
        paf = api.assign_paf_command(gpu_ctx, *args(c), max_cells=cap, secondary=K - 1)[2]
        lines, order = split_lines(paf)
        assert (r, keep) in lines and (r, drop) not in lines
        for (a, j) in [(a, j) for a in range(60) for j in range(int(cands["count"][a]))]:
            assert ((a, j) in lines) == (cells(a, j) <= cap), (a, j)
