"""Kernel C, barrier form, 1536-column class: the row loop's ring of six rows lies over the front of the workgroup's LDS (the sequence's copy,
the graph walks' bitmaps and their stack; dp_rows_v3 with FRONT rows, poa.hip).  Every case runs under RATTLE_POA_MODE=dense, so that the
barrier form runs whatever the device's load, and compares the MSA bytes with the oracle's.

What can go wrong, and the case that meets it:
  * a row served from the wrong slot, or from a slot already overwritten, at the ring's old length (4), at its new one (6) or at its wrap:
    ladders and fans with distances on both sides of both, with the front padded (longest read just over 1024) and at its own size (1536);
  * a sequence copy that is stale or partly overwritten when the traceback tests its letters: reads that differ from the graph only beyond
    column 1024 and in their last 16 columns;
  * a wavefront that only counts the row barriers and misses the one behind the prologue: short reads (three, then two counting
    wavefronts) among long ones, several alignments per pack, so that the front is used again after the traceback had its tables there;
  * another front size: the retry pass with four times the nodes (larger bitmaps);
  * a distance byte that is saturated: the row then comes from the full plan, not from row - 255."""
import re

import numpy as np
import pytest

import constructed_graphs as cg
from test_gpu_poa_variants import _group_of, _lines, _want

pytestmark = pytest.mark.gpu

_BLOCKS = re.compile(r"poa class [^\n]*? (\d+) blocks/CU, group (\d+) ")


def _run_dense(gpu_ctx, oracle, capfd, monkeypatch, packs, env=None):
    """one call of the MSA entry in the barrier form: every pack's rows == the oracle's; returns the timing lines of group 1, each with its
    workgroups per CU"""
    monkeypatch.setenv("RATTLE_TIMING", "1")
    monkeypatch.setenv("RATTLE_POA_MODE", "dense")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    for p in packs:
        assert _group_of(p) == 1, [len(s) for s in p][:4]
    capfd.readouterr()
    rows, width, counters = gpu_ctx.poa_msa(packs)
    err = capfd.readouterr().err
    cells = 0
    for p, pack in enumerate(packs):
        want, c = _want(oracle, pack)
        cells += c
        assert width[p] == len(want[0]), p
        assert rows[p] == want, p
    assert int(counters[0]) == cells
    lines = [d for d in _lines(err) if d["group"] == 1]
    bpc = [int(b) for b, g in _BLOCKS.findall(err) if int(g) == 1]
    assert lines and len(bpc) == len(lines), err[-2000:]
    for d, b in zip(lines, bpc):
        d["bpc"] = b
        assert d["variant"] == (6, 4, 4, 1), d                  # the instance keeps its name: its ring argument still reads 4
    return lines


def _fan_at(m, s, L):
    """fan(m, s) on a backbone of exactly L bases"""
    pack, c = cg.fan(m, s, head=L - 200 - m * s)
    assert max(map(len, pack)) == L
    return pack


@pytest.mark.parametrize("L", [1060, 1536])
def test_distances_on_both_sides_of_both_ring_lengths(gpu_ctx, oracle, capfd, monkeypatch, L):
    """The ladder has every distance 2 .. 26, the fans 1 + 2 i and 1 + 3 i: 4, 5 (the instance's ring argument), 6, 7 (the rows it keeps) and
    the wrap behind them.  1060 columns: the front is padded up to the two extra rows; 1536: every thread of the row is in use.  Default
    capacities: eight workgroups per CU, as with a ring of four rows."""
    assert {4, 5, 6, 7} <= set(cg.LADDER_DISTANCES) and {5, 7} <= set(cg.fan_distances(9, 2)) and {4, 7} <= set(cg.fan_distances(9, 3))
    packs = [cg.ladder(1, 25, L), _fan_at(9, 2, L), _fan_at(16, 2, L), _fan_at(9, 3, L)]
    assert all(max(map(len, p)) == L for p in packs)
    lines = _run_dense(gpu_ctx, oracle, capfd, monkeypatch, packs)
    first = [d for d in lines if d["pass"] == 0]
    assert first and all(d["ring"] == 4 and d["bpc"] == 8 for d in first), first


def _tail_edits(L, seed):
    """B, then reads that are B but for ONE edit each: a mismatch, a deletion, an insertion beyond column 1024, and the same in the last 16
    columns; then B again.  An alignment whose traceback tests a letter of a stale sequence copy puts the edit elsewhere (or nowhere)."""
    rng = np.random.default_rng(seed)
    B = cg.backbone(seed, L)
    for a in range(1, L):                                       # no two equal neighbours: an indel has one place to go
        if B[a] == B[a - 1]:
            B[a] = cg._other(rng, B[a - 1])
    reads = [B.tobytes()]
    for at in (1030, 1100, 1290, L - 14, L - 9, L - 3):
        sub = B.copy()
        sub[at] = cg._other(rng, B[at])
        reads.append(sub.tobytes())
        reads.append(np.delete(B, at).tobytes())
        ins = cg._other(rng, B[at])
        if ins == B[at - 1]:
            ins = [c for c in cg.ACGT if c != B[at] and c != B[at - 1]][0]
        reads.append(np.insert(B, at, ins).tobytes())
    return reads + [B.tobytes()]


@pytest.mark.parametrize("L", [1300, 1535])
def test_the_sequence_copy_is_restored_behind_the_rows(gpu_ctx, oracle, capfd, monkeypatch, L):
    """Twenty sequences that differ from the graph only beyond column 1024 and in their last 16 columns (1535 + an insertion: the last
    column of the class).  With the test's small capacities the ring begins where the sequence copy begins: all of it is overwritten by the
    rows, and the traceback's letter tests read what was copied in again."""
    pack = _tail_edits(L, 11 + L)
    assert len(pack) == 20 and max(map(len, pack)) == L + 1 <= 1536
    _run_dense(gpu_ctx, oracle, capfd, monkeypatch, [pack])


def _mixed_lengths(seed):
    """reads of 1300 nt at 4 % substitutions and indels, among them pieces of the backbone of 350 nt (one wavefront runs the rows, three only
    count the barriers) and 700 nt (two and two), each followed by long reads again"""
    rng = np.random.default_rng(seed)
    B = cg.backbone(seed, 1300)

    def noisy(a):
        keep = rng.random(len(a)) >= 0.012
        a = a[keep].copy()
        sub = rng.random(len(a)) < 0.016
        a[sub] = cg.ACGT[rng.integers(0, 4, int(sub.sum()))]
        pos = np.sort(rng.integers(0, len(a) + 1, int(0.012 * len(a))))
        return np.insert(a, pos, cg.ACGT[rng.integers(0, 4, len(pos))])

    pack = [B.tobytes(), noisy(B).tobytes(), noisy(B[400:750]).tobytes(), noisy(B).tobytes(), noisy(B[300:1000]).tobytes(), noisy(B).tobytes(),
            noisy(B[900:1250]).tobytes(), noisy(B[600:1300]).tobytes(), noisy(B).tobytes(), B.tobytes()]
    lens = [len(s) for s in pack]
    assert sum(n <= 384 for n in lens) == 2 and sum(384 < n <= 768 for n in lens) == 2 and max(lens) > 1024
    return pack


def test_wavefronts_that_only_count_barriers(gpu_ctx, oracle, capfd, monkeypatch):
    """ten alignments per pack, short and long reads in turn: the barrier between the prologue and the first ring write is counted by the
    wavefronts without columns too, and the front serves the rows again after the traceback and the graph update have used it"""
    _run_dense(gpu_ctx, oracle, capfd, monkeypatch, [_mixed_lengths(3), _mixed_lengths(4)])


def test_retry_pass_with_larger_bitmaps(gpu_ctx, oracle, capfd, monkeypatch):
    """RATTLE_POA_NODE_CAP=512: the ladder's graph (1300 nodes and more) does not fit, the pack runs again with four times the nodes --
    other bitmaps, another pad in front of the same ring, the same rows"""
    lines = _run_dense(gpu_ctx, oracle, capfd, monkeypatch, [cg.ladder(1, 25, 1300), _fan_at(9, 2, 1400)], {"RATTLE_POA_NODE_CAP": "512"})
    assert max(d["pass"] for d in lines) >= 1, lines
    assert all(d["ring"] == 4 for d in lines), lines


def test_saturated_distance_byte(gpu_ctx, oracle, capfd, monkeypatch):
    """in-edges 254 .. 257 rows back (far ladders: the byte is exact up to 254 and saturated from 255 on) and the fan with three in-edges
    beyond the distance byte (281, 321 and 361 rows back): a saturated byte is no distance, the row comes from the full plan"""
    assert [d for d in cg.fan_distances(9, 40) if d >= 255] == [281, 321, 361]
    packs = [cg.far_ladder(D, 1300) for D in cg.FAR_DS] + [cg.class_fan(9, 40, 1)[0]]
    _run_dense(gpu_ctx, oracle, capfd, monkeypatch, packs)
