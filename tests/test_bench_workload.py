"""bench.py draws its workload segment by segment on several cores from recorded states of the random stream: the result must be
synth.reads_packed's to the byte, and a stale record must fall back to drawing in one piece."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _same(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_segments_equal_reads_packed(tmp_path, monkeypatch):
    n, genes, seed = 37_000, 185, 20260929                 # 74 chunks: three segments, the last one short
    states = bench.record_workload_states(n, genes, seed)
    assert len(states) == 4
    path = tmp_path / "states.json"
    path.write_text(json.dumps({bench._workload_key(n, genes, seed, 1): states}))
    monkeypatch.setattr(bench, "STATES_FILE", str(path))
    _same(bench.make_workload_fast(n, genes, seed, workers=3), bench.make_workload(n, genes, seed))


def test_stale_states_fall_back(tmp_path, monkeypatch, capsys):
    n, genes, seed = 20_000, 100, 7
    states = bench.record_workload_states(n, genes, seed)
    states[1] = states[2]                                   # a segment that cannot end where the record says
    path = tmp_path / "states.json"
    path.write_text(json.dumps({bench._workload_key(n, genes, seed, 1): states}))
    monkeypatch.setattr(bench, "STATES_FILE", str(path))
    _same(bench.make_workload_fast(n, genes, seed, workers=2), bench.make_workload(n, genes, seed))
    assert "did not end in its recorded state" in capsys.readouterr().err


def test_recorded_states_match_the_prelude():
    """the committed record describes the bench's default workload as this tree draws it (its first state: the prelude's)"""
    rec = json.load(open(bench.STATES_FILE))
    key = bench._workload_key(1000000, 5000, 20260929, 1)
    assert key in rec and len(rec[key]) == 1000000 // 500 // bench.SEGMENT_CHUNKS + 2
    _, _, _, rng = bench._prelude(1000000, 5000, 20260929, 1)
    assert rng.bit_generator.state == rec[key][0]
