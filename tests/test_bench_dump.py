"""bench.py --dump-outputs: what the timed path returned, as float32 / float64 .npy files that hold the integers exactly, within 64 MB."""
import ctypes as C
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rattle_amd import _lib  # noqa: E402
from rattle_amd.api import Clusters, CorrectionHandle  # noqa: E402


def _readset(recs, keep):
    seq = b"".join(r[3] for r in recs)
    qual = b"".join(r[4] for r in recs)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r[3]) for r in recs])
    cols = [np.array([r[i] for r in recs] or [0], np.int32) for i in range(3)]
    sb, qb = C.create_string_buffer(seq, max(len(seq), 1)), C.create_string_buffer(qual, max(len(qual), 1))
    keep += cols + [off, sb, qb]
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    return _lib.ReadSet(len(recs), p32(cols[0]), p32(cols[1]), p32(cols[2]), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                        C.cast(sb, C.POINTER(C.c_char)), C.cast(qb, C.POINTER(C.c_char)))


def _fixture(n_reads, rng):
    keep = []
    recs = {}
    for name, n in (("corrected", n_reads - n_reads // 10), ("uncorrected", n_reads // 10), ("consensi", 37)):
        recs[name] = [(int(rng.integers(0, 1 << 30)), int(rng.integers(0, 5000)), int(rng.integers(1, 200)),
                       bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, 50)))), bytes(rng.integers(33, 74, 0, np.uint8)))
                      for _ in range(n)]
        recs[name] = [(a, b, c, s, bytes(rng.integers(33, 74, len(s), np.uint8))) for a, b, c, s, _ in recs[name]]
    R = _lib.Correction()
    R.corrected, R.uncorrected, R.consensi = (_readset(recs[k], keep) for k in ("corrected", "uncorrected", "consensi"))
    R_ptr = C.pointer(R)
    keep.append(R)
    cl = Clusters(np.arange(0, n_reads, 7, dtype=np.int32), np.zeros(-(-n_reads // 7), np.uint8), np.arange(0, n_reads + 7, 7).clip(0, n_reads).astype(np.uint32)[:-(-n_reads // 7) + 1],
                  rng.permutation(n_reads).astype(np.int32), rng.integers(0, 2, n_reads).astype(np.uint8), np.zeros(8, np.uint64))
    return cl, CorrectionHandle(None, R_ptr), recs, keep


def test_dump_is_exact_and_complete(tmp_path):
    rng = np.random.default_rng(3)
    cl, h, recs, keep = _fixture(3000, rng)
    bench.dump_outputs(str(tmp_path), cl, h)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["clusters_member_id"], cl.member_id) and np.array_equal(got["clusters_offsets"], cl.offsets)
    for name, rs in recs.items():
        assert np.array_equal(got[name + "_read_id"], [r[0] for r in rs]) and np.array_equal(got[name + "_n_reads"], [r[2] for r in rs])
        assert np.array_equal(got[name + "_seq_crc32"], [zlib.crc32(r[3]) for r in rs])
        assert np.array_equal(got[name + "_qual_crc32"], [zlib.crc32(r[4]) for r in rs])
        idx = got[name + "_sample_index"].astype(np.int64)
        assert bytes(got[name + "_sample_seq"].astype(np.uint8)) == b"".join(rs[i][3] for i in idx)
    assert "corrected_index" not in got


def test_dump_is_sampled_within_the_limit(tmp_path):
    rng = np.random.default_rng(4)
    cl, h, recs, keep = _fixture(20000, rng)
    bench.dump_outputs(str(tmp_path / "a"), cl, h, limit=200_000)
    bench.dump_outputs(str(tmp_path / "b"), cl, h, limit=200_000)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 200_000 + 128 * len(files)
    idx = np.load(tmp_path / "a" / "corrected_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "corrected_read_id.npy"), [recs["corrected"][i][0] for i in idx])
    for f in files:                                                   # a fixed sample: the same files from run to run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
