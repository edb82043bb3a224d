import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def read_fastq_gz(path):
    with gzip.open(path, "rb") as f:
        lines = f.read().split(b"\n")
    recs = []
    for i in range(0, len(lines) - 1, 4):
        recs.append((lines[i], lines[i + 1], lines[i + 3]))
    return recs


@pytest.fixture(scope="session")
def toyset():
    """Recovered toyset/rna input: list of (header, seq, qual) in seq_id order (= length-descending)."""
    return read_fastq_gz(os.path.join(GOLDEN, "toyset_rna.fastq.gz"))


@pytest.fixture(scope="session")
def toyset_clusters():
    from rattle_amd import hps
    return hps.decode(open(os.path.join(GOLDEN, "toyset_rna.clusters.out"), "rb").read(), fields=2)


@pytest.fixture(scope="session")
def oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as orc_mod
    orc_mod.build(ref=True)
    return orc_mod.Oracle()


REF_GOLDEN = os.path.join(GOLDEN, "ref_units.json.gz")


class RefAnswers:
    """The reference's own kmer.cpp / similarity.cpp / utils.cpp / fasta.cpp (oracle/_ref/libref.so) where the build could make it,
    else their answers to the same calls as recorded from it in tests/golden/ref_units.json.gz (tools/record_ref_units.py; a call
    that was not recorded fails).  Answers are tuples keyed by the call's arguments: scalars and bytes as they are, every array as
    digest(array) -- in both cases, so that the tests compare the same things either way."""

    def __init__(self, live=None, record=False):
        self.live, self.recorded = live, ({} if record else None)
        self.store = None
        if live is None:
            import json
            with gzip.open(REF_GOLDEN, "rt") as f:
                self.store = json.load(f)

    @staticmethod
    def digest(a):
        """the values and the shape of an integer array (a 64-bit prefix of their SHA-256)"""
        import hashlib
        a = np.asarray(a)
        return hashlib.sha256(repr(a.shape).encode() + np.ascontiguousarray(a, np.int64).tobytes()).hexdigest()[:16]

    @staticmethod
    def _key(name, *args):
        import hashlib
        h = hashlib.sha1(name.encode())
        for a in args:
            h.update(b"|" + (a if isinstance(a, bytes) else repr(a).encode()))
        return name + "_" + h.hexdigest()[:16]

    def _answer(self, key, call):
        if self.live is None:
            return tuple(x.encode("latin-1") if key.startswith("reads") and isinstance(x, str) else x for x in self.store[key])
        out = tuple(self.digest(x) if isinstance(x, np.ndarray) else x for x in call())
        if self.recorded is not None:
            self.recorded[key] = [x.decode("latin-1") if isinstance(x, bytes) else x for x in out]
        return out

    def extract_kmers(self, seq, k, both):
        return self._answer(self._key("kmers", seq, k, bool(both)), lambda: self.live.extract_kmers(seq, k, both))

    def pair_score(self, a, b, k, strand):
        return self._answer(self._key("pair", a, b, k, strand), lambda: self.live.pair_score(a, b, k, strand))

    def var(self, v):
        v = np.ascontiguousarray(v, np.int32)
        return self._answer(self._key("var", v.tobytes()), lambda: (self.live.var(v),))[0]

    def dump_reads(self, path, label, kind, index, raw, lower, upper):
        """fasta.cpp's reader `kind` on the file at `path`: (what it read, as ref_shim.cpp prints it; the index after the last record)"""
        data = open(path, "rb").read()

        def call():
            import ctypes as C
            f = self.live.lib.ref_dump_reads
            f.restype = C.c_int32
            f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
            out = path + ".ref_dump"
            nxt = f(path.encode(), label, kind, index, raw, lower, upper, out.encode())
            text = open(out, "rb").read()
            os.remove(out)
            return text, nxt
        return self._answer(self._key("reads", data, label, kind, index, raw, lower, upper), call)


@pytest.fixture(scope="session")
def ref_lib(oracle):
    import oracle as orc_mod
    record = os.environ.get("RATTLE_RECORD_REF")          # tools/record_ref_units.py: the live library's answers -> this file
    if record and not orc_mod.have_ref():
        raise RuntimeError("RATTLE_RECORD_REF needs oracle/_ref/libref.so")
    ref = RefAnswers(orc_mod.Ref() if orc_mod.have_ref() else None, record=bool(record))
    yield ref
    if record:
        import json
        with gzip.GzipFile(record, "wb", mtime=0) as f:
            f.write(json.dumps(ref.recorded, sort_keys=True, separators=(",", ":")).encode())


@pytest.fixture(scope="session")
def gpu_ctx():
    from rattle_amd.api import Context
    ctx = Context(0)          # raises loudly without a device / library
    yield ctx
    ctx.close()
