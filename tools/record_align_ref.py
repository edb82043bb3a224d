"""Records the answers of the pair-alignment references (tests/align_affine_ref.py in local mode, tests/align_ends_ref.py in read mode) into
tests/golden/align_pairs_ref.json.gz, which tests/test_align_model.py holds tests/align_model.py to: for every distinct (read, transcript,
strand, scoring, mode) their cases submit -- 5,4,8,8 and 5,4,8,6 on every case, every other scoring of the module's SCORINGS on its
EDGE_CASES, as the device tests run them -- the 10-field record and the CIGAR text of pair().  The file was first written from the two
modules when each still held its own copy of the recurrence.  Run it again after adding or changing a case: an entry that is already in
the file has to come out as it stands there, else nothing is written.  usage: python tools/record_align_ref.py"""
import gzip
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "align_pairs_ref.json.gz")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def key(q: bytes, t: bytes, rev: int, sc, mode: str) -> str:
    return hashlib.sha1(repr((q, t, int(rev), tuple(int(v) for v in sc), mode)).encode()).hexdigest()[:20]


def submissions():
    """{key: (read as given, transcript, strand, scoring, mode, reference module)} of every pair the cases submit; no empty sequence"""
    import align_affine_ref as A
    import align_ends_ref as E
    out = {}
    for mode, ref in (("local", A), ("read", E)):
        for name, build in sorted(ref.all_cases().items()):
            targets, reads, tor, rev = build()
            for sc in ref.SCORINGS:
                if sc not in (A.LINEAR, A.ENGINE) and name not in ref.EDGE_CASES:
                    continue
                for q, x, s in zip(reads, tor, rev):
                    if x >= 0 and q and targets[x]:
                        out.setdefault(key(q, targets[x], s, sc, mode), (q, targets[x], int(s), sc, mode, ref))
    return out


def load():
    """{key: (record, CIGAR text)} of the file"""
    with gzip.open(FIXTURE, "rt") as f:
        doc = json.load(f)
    assert doc["count"] == len(doc["pairs"])
    return {k: (tuple(rec), cg.encode()) for k, (rec, cg) in doc["pairs"].items()}


if __name__ == "__main__":
    import cigar_ref as CG
    old = load() if os.path.exists(FIXTURE) else {}
    pairs, moved = {}, 0
    for k, (q, t, s, sc, mode, ref) in submissions().items():
        rec, ops = ref.pair(q, t, s, sc)
        assert ref.pair(q, t, s, sc, "forward")[0] == rec, (q, t, s, sc, mode)
        pairs[k] = (tuple(int(v) for v in rec), CG.text(ops))
        moved += k in old and old[k] != pairs[k]
    print(f"{len(pairs)} entries, {len(pairs.keys() - old.keys())} new, {len(old.keys() - pairs.keys())} gone, {moved} with another answer")
    if moved:
        sys.exit("an answer that is on record has changed: nothing written")
    with open(FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps({"count": len(pairs), "pairs": {k: [list(rec), cg.decode()] for k, (rec, cg) in sorted(pairs.items())}},
                           separators=(",", ":")).encode())
