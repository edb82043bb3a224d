"""Kernel G (`align_pileup`) at bench size: usage bench_pileup.py [READS=100000] [OUT=profiles/pair_pileup.json] [SKEW=0]

The reads and transcripts of tools/bench_align.py (READS synthetic 1 kb cDNA reads of rattle_amd.synth on the transcripts they were drawn
from, the generator's own placement).  Three rounds in one process, each round align_cigars, align_pileup(cigars=False) and
align_pileup(cigars=True) in turn.  Per call one entry: device time and launches of kernels E, F and G (rattle_hip_kernel_stats 6, 7, 11),
the wall time of the call, and the bytes it returns to the host per read (40 for the record, 4 for the count, 4 per op where the ops
return, and 32 per target base once for the table).  The first round checks the table against the records: the letters sum to matches +
mismatches, del to t_gap, starts and ends to the aligned reads, and the three calls return the same records and the same table.

SKEW = a fraction: that share of the reads is placed on transcript 0 instead (reads of other transcripts: they align badly, but the adds
they make all fall on one transcript's positions) -- the case where the atomics queue on few addresses.

With RATTLE_HIP_LIB naming a library that has no rattle_hip_align_pileup (a build of the parent commit) only align_cigars is run: ids 6
and 7 of the two builds are compared through the same script."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from rattle_amd import _lib, synth

from rattle_amd.api import K_ALIGN, K_CIGAR, K_PILEUP, Context

OPTIONAL = ("rattle_hip_align_pileup", "rattle_hip_pileup_free")


def bind_library():
    """The library bound as _lib.load() binds it, from the binding's table as it stands, except that the two symbols of align_pileup
    may be missing (a build of the commit before); handed to _lib as the loaded library.  Returns whether they are there."""
    lib, has = ctypes.CDLL(_lib.LIB_PATH), True
    for name, (res, args) in _lib.SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if name not in OPTIONAL:
                raise
            has = False
            continue
        fn.restype, fn.argtypes = res, args
    _lib._lib = lib
    return has


HAS_PILEUP = bind_library()

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pair_pileup.json")
skew = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
genes = max(5, n // 200)
tx, _ = synth.transcriptome(genes, 1, exon=(50, 210))
cat, _, off, tid, flip = synth.reads_packed(n, genes, 1, True, seed=20260929, exon=(50, 210))
tid = np.array(tid, np.int32)
if skew > 0:
    tid[np.random.default_rng(7).random(n) < skew] = 0
tcat = np.concatenate(tx)
toff = np.zeros(len(tx) + 1, np.uint64)
toff[1:] = np.cumsum([len(t) for t in tx])
lq, lt = np.diff(off.astype(np.int64)), np.diff(toff.astype(np.int64))[tid]
result = {"reads": n, "transcripts": len(tx), "target_bases": int(toff[-1]), "mean_read_len": round(float(lq.mean()), 1),
          "mean_target_len": round(float(lt.mean()), 1), "cells": int((lq * lt).sum()), "skew": skew, "library_has_align_pileup": HAS_PILEUP,
          "runs": []}
print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)

ctx = Context(0)
args = (tcat, toff, cat, off, tid, flip)
CALLS = [("align_cigars", lambda: ctx.align_cigars_packed(*args))]
if HAS_PILEUP:
    CALLS += [("align_pileup", lambda: ctx.align_pileup_packed(*args)), ("align_pileup_cigars", lambda: ctx.align_pileup_packed(*args, cigars=True))]
for _, call in CALLS:                                                     # warm-up: the code objects, the buffers' first touch
    call()
for it in range(3):
    got = {}
    for name, call in CALLS:
        ctx.reset_stats()
        t = time.time(); res = call(); wall = time.time() - t
        got[name] = res
        aln = res[0]
        ok = aln["status"] == 0
        stats = {k: ctx.kernel_stats(k) for k in ((K_ALIGN, K_CIGAR, K_PILEUP) if HAS_PILEUP else (K_ALIGN, K_CIGAR))}
        run = {"run": it, "call": name, "aligned": int(ok.sum()), "wall_s": round(wall, 3),
               "kernel_e_ms": round(stats[K_ALIGN][0], 3), "kernel_e_launches": int(stats[K_ALIGN][1]),
               "kernel_f_ms": round(stats[K_CIGAR][0], 3), "kernel_f_launches": int(stats[K_CIGAR][1])}
        returned = 40.0 * n + 4.0 * int(ok.sum())
        if name == "align_cigars":
            returned += 4.0 * len(res[2])
        else:
            run.update({"kernel_g_ms": round(stats[K_PILEUP][0], 3), "kernel_g_launches": int(stats[K_PILEUP][1]),
                        "kernel_g_alg_bytes": int(stats[K_PILEUP][2]), "g_over_f": round(stats[K_PILEUP][0] / stats[K_CIGAR][0], 4)})
            returned += 32.0 * int(toff[-1]) + (4.0 * len(res[1][1]) if res[1] is not None else 0.0)
        run["bytes_returned_per_read"] = round(returned / n, 1)
        result["runs"].append(run)
        print(json.dumps(run), flush=True)
    if it == 0 and HAS_PILEUP:
        aln, table = got["align_pileup"][0], got["align_pileup"][2]
        ok = aln["status"] == 0
        for other in ("align_cigars", "align_pileup_cigars"):
            assert all(aln[f].tobytes() == got[other][0][f].tobytes() for f in aln), other
        assert all(table[f].tobytes() == got["align_pileup_cigars"][2][f].tobytes() for f in table)
        assert got["align_pileup_cigars"][1][1].tobytes() == got["align_cigars"][2].tobytes()
        letters = sum(int(table[f].sum(dtype=np.int64)) for f in "acgt")
        assert letters == int(aln["matches"][ok].sum(dtype=np.int64)) + int(aln["mismatches"][ok].sum(dtype=np.int64))
        assert int(table["del"].sum(dtype=np.int64)) == int(aln["t_gap"][ok].sum(dtype=np.int64))
        assert int(table["starts"].sum(dtype=np.int64)) == int(table["ends"].sum(dtype=np.int64)) == int(ok.sum())
        depth = sum(table[f].astype(np.int64) for f in ("a", "c", "g", "t", "del"))
        result["positions_covered"], result["largest_depth"] = int((depth > 0).sum()), int(depth.max())
ctx.close()
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
