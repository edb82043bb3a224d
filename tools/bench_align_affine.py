"""The three-state kernels E and F (`align_pairs` / `align_cigars` with a scoring) beside kernels E and F at bench size:
usage bench_align_affine.py [READS=100000] [RUNS=3] [OUT=profiles/pair_align_affine.json] [SCORING=5,4,8,6]

The reads and transcripts of tools/bench_align.py (READS synthetic 1 kb cDNA reads of rattle_amd.synth on the transcripts they were drawn
from, the generator's own placement), the pairs of profiles/pair_align.json's measurement.  Per run, one JSON line, from ONE process: the
device time and launches of kernels 6 and 7 (align_cigars) and of kernels 8 and 9 (align_cigars with the scoring) on the same pairs
(rattle_hip_kernel_stats, HIP events), the ratios 8 / 6 and 9 / 7, GCUPS of both forward kernels, the code bytes per pair of both
traceback kernels, the strip bytes per pair, and the wall time of both calls.  The first run also checks that the scoring 5,4,8,8
returns the records and the ops of kernels E and F.  Everything is written to profiles/pair_align_affine.json as well."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from rattle_amd import synth
from rattle_amd.api import K_ALIGN, K_ALIGN_AFFINE, K_CIGAR, K_CIGAR_AFFINE, Context

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
scoring = tuple(int(v) for v in sys.argv[4].split(",")) if len(sys.argv) > 4 else (5, 4, 8, 6)
genes = max(5, n // 200)
tx, _ = synth.transcriptome(genes, 1, exon=(50, 210))
cat, _, off, tid, flip = synth.reads_packed(n, genes, 1, True, seed=20260929, exon=(50, 210))
tcat = np.concatenate(tx)
toff = np.zeros(len(tx) + 1, np.uint64)
toff[1:] = np.cumsum([len(t) for t in tx])
lq, lt = np.diff(off.astype(np.int64)), np.diff(toff.astype(np.int64))[tid]
cells = int((lq * lt).sum())
result = {"reads": n, "transcripts": len(tx), "mean_read_len": round(float(lq.mean()), 1), "mean_target_len": round(float(lt.mean()), 1),
          "cells": cells, "scoring": list(scoring), "runs": []}
print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)


def code_bytes(aln, rec_bytes):
    ok = aln["status"] == 0
    rows, cols = (aln["q_end"] - aln["q_start"]).astype(np.int64)[ok], (aln["t_end"] - aln["t_start"]).astype(np.int64)[ok]
    return int((rec_bytes * ((rows + 63) // 64 * (cols - 1) + rows)).sum()) / max(1, int(ok.sum()))


ctx = Context(0)
args = (tcat, toff, cat, off, tid, flip)
ctx.align_cigars_packed(*args)                                             # warm-up: the code objects, the buffers' first touch
ctx.align_cigars_packed(*args, scoring=scoring)
for it in range(runs):
    ctx.reset_stats()
    t = time.time(); lin, lin_off, lin_ops = ctx.align_cigars_packed(*args); wall_lin = time.time() - t
    t = time.time(); aff, aff_off, aff_ops = ctx.align_cigars_packed(*args, scoring=scoring); wall_aff = time.time() - t
    k = {i: ctx.kernel_stats(i) for i in (K_ALIGN, K_CIGAR, K_ALIGN_AFFINE, K_CIGAR_AFFINE)}
    if it == 0:                                                          # 5,4,8,8 on the three-state kernels is kernels E and F
        same, same_off, same_ops = ctx.align_cigars_packed(*args, scoring=(5, 4, 8, 8))
        assert all(same[f].tobytes() == lin[f].tobytes() for f in lin) and same_off.tobytes() == lin_off.tobytes() and same_ops.tobytes() == lin_ops.tobytes()
    strip = float(np.where(lq > 64, lt, 0).mean())                       # strip records per pair of both forward kernels
    run = {"run": it, "aligned_linear": int((lin["status"] == 0).sum()), "aligned_scored": int((aff["status"] == 0).sum()),
           "records_that_differ": int(sum(np.any([lin[f] != aff[f] for f in lin], axis=0))),
           "kernel_6_ms": round(k[K_ALIGN][0], 3), "kernel_6_launches": int(k[K_ALIGN][1]),
           "kernel_8_ms": round(k[K_ALIGN_AFFINE][0], 3), "kernel_8_launches": int(k[K_ALIGN_AFFINE][1]),
           "kernel_7_ms": round(k[K_CIGAR][0], 3), "kernel_7_launches": int(k[K_CIGAR][1]),
           "kernel_9_ms": round(k[K_CIGAR_AFFINE][0], 3), "kernel_9_launches": int(k[K_CIGAR_AFFINE][1]),
           "ratio_8_over_6": round(k[K_ALIGN_AFFINE][0] / k[K_ALIGN][0], 3), "ratio_9_over_7": round(k[K_CIGAR_AFFINE][0] / k[K_CIGAR][0], 3),
           "kernel_6_gcups": round(cells / k[K_ALIGN][0] / 1e6, 2), "kernel_8_gcups": round(cells / k[K_ALIGN_AFFINE][0] / 1e6, 2),
           "kernel_6_strip_bytes_per_pair": round(16 * strip, 1), "kernel_8_strip_bytes_per_pair": round(40 * strip, 1),
           "kernel_7_code_bytes_per_pair": round(code_bytes(lin, 16), 1), "kernel_9_code_bytes_per_pair": round(code_bytes(aff, 32), 1),
           "kernel_7_alg_bytes_per_pair": round(k[K_CIGAR][2] / n, 1), "kernel_9_alg_bytes_per_pair": round(k[K_CIGAR_AFFINE][2] / n, 1),
           "align_cigars_wall_s": round(wall_lin, 3), "align_cigars_scored_wall_s": round(wall_aff, 3)}
    result["runs"].append(run)
    print(json.dumps(run), flush=True)
ctx.close()
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pair_align_affine.json")
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
