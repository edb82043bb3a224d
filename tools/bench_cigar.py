"""Kernel F (`align_cigars`) at bench size: usage bench_cigar.py [READS=100000] [RUNS=3] [OUT=profiles/pair_cigar.json]

The reads and transcripts of tools/bench_align.py (READS synthetic 1 kb cDNA reads of rattle_amd.synth on the transcripts they were drawn
from, the generator's own placement).  Per run, one JSON line: the device time of kernel F (rattle_hip_kernel_stats(7)) beside kernel E's
(id 6) in the same call on the same pairs, kernel F's launches (sub-chunks), the code bytes it wrote per pair, the bytes that came back
per pair for the CIGAR (4 per op and 4 for the count; the 40-byte record comes back as before), and the wall time of align_cigars beside
align_pairs.  The first run also checks the ops against the records: the summed lengths of every read's ops are its counts.  Everything
is written to profiles/pair_cigar.json as well."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from rattle_amd import synth
from rattle_amd.api import K_ALIGN, K_CIGAR, Context

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
genes = max(5, n // 200)
tx, _ = synth.transcriptome(genes, 1, exon=(50, 210))
cat, _, off, tid, flip = synth.reads_packed(n, genes, 1, True, seed=20260929, exon=(50, 210))
tcat = np.concatenate(tx)
toff = np.zeros(len(tx) + 1, np.uint64)
toff[1:] = np.cumsum([len(t) for t in tx])
lq, lt = np.diff(off.astype(np.int64)), np.diff(toff.astype(np.int64))[tid]
result = {"reads": n, "transcripts": len(tx), "mean_read_len": round(float(lq.mean()), 1), "mean_target_len": round(float(lt.mean()), 1),
          "cells": int((lq * lt).sum()), "runs": []}
print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)

ctx = Context(0)
ctx.align_cigars_packed(tcat, toff, cat, off, tid, flip)                  # warm-up: the code objects, the buffers' first touch
ctx.align_pairs_packed(tcat, toff, cat, off, tid, flip)
for it in range(runs):
    ctx.reset_stats()
    t = time.time(); aln, offsets, ops = ctx.align_cigars_packed(tcat, toff, cat, off, tid, flip); wall = time.time() - t
    f_ms, f_launches, f_bytes = ctx.kernel_stats(K_CIGAR)
    e_ms, e_launches, _ = ctx.kernel_stats(K_ALIGN)
    ctx.reset_stats()
    t = time.time(); aln2 = ctx.align_pairs_packed(tcat, toff, cat, off, tid, flip); wall_pairs = time.time() - t
    e_alone_ms = ctx.kernel_stats(K_ALIGN)[0]
    assert all(aln[f].tobytes() == aln2[f].tobytes() for f in aln)
    ok = aln["status"] == 0
    rows, cols = (aln["q_end"] - aln["q_start"]).astype(np.int64)[ok], (aln["t_end"] - aln["t_start"]).astype(np.int64)[ok]
    code_bytes = int((16 * ((rows + 63) // 64 * (cols - 1) + rows)).sum())
    n_ops = np.diff(offsets.astype(np.int64))
    assert f_bytes == int((rows + cols).sum()) + code_bytes + 4 * int(n_ops.sum()) + 4 * int(ok.sum())
    if it == 0:                                                          # the ops against the records, in bulk
        read = np.repeat(np.arange(n), n_ops)
        length, op = (ops >> 4).astype(np.int64), ops & 15
        for code, field in ((7, "matches"), (8, "mismatches"), (1, "q_gap"), (2, "t_gap")):
            assert (np.bincount(read[op == code], length[op == code], n).astype(np.int64) == aln[field]).all(), field
    run = {"run": it, "aligned": int(ok.sum()), "kernel_f_ms": round(f_ms, 3), "kernel_f_launches": int(f_launches),
           "kernel_e_ms_same_call": round(e_ms, 3), "kernel_e_launches": int(e_launches), "kernel_e_ms_align_pairs": round(e_alone_ms, 3),
           "f_over_e": round(f_ms / e_ms, 3), "kernel_f_us_per_pair": round(1e3 * f_ms / max(1, int(ok.sum())), 3),
           "code_bytes_per_pair": round(code_bytes / max(1, int(ok.sum())), 1), "mean_ops_per_pair": round(float(n_ops[ok].mean()), 2),
           "cigar_bytes_returned_per_pair": round(4 * float(n_ops[ok].mean()) + 4, 1),
           "align_cigars_wall_s": round(wall, 3), "align_pairs_wall_s": round(wall_pairs, 3)}
    result["runs"].append(run)
    print(json.dumps(run), flush=True)
ctx.close()
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pair_cigar.json")
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
