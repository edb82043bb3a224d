"""Kernel E (`align_pairs`) at bench size: usage bench_align.py [READS=100000] [RUNS=3] [POA_PAIRS=2000] [OUT=profiles/pair_align.json]

READS synthetic 1 kb cDNA reads (rattle_amd.synth, the reads of tools/bench_assign.py) on the transcripts they were drawn from: the
placement handed to align_pairs is the generator's own (transcript, strand).  Per run, one JSON line: kernel E's device time
(rattle_hip_kernel_stats(6)), GCUPS = sum Lq * Lt over that time, the record bytes returned per read, and the wall time of `assign`
alone and of `assign` followed by the alignment of its placement.  The only other alignment engine the library has is kernel C: the
first POA_PAIRS pairs go through Context.poa_msa as two-sequence packs (transcript, read on the transcript's strand) in the same
process, device time from rattle_hip_kernel_stats(3).  Everything is written to profiles/pair_align.json as well."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from rattle_amd import synth
from rattle_amd.api import K_ALIGN, K_POA, Context

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n_poa = min(n, int(sys.argv[3]) if len(sys.argv) > 3 else 2000)
genes = max(5, n // 200)
tx, _ = synth.transcriptome(genes, 1, exon=(50, 210))
cat, _, off, tid, flip = synth.reads_packed(n, genes, 1, True, seed=20260929, exon=(50, 210))
tcat = np.concatenate(tx)
toff = np.zeros(len(tx) + 1, np.uint64)
toff[1:] = np.cumsum([len(t) for t in tx])
lq, lt = np.diff(off.astype(np.int64)), np.diff(toff.astype(np.int64))[tid]
cells = int((lq * lt).sum())
seq_bytes = int((lq + lt).sum())
result = {"reads": n, "transcripts": len(tx), "mean_read_len": round(float(lq.mean()), 1), "mean_target_len": round(float(lt.mean()), 1),
          "cells": cells, "runs": []}
print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)

ctx = Context(0)
ctx.align_pairs_packed(tcat, toff, cat, off, tid, flip)                   # warm-up: the code object, the buffers' first touch
for it in range(runs):
    ctx.reset_stats()
    t = time.time(); aln = ctx.align_pairs_packed(tcat, toff, cat, off, tid, flip); wall = time.time() - t
    ms, launches, nbytes = ctx.kernel_stats(K_ALIGN)
    t = time.time(); rec = ctx.assign_packed(tcat, toff, cat, off); t_assign = time.time() - t
    t = time.time()
    rec2 = ctx.assign_packed(tcat, toff, cat, off)
    aln2 = ctx.align_pairs_packed(tcat, toff, cat, off, rec2["target"], rec2["rev"])
    t_both = time.time() - t
    ok = aln["status"] == 0
    run = {"run": it, "kernel_e_ms": round(ms, 3), "launches": int(launches), "gcups": round(cells / ms / 1e6, 2),
           "us_per_pair": round(1e3 * ms / n, 3), "align_pairs_wall_s": round(wall, 3),
           "record_bytes_per_read": (nbytes - seq_bytes) / n, "aligned": int(ok.sum()),
           "mean_identity": round(float((aln["matches"][ok] / np.maximum(1, aln["matches"][ok] + aln["mismatches"][ok] + aln["q_gap"][ok] + aln["t_gap"][ok])).mean()), 4),
           "assign_wall_s": round(t_assign, 3), "assign_then_align_wall_s": round(t_both, 3),
           "assign_placed": int((rec["target"] >= 0).sum()), "assign_placed_and_aligned": int((aln2["status"] == 0).sum())}
    result["runs"].append(run)
    print(json.dumps(run), flush=True)

# kernel C on the same pairs, as packs of two sequences (the transcript first: it is the graph the read is aligned to)
comp = bytes.maketrans(b"ACGT", b"TGCA")
packs = []
for r in range(n_poa):
    q = cat[int(off[r]):int(off[r + 1])].tobytes()
    packs.append([tx[tid[r]].tobytes(), q.translate(comp)[::-1] if flip[r] else q])
ctx.poa_msa(packs[:64])                                                  # warm-up
poa = []
for it in range(runs):
    ctx.reset_stats()
    t = time.time(); ctx.poa_msa(packs); wall = time.time() - t
    ms = ctx.kernel_stats(K_POA)[0]
    poa.append({"run": it, "pairs": n_poa, "kernel_c_ms": round(ms, 3), "us_per_pair": round(1e3 * ms / n_poa, 3), "poa_msa_wall_s": round(wall, 3)})
    print(json.dumps(poa[-1]), flush=True)
ctx.reset_stats()
ctx.align_pairs_packed(tcat, toff[:], cat[:int(off[n_poa])], off[:n_poa + 1], tid[:n_poa], flip[:n_poa])
result["kernel_c_two_sequence_packs"] = poa
result["kernel_e_on_the_same_pairs"] = {"pairs": n_poa, "kernel_e_ms": round(ctx.kernel_stats(K_ALIGN)[0], 3),
                                        "us_per_pair": round(1e3 * ctx.kernel_stats(K_ALIGN)[0] / n_poa, 3)}
print(json.dumps(result["kernel_e_on_the_same_pairs"]), flush=True)
ctx.close()
out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "pair_align.json")
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
