"""Kernels E and F in read mode (`align_cigars(..., mode="read")`, `--paf-end-to-end`) beside the local mode at bench size:
usage bench_align_ends.py [READS=100000] [RUNS=3] [OUT=profiles/pair_align_ends.json] [SCORING=5,4,8,6] [local-only]

The reads and transcripts of tools/bench_align.py and tools/bench_align_affine.py (READS synthetic 1 kb cDNA reads of rattle_amd.synth on
the transcripts they were drawn from, the generator's own placement).  Per run, one JSON line, from ONE process, the four calls
alternating -- linear local, linear read, affine local, affine read -- each behind a reset of the stats, since a mode counts under the
ids of its gap form: the device time of kernel E and of kernel F (rattle_hip_kernel_stats, HIP events), the ratios read / local, the
rows and columns kernel F's rectangles span, the wall time of each call.  At the end the medians.  The first run also checks what the
read mode promises: status 0 wherever the local mode has 0 or 1, q_start 0, q_end Lq.  `local-only` measures the two local calls alone,
through the calls without a mode: the form in which a build from before the read mode runs this file, for the comparison of the local
mode with its own past (same process layout, same pairs).  Everything is written to profiles/pair_align_ends.json as well."""
import json
import os
import statistics
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
local_only = len(sys.argv) > 5 and sys.argv[5] == "local-only"
genes = max(5, n // 200)
tx, _ = synth.transcriptome(genes, 1, exon=(50, 210))
cat, _, off, tid, flip = synth.reads_packed(n, genes, 1, True, seed=20260929, exon=(50, 210))
tcat = np.concatenate(tx)
toff = np.zeros(len(tx) + 1, np.uint64)
toff[1:] = np.cumsum([len(t) for t in tx])
lq, lt = np.diff(off.astype(np.int64)), np.diff(toff.astype(np.int64))[tid]
cells = int((lq * lt).sum())
result = {"reads": n, "transcripts": len(tx), "mean_read_len": round(float(lq.mean()), 1), "mean_target_len": round(float(lt.mean()), 1),
          "cells": cells, "scoring": list(scoring), "local_only": local_only, "runs": []}
print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)

FORMS = (("linear", None, K_ALIGN, K_CIGAR), ("affine", scoring, K_ALIGN_AFFINE, K_CIGAR_AFFINE))
MODES = ("local",) if local_only else ("local", "read")
ctx = Context(0)
args = (tcat, toff, cat, off, tid, flip)


def call(sc, mode):
    kw = {} if local_only else {"mode": mode}
    return ctx.align_cigars_packed(*args, scoring=sc, **kw)


for _, sc, _, _ in FORMS:                                                  # warm-up: the code objects, the buffers' first touch
    for mode in MODES:
        call(sc, mode)
for it in range(runs):
    run = {"run": it}
    got = {}
    for form, sc, k_align, k_cigar in FORMS:
        for mode in MODES:
            ctx.reset_stats()
            t = time.time(); aln, _, ops = call(sc, mode); wall = time.time() - t
            got[form, mode] = aln
            e, f = ctx.kernel_stats(k_align), ctx.kernel_stats(k_cigar)
            ok = aln["status"] == 0
            rows, cols = (aln["q_end"] - aln["q_start"]).astype(np.int64)[ok], (aln["t_end"] - aln["t_start"]).astype(np.int64)[ok]
            run.update({f"e_{form}_{mode}_ms": round(e[0], 3), f"f_{form}_{mode}_ms": round(f[0], 3), f"e_{form}_{mode}_gcups": round(cells / e[0] / 1e6, 2),
                        f"f_{form}_{mode}_launches": int(f[1]), f"aligned_{form}_{mode}": int(ok.sum()),
                        f"mean_rows_{form}_{mode}": round(float(rows.mean()), 1), f"mean_cols_{form}_{mode}": round(float(cols.mean()), 1),
                        f"ops_{form}_{mode}": int(len(ops)), f"wall_{form}_{mode}_s": round(wall, 3)})
        if not local_only:
            run[f"e_{form}_read_over_local"] = round(run[f"e_{form}_read_ms"] / run[f"e_{form}_local_ms"], 3)
            run[f"f_{form}_read_over_local"] = round(run[f"f_{form}_read_ms"] / run[f"f_{form}_local_ms"], 3)
            if it == 0:
                loc, rd = got[form, "local"], got[form, "read"]
                sent = loc["status"] <= 1
                assert (rd["status"][sent & (lq > 0) & (lt > 0)] == 0).all() and (rd["status"][~sent] == loc["status"][~sent]).all()
                ok = rd["status"] == 0
                assert (rd["q_start"][ok] == 0).all() and (rd["q_end"][ok] == lq[ok]).all()
    result["runs"].append(run)
    print(json.dumps(run), flush=True)
ctx.close()
keys = [k for k in result["runs"][0] if k.endswith("_ms") or k.endswith("_over_local")]
result["median"] = {k: round(statistics.median(r[k] for r in result["runs"]), 3) for k in keys}
result["spread"] = {k: round(max(r[k] for r in result["runs"]) - min(r[k] for r in result["runs"]), 3) for k in keys if k.endswith("_ms")}
print(json.dumps({"median": result["median"], "spread": result["spread"]}), flush=True)
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pair_align_ends.json")
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
