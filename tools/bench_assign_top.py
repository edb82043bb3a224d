"""`assign` with the candidate list at bench size: usage bench_assign_top.py [READS=100000] [RUNS=3] [OUT.json]

The reads and targets of tools/bench_assign.py (synthetic 1 kb cDNA reads, clustered and corrected once; the consensi are the
targets).  RUNS times each: `assign` without candidates -- the path the candidate list leaves untouched, to be held against
tools/bench_assign.py at the parent commit on the same box --, then `assign_top` at K = 2, 4 and 8.  Per call one JSON line: wall time
of the whole call (index of targets + reads included), the device time and launches of the reduction kernels (kernel id 5, assign.hip)
beside kernels A and B, and the bytes per read copied to the host.  With OUT.json the ranges over the runs are written there
(profiles/assign_top.json is such a file)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rattle_amd import synth
from rattle_amd.api import K_ASSIGN, K_FILTER, K_KMER, K_SCORE, Context

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else None
cat, qcat, off, tid, _ = synth.reads_packed(n, max(5, n // 200), 1, True, seed=20260929, exon=(50, 210))
ctx = Context(0)
cl = ctx.cluster_unsorted_packed(cat, off)
h = ctx.correct_packed(cat, qcat, off, cl, keep=True)
S = h.ptr.contents.consensi
toff = np.ctypeslib.as_array(S.off, (S.n + 1,)).copy()
tcat = np.frombuffer(C.string_at(S.seq, int(toff[S.n])), np.uint8).copy()
h.free()
head = {"reads": n, "mean_read_len": round(float(off[n]) / n, 1), "targets": len(toff) - 1,
        "mean_target_len": round(float(toff[-1]) / max(1, len(toff) - 1), 1)}
print(json.dumps(head), flush=True)
seen = {}
for it in range(runs):
    for K in (0, 2, 4, 8):
        ctx.reset_stats()
        t = time.time()
        if K:
            rec, cands = ctx.assign_packed_top(tcat, toff, cat, off, K)
        else:
            rec, cands = ctx.assign_packed(tcat, toff, cat, off), None
        dt = time.time() - t
        ks = {name: ctx.kernel_stats(k) for name, k in (("kmer", K_KMER), ("filter_A", K_FILTER), ("score_B", K_SCORE), ("assign_reduce", K_ASSIGN))}
        line = {"run": it, "K": K, "assign_s": round(dt, 3), "reads_per_s": round(n / dt), "assigned": int((rec["target"] >= 0).sum()),
                "device_ms": {k: round(v[0], 2) for k, v in ks.items()}, "launches": {k: int(v[1]) for k, v in ks.items()},
                "d2h_bytes_per_read": ks["assign_reduce"][2] / n}
        if K:
            assert (cands["target"][:, 0] == rec["target"]).all()
            line["slots_filled"] = int(cands["count"].sum())
            line["reads_with_a_second"] = int((cands["count"] > 1).sum())
        print(json.dumps(line), flush=True)
        seen.setdefault(K, []).append(line)
ctx.close()
if out_path:
    rng = lambda v: [min(v), max(v)]
    res = dict(head, runs=runs, what="ranges [min, max] over the runs; K = 0: assign without candidates")
    for K, lines in seen.items():
        res[f"K={K}"] = {"assign_s": rng([l["assign_s"] for l in lines]),
                         "device_ms": {k: rng([l["device_ms"][k] for l in lines]) for k in lines[0]["device_ms"]},
                         "assign_reduce_launches": lines[0]["launches"]["assign_reduce"], "d2h_bytes_per_read": lines[0]["d2h_bytes_per_read"]}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
