"""`assign` at bench size: usage bench_assign.py [READS=100000] [RUNS=3]

The reads of tools/bench_cluster.py (synthetic 1 kb cDNA reads) are clustered and corrected once; the consensi `correct` makes are the
targets and the same reads are placed on them RUNS times.  Per run, one JSON line: reads/s of the whole call (index of targets + reads
included), the device time of the reduction kernels (assign.hip) beside kernels A and B, and the bytes of records copied to the host per
read.  Beside it the time `cluster` takes on the same reads in the same process: what answering the same question costs without assign."""
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
cat, qcat, off, tid, _ = synth.reads_packed(n, max(5, n // 200), 1, True, seed=20260929, exon=(50, 210))
ctx = Context(0)
t = time.time(); cl = ctx.cluster_unsorted_packed(cat, off); t_cluster = time.time() - t
h = ctx.correct_packed(cat, qcat, off, cl, keep=True)
S = h.ptr.contents.consensi
toff = np.ctypeslib.as_array(S.off, (S.n + 1,)).copy()
tcat = np.frombuffer(C.string_at(S.seq, int(toff[S.n])), np.uint8).copy()
h.free()
print(json.dumps({"reads": n, "mean_read_len": round(float(off[n]) / n, 1), "clusters": len(cl.main_id), "targets": len(toff) - 1,
                  "mean_target_len": round(float(toff[-1]) / max(1, len(toff) - 1), 1), "cluster_s_first": round(t_cluster, 3)}), flush=True)
for it in range(runs):
    ctx.reset_stats()
    t = time.time(); rec = ctx.assign_packed(tcat, toff, cat, off); dt = time.time() - t
    ks = {name: ctx.kernel_stats(k) for name, k in (("kmer", K_KMER), ("filter_A", K_FILTER), ("score_B", K_SCORE), ("assign_reduce", K_ASSIGN))}
    ctx.reset_stats()
    t = time.time(); cl2 = ctx.cluster_unsorted_packed(cat, off); dc = time.time() - t
    placed = rec["target"] >= 0
    print(json.dumps({"run": it, "assign_s": round(dt, 3), "reads_per_s": round(n / dt), "assigned": int(placed.sum()),
                      "multiply_accepted": int((rec["n_accepted"] > 1).sum()),
                      "device_ms": {k: round(v[0], 2) for k, v in ks.items()}, "launches": {k: int(v[1]) for k, v in ks.items()},
                      "d2h_record_bytes_per_read": ks["assign_reduce"][2] / n, "cluster_s_same_reads": round(dc, 3),
                      "cluster_clusters": len(cl2.main_id)}), flush=True)
ctx.close()
