"""The abundance EM at bench size: usage bench_abundance.py [READS=1000000] [OUT.json] [TOP_READS=100000]

Synthetic candidate lists, no sequences needed: READS reads on 500 and on 5000 targets in families of 8.  A read draws its best target
from the expression profile -- flat, or skewed: a Zipf law whose exponent is set so that the top target holds a quarter of the reads --
and 0 .. 7 further members of that target's family, all compatible.  The merged scatter (the default) and the plain one
(RATTLE_EM_PLAIN=1: one atomic per entry, no sort, no merge) alternate in one process, three runs each, and must give the same bytes.
Per call one JSON line: the wall time of the call, the iterations, the device time and the launches of kernel id 10, and the device time
per iteration (ordering, start and posterior included: they are a few iterations' worth).  With TOP_READS > 0 the wall time of
assign_top at 8 slots on the reads and targets of tools/bench_assign_top.py follows, for scale: the step that makes the list the EM
works on.  With OUT.json the ranges over the runs are written there (profiles/abundance.json is such a file)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rattle_amd import synth
from rattle_amd.api import K_ABUNDANCE, Context

FAMILY = 8


def zipf_exponent(nt, top=0.25):
    """s with 1 / sum(r ** -s, r = 1 .. nt) == top, by bisection"""
    lo, hi = 0.5, 3.0
    r = np.arange(1, nt + 1, dtype=np.float64)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 1.0 / (r ** -mid).sum() < top else (lo, mid)
    return 0.5 * (lo + hi)


def lists(n, nt, skewed, rng):
    full = nt // FAMILY * FAMILY                          # the targets of whole families; the few behind them stay unnamed
    if skewed:
        w = np.arange(1, full + 1, dtype=np.float64) ** -zipf_exponent(full)
        rank = rng.choice(full, size=n, p=w / w.sum())
        best = rng.permutation(full)[rank]                # the expressed targets lie anywhere in the file
    else:
        best = rng.integers(0, full, n)
    count = rng.integers(1, FAMILY + 1, n).astype(np.uint32)
    others = rng.permuted(np.tile(np.arange(1, FAMILY), (n, 1)), axis=1)      # the other members of the family, in a random order
    target = np.empty((n, FAMILY), np.int32)
    target[:, 0] = best
    target[:, 1:] = (best[:, None] // FAMILY) * FAMILY + (best[:, None] % FAMILY + others) % FAMILY
    used = np.arange(FAMILY)[None, :] < count[:, None]
    target[~used] = -1
    return {"count": count, "target": target, "score": np.where(used, 0.8, -1.0)}


n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
top_reads = int(sys.argv[3]) if len(sys.argv) > 3 else 100000
ctx = Context(0)
res = {"reads": n, "slots": FAMILY, "runs": 3, "what": "ranges [min, max] over three runs of each form, alternating in one process", "cases": {}}
for nt in (500, 5000):
    for skewed in (False, True):
        name = f"{nt} targets, {'skewed' if skewed else 'flat'}"
        cands = lists(n, nt, skewed, np.random.default_rng(20261021 + nt + int(skewed)))
        share = float(np.bincount(cands["target"][:, 0], minlength=nt).max()) / n
        seen, first = {"merged": [], "plain": []}, None
        for it in range(3):
            for form in ("merged", "plain"):
                if form == "plain":
                    os.environ["RATTLE_EM_PLAIN"] = "1"
                else:
                    os.environ.pop("RATTLE_EM_PLAIN", None)
                ctx.reset_stats()
                t = time.time()
                ab = ctx.abundance(cands, nt)
                dt = time.time() - t
                ms, launches, _ = ctx.kernel_stats(K_ABUNDANCE)
                digest = (ab["units"].tobytes(), ab["delta"].tobytes(), ab["posterior"].tobytes(), ab["compatible_reads"].tobytes())
                first = first or digest
                assert digest == first, "the two forms, or two runs, differ"
                line = {"case": name, "form": form, "run": it, "call_s": round(dt, 4), "iterations": ab["iterations"], "converged": ab["converged"],
                        "device_ms": round(ms, 3), "launches": int(launches), "device_ms_per_iteration": round(ms / max(1, ab["iterations"]), 5)}
                print(json.dumps(line), flush=True)
                seen[form].append(line)
        os.environ.pop("RATTLE_EM_PLAIN", None)
        rng = lambda v: [min(v), max(v)]
        res["cases"][name] = {"top_target_share": round(share, 4), "iterations": seen["merged"][0]["iterations"], "launches": seen["merged"][0]["launches"]}
        for form, lines in seen.items():
            res["cases"][name][form] = {f: rng([l[f] for l in lines]) for f in ("call_s", "device_ms", "device_ms_per_iteration")}
if top_reads:
    cat, qcat, off, tid, _ = synth.reads_packed(top_reads, max(5, top_reads // 200), 1, True, seed=20260929, exon=(50, 210))
    cl = ctx.cluster_unsorted_packed(cat, off)
    h = ctx.correct_packed(cat, qcat, off, cl, keep=True)
    S = h.ptr.contents.consensi
    toff = np.ctypeslib.as_array(S.off, (S.n + 1,)).copy()
    tcat = np.frombuffer(C.string_at(S.seq, int(toff[S.n])), np.uint8).copy()
    h.free()
    times = []
    for it in range(3):
        t = time.time()
        rec, cands = ctx.assign_packed_top(tcat, toff, cat, off, 8)
        times.append(round(time.time() - t, 4))
    t = time.time()
    ab = ctx.abundance(cands, len(toff) - 1)
    res["assign_top_for_scale"] = {"reads": top_reads, "targets": len(toff) - 1, "assign_top_8_s": [min(times), max(times)],
                                   "abundance_on_its_list_s": round(time.time() - t, 4), "iterations": ab["iterations"]}
    print(json.dumps(res["assign_top_for_scale"]), flush=True)
ctx.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
