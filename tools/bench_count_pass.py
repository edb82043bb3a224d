"""The count pass of one cluster evaluation through its "seed" and "index" forms (pair_count.hip / pair_index.hip), on one context,
through the test hook rattle_hip_debug_evaluate: the same rectangle list, one warm-up call per form, then REPS timed calls per form
in alternation.  Two clocks per call: host wall time around the call (it includes kernel A, the survivor list's trip to the host and
the hook's own bookkeeping, the same for both forms) and the count pass's device time from rattle_hip_kernel_stats (HIP events; for
"seed" the count kernel, for "index" grouping + build + count; t_s is out of reach, so the full pass never runs).

Shapes (rattle_amd.synth):
  a  1 kb cDNA reads, k = 10, 256 seeds x 1e5 candidates, bit-vector threshold 0.4 (the headline shape)
  b  4 - 8 kb --rna reads, k = 10, 256 and 1024 seeds x 2e4 candidates, threshold 0.2 (the filter saturates)
  c  500 rectangles of 8 seeds x 200 candidates, the reads of (a), k = 11
  d  shape (b) with 256 seeds at k = 6 (the `polish` setting)

Writes profiles/count_pass_index.json.  usage: python tools/bench_count_pass.py [--reps 5] [--out FILE] [--shapes a,b,c,d]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rattle_amd import synth  # noqa: E402
from rattle_amd.api import Context  # noqa: E402

K_SCORE = 2
ACGT = np.frombuffer(b"ACGT", np.uint8)


def draw(n, lens_lo, lens_hi, n_tx, both, seed):
    rng = np.random.default_rng(seed)
    tx = [ACGT[rng.integers(0, 4, int(l))] for l in rng.integers(lens_lo, lens_hi + 1, n_tx)]
    cat, _, off, _, _ = synth.reads_packed(n, 0, 1, both, seed=seed + 1, tx=tx)
    return cat, off


def measure(ctx, rects, is_rna, reps):
    out = {}
    info = None
    for form in ("seed", "index"):                               # warm-up: buffers grown, code loaded
        got = ctx.debug_evaluate(rects, 1e9, is_rna=is_rna, count_pass=form)
        assert got["count_pass"] == {form} and len(got["kept"]["seed"]) == 0
        s = got["survivors"]
        digest = (len(s["seed"]), int(s["count"].astype(np.int64).sum()))
        if info is None:
            info = digest
        elif ctx.k == 10:
            assert digest == info, (digest, info)                # both exact (k = 6: kb-long seeds overflow the seed form's repeat list; k = 11: the fold)
        else:
            assert digest[0] == info[0]
        out[form] = {"wall_ms": [], "count_pass_device_ms": []}
        del got
    for _ in range(reps):
        for form in ("seed", "index"):
            ctx.reset_stats()
            t0 = time.perf_counter()
            got = ctx.debug_evaluate(rects, 1e9, is_rna=is_rna, count_pass=form)
            out[form]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            out[form]["count_pass_device_ms"].append(ctx.kernel_stats(K_SCORE)[0])
            del got
    for form in out:
        for f in ("wall_ms", "count_pass_device_ms"):
            v = out[form][f]
            out[form][f] = {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}
    return info[0], out


def shape_record(ctx, name, rects, is_rna, reps, lens, note):
    ns = sum(len(r[0]) for r in rects)
    nc = sum(len(r[1]) for r in rects)
    entries = int(sum(np.maximum(lens[np.asarray(r[0], np.int64)] - ctx.k, 0).sum() for r in rects))
    nsurv, forms = measure(ctx, rects, is_rna, reps)
    rec = {"shape": name, "note": note, "k": ctx.k, "rectangles": len(rects), "seeds": ns, "candidates": nc, "survivors": nsurv,
           "survivors_per_candidate": round(nsurv / nc, 2), "bucket_entries_per_seed_batch": entries, "repetitions": reps, "forms": forms}
    for clock in ("wall_ms", "count_pass_device_ms"):
        rec[f"index_slowest_below_seed_fastest_{clock}"] = forms["index"][clock]["max"] < forms["seed"][clock]["min"]
    print(json.dumps({k: v for k, v in rec.items() if k != "forms"}), flush=True)
    print("   ", {f: {c: (forms[f][c]["min"], forms[f][c]["median"], forms[f][c]["max"]) for c in forms[f]} for f in forms}, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_pass_index.json"))
    ap.add_argument("--shapes", default="a,b,c,d")
    a = ap.parse_args()
    assert a.reps >= 5
    want = set(a.shapes.split(","))
    ctx = Context(0)
    records = []
    if want & {"a", "c"}:
        cat, off = draw(256 + 100000, 1000, 1000, 2000, True, 101)
        lens = np.diff(off.astype(np.int64))
        n = len(lens)
        if "a" in want:
            ctx.load_packed(cat, off, 10, True)
            rects = [(np.arange(256, dtype=np.uint32), np.arange(256, n, dtype=np.uint32), 0.4)]
            records.append(shape_record(ctx, "a", rects, False, a.reps, lens, "1 kb cDNA reads, 256 seeds x 1e5 candidates, bit-vector threshold 0.4"))
        if "c" in want:
            ctx.load_packed(cat, off, 11, True)
            rng = np.random.default_rng(7)
            rects = [(rng.choice(n, 8, replace=False).astype(np.uint32), rng.choice(n, 200, replace=False).astype(np.uint32), 0.2) for _ in range(500)]
            records.append(shape_record(ctx, "c", rects, False, a.reps, lens, "500 rectangles of 8 seeds x 200 candidates (the --iso level's shape), threshold 0.2"))
    if want & {"b", "d"}:
        cat, off = draw(1024 + 20000, 4000, 8000, 400, False, 202)
        lens = np.diff(off.astype(np.int64))
        n = len(lens)
        if "b" in want:
            ctx.load_packed(cat, off, 10, False)
            for ns in (256, 1024):
                rects = [(np.arange(ns, dtype=np.uint32), np.arange(1024, n, dtype=np.uint32), 0.2)]
                records.append(shape_record(ctx, f"b{ns}", rects, True, a.reps, lens, f"4 - 8 kb --rna reads, {ns} seeds x 2e4 candidates, bit-vector threshold 0.2 (saturated filter)"))
        if "d" in want:
            ctx.load_packed(cat, off, 6, False)
            rects = [(np.arange(256, dtype=np.uint32), np.arange(1024, n, dtype=np.uint32), 0.2)]
            records.append(shape_record(ctx, "d256", rects, True, a.reps, lens, "shape b with 256 seeds at k = 6, the `polish` setting"))
    ctx.close()
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_count_pass.py", "clocks": {"wall_ms": "host wall time around rattle_hip_debug_evaluate",
                   "count_pass_device_ms": "rattle_hip_kernel_stats, kernel 2: seed = count kernel; index = grouping + build + count"},
                   "shapes": records}, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
