"""Records the random stream's states of bench.py's workloads into bench_workload_states.json, so that bench.py can draw a workload
segment by segment on several cores (bench.make_workload_fast) instead of ~100 s on one.  Run it again after a change to
rattle_amd/synth.py or to numpy's generators: bench.py checks every segment against the recorded states and draws in one piece
where they do not match.
usage: python tools/bench_workload_states.py   (the default workload and the --iso one, 1e6 reads each)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

WORKLOADS = [  # (reads, genes, seed, isoforms): bench.py's defaults without and with --iso
    (1000000, 1000000 // 200, 20260929, 1),
    (1000000, 1000000 // 600, 20260929, 3),
]

if __name__ == "__main__":
    out = {}
    for n, genes, seed, iso in WORKLOADS:
        out[bench._workload_key(n, genes, seed, iso)] = bench.record_workload_states(n, genes, seed, iso)
        print(bench._workload_key(n, genes, seed, iso), len(out[bench._workload_key(n, genes, seed, iso)]), "states", file=sys.stderr)
    with open(bench.STATES_FILE, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
