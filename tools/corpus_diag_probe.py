"""Timing of the trainer's corpus diagnostics on the device (isle_hip_log_combinatorial, isle_hip_distinct_top_five) at full size: the count
matrix A of a synthetic corpus uploaded, then each diagnostic timed as a call (host clock around a call that ends in a synchronise) and
as device time of the post family (the library's timer).  One JSON line per case.  Floors at the measured 6.3 TB/s of HBM: log-combinatorial
one read of the counts and offsets and one write of the result; top five one read of the normalised values and offsets (together about
8.8 GB at config 3).  The kernels do more: the counts are read twice (word counts, then ordered sums), the normalised values are rewritten
on every call, and the tuples go through 20 radix passes.
Usage: python tools/corpus_diag_probe.py [V D K reps]   (default: config 3 shape, 100 000 x 10 M)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.synth import Corpus
import isle_amd

V, D, K, reps = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (100000, 10000000, 1000, 5)
HBM = 6.3e12


def measure(hp, case, fn, floor_bytes, extra):
    out = fn()  # warm-up (code objects, buffers)
    hp.timing_enable(1)
    walls = []
    for _ in range(reps):
        hp.timing_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
    dev_ms, launches = hp.timing_get()["post"]
    hp.timing_enable(0)
    floor_ms = floor_bytes / HBM * 1e3
    rec = {"case": case, "shape": [V, D], "nnz_A": nnz, "ms_call_median": round(float(np.median(walls)), 3), "ms_call_min": round(float(min(walls)), 3),
           "device_ms_post_family": round(dev_ms, 3), "launches": launches, "floor_bytes": int(floor_bytes), "floor_ms": round(floor_ms, 3),
           "device_over_floor": round(dev_ms / floor_ms, 2)}
    rec.update(extra(out))
    print(json.dumps(rec), flush=True)


t0 = time.perf_counter()
c = Corpus(V, D, K, 31337)
cnt, rows, offs = c.A_views()
nnz = int(offs[-1])
hp = isle_amd.HotPath()
hp.upload_counts(V, cnt, rows, offs)
print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
offs_bytes = 8 * (D + 1)
measure(hp, "log_combinatorial", hp.log_combinatorial, 4 * nnz + offs_bytes + 4 * D,
        lambda o: {"finite": int(np.isfinite(o).sum()), "mean": float(np.mean(o, dtype=np.float64))})
measure(hp, "distinct_top_five_sets (8 m, one device pass)", hp.distinct_top_five_sets, 4 * nnz + offs_bytes,
        lambda o: {"num_quintuples": o["num_quintuples"], "runs": int(o["run_lengths"].size), "counts": {str(k): v for k, v in o["counts"].items()}})
hp.close()
