"""Timing of the cluster-average topic model (isle_hip_avg_topic_model), device top-word selection (isle_hip_model_top_words) of the
catch and average models, and topic diversity (isle_hip_topic_diversity), with the catch model (isle_hip_topic_model, whose
accumulation is fp32 atomics over the same entries) at the same size for comparison.  A planted corpus with the planted partition.
One JSON line per case.
Usage: python tools/avg_model_probe.py [V D k reps]   (default: config 3 shape)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.synth import Corpus
import isle_amd
from isle_amd.hot_path import catchword_rank, model_rank_threshold

V, D, k, reps = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (100000, 10000000, 1000, 5)


def measure(hp, case, fn, **extra):
    fn()  # warm-up
    hp.timing_enable(1)
    walls, devs = [], []
    for _ in range(reps):
        hp.timing_reset()
        t = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t) * 1e3)
        devs.append(hp.timing_get()["post"][0])
    launches = hp.timing_get()["post"][1]
    hp.timing_enable(0)
    print(json.dumps(dict({"case": case, "shape": [V, D], "nnz_A": nnz, "topics": k, "ms_call_median": round(float(np.median(walls)), 3),
                           "ms_call_min": round(float(min(walls)), 3), "device_ms_median": round(float(np.median(devs)), 3),
                           "launches": launches}, **extra)), flush=True)


t0 = time.perf_counter()
c = Corpus(V, D, k, 31337)
cnt, rows, offs = c.A_views()
nnz = int(offs[-1])
hp = isle_amd.HotPath()
hp.upload_counts(V, cnt, rows, offs)
hp.threshold(k)
oc = np.empty(hp.D, np.uint64)  # original_cols only: no host copy of B
hp._chk(hp._lib.isle_hip_get_B(hp._h, None, None, None, oc.ctypes.data_as(C.c_void_p), None))
assign = c.planted()[oc.astype(np.int64)].astype(np.uint32)
hp.find_catchwords(k, catchword_rank(D, k), assign=assign, fetch_thresholds=False)
print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1)}), flush=True)

lib, h = hp._lib, hp._h
measure(hp, "catch topic model (isle_hip_topic_model: sums, thresholds, fp32 atomic accumulation)",
        lambda: hp._chk(lib.isle_hip_topic_model(h, k, model_rank_threshold(D, k), None, None, None, None, None)))
measure(hp, "average topic model (exact fixed-point accumulation)", lambda: hp._chk(lib.isle_hip_avg_topic_model(h, k, None)),
        model_bytes=V * k * 4, accumulator_bytes=V * k * 16)
ids = np.empty((k, 10), np.uint32)
for name, which in (("catch", 0), ("avg", 1)):
    measure(hp, "top words n=10, %s model" % name, lambda: hp._chk(lib.isle_hip_model_top_words(h, which, None, V, k, 10, ids.ctypes.data_as(C.c_void_p), None)))
    dist = np.empty(k, np.float64)
    avg = C.c_double()
    measure(hp, "topic diversity, %s model" % name,
            lambda: hp._chk(lib.isle_hip_topic_diversity(h, which, k, dist.ctypes.data_as(C.c_void_p), C.byref(avg))))
    print(json.dumps({"model": name, "avg_diversity": avg.value}), flush=True)
hp.close()
