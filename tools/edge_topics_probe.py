"""Timing of the edge-topic stage after the topic model: the device selection and top words against the host paths beside them.
Medians of --reps runs each:

  (a) HotPath.select_edge_pairs on the resident top-two topics: wall, and the device time of the ISLE_T_POST family inside it
  (b) hot_path.select_edge_pairs on fetched top1 / top2, with their fetch (a second construct_topic_model call's copies are not
      separable, so the fetch is timed as isle_hip_topic_model with and without the two arrays) timed as well
  (c) HotPath.edge_top_words(n = 20) for the selected pairs
  (d) HotPath.edge_topics (the V x n model to the host) + hot_path.top_words on that copy

Usage: python tools/edge_topics_probe.py [V D k max_edge_topics] [--reps N] [--out FILE]   (default 100000 10000000 1000 5000: config 5)
The partition is the corpus' planted one (the stage's cost does not depend on how the partition was found).  One JSON line per
measurement, appended to FILE (default profiles/edge_topics_c5.jsonl).  isle_amd/host/edge_select_main --time gives the C++ side's figure."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.synth import Corpus  # noqa: E402
import isle_amd  # noqa: E402
from isle_amd import hot_path as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[100000, 10000000, 1000, 5000])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_topics_c5.jsonl"))
args = ap.parse_args()
V, D, k, max_edge = args.shape


def emit(rec):
    rec = dict(shape=[V, D, k, max_edge], **rec)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def med(xs):
    return round(float(np.median(xs)), 3)


def timed(fn):
    """(wall ms, ISLE_T_POST device ms, result) of one call."""
    hp.timing_reset()
    t0 = time.perf_counter()
    out = fn()
    hp.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, float(hp.timing_get()["post"][0]), out


c = Corpus(V, D, k, 1)
cnt, rows, offs = c.A()
hp = isle_amd.HotPath(0)
hp.upload_counts(V, cnt, rows, offs)
hp.threshold(k)
oc = hp.get_B()["original_cols"].astype(np.int64)
hp.find_catchwords(k, H.catchword_rank(D, k), assign=c.planted()[oc].astype(np.uint32), fetch_thresholds=False)
rank_thr = H.model_rank_threshold(D, k)
tm = hp.construct_topic_model(k, rank_thr, D, fetch_sums=False)
del cnt, rows, offs
hp.timing_enable(True)

runs = [timed(lambda: hp.select_edge_pairs(max_edge)) for _ in range(args.reps + 1)][1:]
pairs, info = runs[-1][2]
emit(dict(what="device_select", wall_ms=med([r[0] for r in runs]), post_ms=med([r[1] for r in runs]), selected=int(pairs.shape[0]), **info))

t1, t2 = np.empty(D, np.int32), np.empty(D, np.int32)
lib, h = hp._lib, hp._h
fetch = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    hp._chk(lib.isle_hip_topic_model(h, k, rank_thr, None, None, None, None, None))
    base = time.perf_counter() - t0
    t0 = time.perf_counter()
    hp._chk(lib.isle_hip_topic_model(h, k, rank_thr, None, None, t1.ctypes.data_as(C.c_void_p), t2.ctypes.data_as(C.c_void_p), None))
    fetch.append((time.perf_counter() - t0 - base) * 1e3)
host = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    want = H.select_edge_pairs(t1, t2, max_edge)
    host.append((time.perf_counter() - t0) * 1e3)
emit(dict(what="host_select", wall_ms=med(host), fetch_ms=med(fetch), identical=bool(np.array_equal(want, pairs))))

runs = [timed(lambda: hp.edge_top_words(pairs, 20)) for _ in range(args.reps + 1)][1:]
ids = runs[-1][2][0]
emit(dict(what="device_edge_top_words", n=20, wall_ms=med([r[0] for r in runs]), post_ms=med([r[1] for r in runs])))

edge_ms, top_ms = [], []
for _ in range(args.reps):
    t0 = time.perf_counter()
    E = hp.edge_topics(pairs[:, :2], H.EDGE_TOPIC_PRIMARY_RATIO)
    t1_ = time.perf_counter()
    want_ids = H.top_words(E, 20)
    edge_ms.append((t1_ - t0) * 1e3)
    top_ms.append((time.perf_counter() - t1_) * 1e3)
emit(dict(what="host_edge_top_words", n=20, edge_topics_ms=med(edge_ms), top_words_ms=med(top_ms), identical=bool(np.array_equal(want_ids, ids))))
hp.close()
