"""Timing of the device topic coherence (isle_hip_topic_coherence) at full size: the top words of the device topic model of a planted
corpus (catchwords + topic model with the planted partition), and of its edge model.  One JSON line per case.
Usage: python tools/coherence_probe.py [V D k edge_topics M reps]   (default: config 3 shape, 5000 edge topics as in config 5, M = 5)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.synth import Corpus
import isle_amd
from isle_amd.hot_path import catchword_rank, model_rank_threshold, select_edge_pairs, top_words

V, D, k, n_edge, M, reps = (int(x) for x in sys.argv[1:7]) if len(sys.argv) >= 7 else (100000, 10000000, 1000, 5000, 5, 5)


def counters(tw):
    """|U|, |P| and the passes over A the library makes for them (its LDS tile: coherence.hip COH_LDS, CW * HCAP, bitmap bound)."""
    U = np.unique(tw)
    loc = np.searchsorted(U, tw).astype(np.int64)
    m = tw.shape[1]
    keys = [np.minimum(loc[:, i], loc[:, j]) * U.size + np.maximum(loc[:, i], loc[:, j]) for i in range(1, m) for j in range(i)]
    P = np.unique(np.concatenate(keys)).size if keys else 0
    nwords = 0 if V > 131072 else (V + 31) // 32
    tile = (160 * 1024 - 512 - 4 * (2 * nwords + 16 * 256)) // 4
    return int(U.size), int(P), int(-(-(U.size + P) // tile))


def measure(hp, case, tw):
    hp.topic_coherence(tw, fetch_counts=False)  # warm-up
    hp.timing_enable(1)
    walls = []
    for _ in range(reps):
        hp.timing_reset()
        t = time.perf_counter()
        out = hp.topic_coherence(tw)
        walls.append((time.perf_counter() - t) * 1e3)
    dev_ms, launches = hp.timing_get()["post"]
    hp.timing_enable(0)
    nU, nP, passes = counters(tw)
    coh = out["coherence"]
    print(json.dumps({"case": case, "shape": [V, D], "nnz_A": nnz, "topics": int(tw.shape[0]), "M": int(tw.shape[1]),
                      "ms_call_median": round(float(np.median(walls)), 3), "ms_call_min": round(float(min(walls)), 3),
                      "device_ms_post_family": round(dev_ms, 3), "launches": launches, "U": nU, "P": nP, "passes_over_A": passes,
                      "finite_topics": int(np.isfinite(coh).sum()), "avg_coherence_finite": float(np.nanmean(np.where(np.isfinite(coh), coh, np.nan)))}),
          flush=True)


t0 = time.perf_counter()
c = Corpus(V, D, k, 31337)
cnt, rows, offs = c.A_views()
nnz = int(offs[-1])
hp = isle_amd.HotPath()
hp.upload_counts(V, cnt, rows, offs)
hp.threshold(k)
oc = np.empty(hp.D, np.uint64)  # original_cols only: no host copy of B
hp._chk(hp._lib.isle_hip_get_B(hp._h, None, None, None, oc.ctypes.data_as(C.c_void_p), None))
oc = oc.astype(np.int64)
assign = c.planted()[oc].astype(np.uint32)
hp.find_catchwords(k, catchword_rank(D, k), assign=assign, fetch_thresholds=False)
tm = hp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
measure(hp, "topic model k=%d" % k, top_words(tm["model"], M))
if n_edge:
    pairs = select_edge_pairs(tm["top1"], tm["top2"], n_edge)
    E = hp.edge_topics(pairs[:, :2])
    del tm
    measure(hp, "edge model (%d edge topics)" % pairs.shape[0], top_words(E, M))
hp.close()
