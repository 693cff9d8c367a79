"""Timing of the k-means objective (isle_hip_kmeans_objective) in both spaces on the state the two Lloyd loops leave resident, with
isle_hip_timing: beside the word-space figure k_doc_norms (the plain pass over the same B: a run_lloyds of zero iterations books nothing
else under sparse_assign), beside the projected figure one iteration of Lloyd in span(U) from the final centres (a full assignment pass
over P plus the centre update).  Then both loops once more with the trace on: the trace, its largest increase and the slack
sum_d 2 ISLE_SLACK_REL (|b_d|^2 + max_d |b_d|^2) the bound-based reassignments are granted (hamerly.h).  One JSON line per figure.
Usage: python tools/objective_probe.py [V D k seed reps]   (default: the C2 shape as bench.py generates it)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.synth import make_B
import isle_amd

V, D, k, seed, reps = (int(x) for x in sys.argv[1:6]) if len(sys.argv) >= 6 else (50_000, 1_000_000, 200, 2024, 5)
SLACK_REL = 1e-4  # ISLE_SLACK_REL, isle_amd/csrc/hamerly.h


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(hp, family, fn):
    fn()  # warm-up: buffers reserved
    ms, walls = [], []
    hp.timing_enable(1)
    for _ in range(reps):
        hp.timing_reset()
        t = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t) * 1e3)
        ms.append(hp.timing_get()[family][0])
    launches = hp.timing_get()[family][1]
    hp.timing_enable(0)
    return dict(device_ms_median=round(float(np.median(ms)), 3), device_ms_min=round(float(min(ms)), 3), wall_ms_median=round(float(np.median(walls)), 3),
                launches=launches)


t0 = time.perf_counter()
B = make_B(V, D, k, seed)
hp = isle_amd.HotPath()
hp.upload_csc(B["V"], B["vals"], B["rows"], B["offs"])
hp.compute_block_ks(k, allow_noconv=True)
C0 = hp.kmeans_init_on_projected_space(k, rng_seed=1)["C_lowd"]
emit(shape=[B["V"], B["D"], int(B["offs"][-1])], k=k, setup_s=round(time.perf_counter() - t0, 1))

lp = hp.run_lloyds_on_projected_space(k, C0)
emit(case="objective, projected space, resident inputs", **timed(hp, "lloyd_proj", lambda: hp.kmeans_objective(k, "projected")))
emit(case="one iteration of Lloyd in span(U) from the final centres (full assignment pass over P + centre update)",
     **timed(hp, "lloyd_proj", lambda: hp.run_lloyds_on_projected_space(k, lp["C_lowd"], max_reps=1)))
hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
ls = hp.run_lloyds(k, fetch_centers=False)
emit(case="objective, word space, resident inputs", iters_of_the_loop=ls["iters"], **timed(hp, "sparse_assign", lambda: hp.kmeans_objective(k, "word")))
total = hp.kmeans_objective(k, "word")["total"]

# the trace of both loops and the slack
bn = np.add.reduceat(B["vals"].astype(np.float64) ** 2, B["offs"][:-1].astype(np.int64))
bn[np.diff(B["offs"]) == 0] = 0.0
slack = float((2 * SLACK_REL * (bn + bn.max())).sum())
hp.lloyds_trace(True)
tp = hp.run_lloyds_on_projected_space(k, C0)
hp.left_multiply_by_U(tp["C_lowd"], fetch=False)
ts = hp.run_lloyds(k, fetch_centers=False)
hp.lloyds_trace(False)
for space, tr in (("projected", tp["objective"]), ("word", ts["objective"])):
    inc = float(np.diff(tr).max()) if len(tr) > 1 else 0.0
    emit(case="trace, %s space" % space, trace=[float(x) for x in tr], largest_increase=inc, slack=slack, increase_over_slack=inc / slack)
emit(case="the objective behind the loop is the last trace entry", equal=bool(total == ts["objective"][-1]), total=total)

# last: the floor.  No iteration: under sparse_assign only k_doc_norms is booked
hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
emit(case="k_doc_norms (run_lloyds of zero iterations): the plain pass over B", **timed(hp, "sparse_assign", lambda: hp.run_lloyds(k, max_reps=0, fetch_centers=False)))
hp.close()
