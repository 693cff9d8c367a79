#!/usr/bin/env python3
"""Timing probe for isle_hip_score_docs on the configuration-2 corpus (50 k words, 1 M resident documents) with k = 200, set up as
tools/topic_prevalence_probe.py sets it up; medians of 5 in one process after a warm-up, with min - max:
  (a) HotPath.score_docs on the resident count matrix with the resident inference entries ("log", normalise, a floor), once with the
      default entries of infer_resident (weights above 1 / k: one or two topics a row) and once with the min_weight = 0 entries: the
      call's wall time and its device time (the growth of ISLE_T_INFER: the pack of the model, the row pass and the walk), and the bytes
      the walk touches, 8 per entry of A + the weight rows (8 per row and 8 per weight entry) + 4 per (entry, stored topic) of model,
      as a share of what 8 TB/s would move in the device time;
  (b) infer_resident of the same documents in the same process: the sibling;
  (c) the path a user has without the call, on the default entries: A and the entries fetched (timed apart), then z at every nonzero and
      the sums per document in numpy, run ONCE, and the largest relative difference between its per-document scores and the device's.
One JSON line per measurement, written as it is taken; nothing is expected in advance.
  score_docs_probe.py [out.jsonl] [docs]      (default: profiles/score_docs_c2.jsonl, 1 000 000 documents)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isle_amd import HotPath  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tools.synth import Corpus  # noqa: E402

REPS = 5
PEAK_BYTES_PER_MS = 8e12 / 1e3
FLOOR = 1e-12


def timed(fn, reps=REPS):
    ms, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, last


def stats(prefix, ms):
    return {prefix + "_median": float(np.median(ms)), prefix + "_min": float(min(ms)), prefix + "_max": float(max(ms))}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "score_docs_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    t0 = time.perf_counter()
    c = Corpus(V, D, k, 1)
    cnt, rows, offs = c.A()
    hp = HotPath(0)
    hp.timing_enable(True)
    hp.upload_counts(V, cnt, rows, offs)
    hp.threshold(k)
    assign = c.planted()[hp.get_B()["original_cols"].astype(np.int64)].astype(np.uint32)
    hp.find_catchwords(k, O.catchword_rank(D, k), assign=assign, fetch_thresholds=False)
    tm = hp.construct_topic_model(k, O.model_rank_threshold(D, k), D, fetch_sums=False)
    shape = dict(V=V, k=k, docs=D, nnz=int(cnt.size), reps=REPS)
    out = open(out_path, "w")

    def emit(**kw):
        kw.update(shape)
        text = json.dumps(kw)
        out.write(text + "\n")
        out.flush()
        print(text, flush=True)

    emit(what="set-up: corpus, upload, threshold, catchwords, topic model", wall_s=time.perf_counter() - t0)
    per_doc = np.diff(offs).astype(np.float64)
    kept = {}
    for name, minw in (("default entries (weight > 1 / k)", None), ("min_weight = 0 entries", 0.0)):
        dev = []

        def infer():
            before = hp.timing_get()["infer"][0]
            res = hp.infer_resident("catch", min_weight=minw, fetch_entries=False)
            dev.append(hp.timing_get()["infer"][0] - before)
            return res

        infer()
        dev.clear()
        wall, inf = timed(infer)
        line = dict(entries=int(inf["nentries"]), nconverged=int(inf["nconverged"]))
        line.update(stats("wall_ms", wall))
        line.update(stats("device_ms", dev))
        emit(what="infer_resident, %s: the sibling" % name, **line)
        woff = hp.infer_entries(D, inf["nentries"])[0]
        pairs = float((per_doc * np.diff(woff)).sum())  # (entry, stored topic) pairs: the model floats the walk gathers
        touched = 8 * cnt.size + 8 * (D + 1) + 8 * int(inf["nentries"]) + 4 * pairs
        dev = []

        def score():
            before = hp.timing_get()["infer"][0]
            res = hp.score_docs("catch", "infer", "resident", measure="log", normalise=True, floor=FLOOR)
            dev.append(hp.timing_get()["infer"][0] - before)
            return res

        score()
        dev.clear()
        wall, got = timed(score)
        kept[minw] = got
        line = dict(weight_entries=int(inf["nentries"]), model_floats_gathered=pairs, bytes_touched=touched,
                    share_of_8_TB_per_s=touched / (float(np.median(dev)) * PEAK_BYTES_PER_MS), perplexity=got["perplexity"],
                    total_tokens=got["total_tokens"], floored=int(got["floored"].sum()), unscored_entries=int(got["unscored_entries"].sum()))
        line.update(stats("wall_ms", wall))
        line.update(stats("device_ms", dev))
        emit(what="score_docs on the resident A, %s, log, normalise, floor %g (device time includes the pack of the model)" % (name, FLOOR), **line)

    # the path a user has today, on the default entries: fetch, then numpy, once
    inf = hp.infer_resident("catch", fetch_entries=False)
    f_ms, (a_cnt, a_rows, a_offs) = timed(hp.get_A, 1)
    e_ms, (woff, wtp, wwt) = timed(lambda: hp.infer_entries(D, inf["nentries"]), 1)
    M = tm["model"]
    t1 = time.perf_counter()
    doc = np.repeat(np.arange(D, dtype=np.int64), np.diff(a_offs))
    nw = np.diff(woff)
    s = np.bincount(np.repeat(np.arange(D, dtype=np.int64), nw), weights=wwt.astype(np.float64), minlength=D)
    z = np.zeros(a_cnt.size, np.float64)
    for j in range(int(nw.max()) if D else 0):
        have = np.nonzero(nw[doc] > j)[0]
        d = doc[have]
        idx = woff[:-1][d] + j
        z[have] += M[a_rows[have], wtp[idx]].astype(np.float64) * (wwt[idx].astype(np.float64) / s[d])
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = np.isfinite(z) & (z >= 0) & ((z > 0) | (FLOOR > 0))
        term = np.where(ok, a_cnt.astype(np.float64) * np.log(np.maximum(z, FLOOR)), 0.0)
    host = np.bincount(doc, weights=term, minlength=D)
    host_ms = (time.perf_counter() - t1) * 1e3
    got = kept[None]["score"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(host != 0, np.abs(got - host) / np.abs(host), np.abs(got))
    emit(what="the host path on the default entries: A and the entries fetched, then z at every nonzero and the sums in numpy (run once)",
         fetch_A_ms=f_ms[0], fetch_entries_ms=e_ms[0], numpy_once_ms=host_ms, largest_relative_difference_of_a_document_score=float(np.nanmax(rel)),
         topics_per_row_max=int(nw.max()))
    emit(what="summary", config3="unmeasured: 10 M documents at k = 1000 were not run",
         part_of_a_wave_per_document="unmeasured: a document is owned by a whole wave; a part of a wave was not built",
         dense_rows="unmeasured: a dense form of the walk for dense weight rows was not built",
         lds_tile="unmeasured: 256 staged weights; no other tile size was timed", several_ranks="unmeasured: no collective in the call")
    hp.close()
    out.close()


if __name__ == "__main__":
    main()
