#!/usr/bin/env python3
"""Timing probe for isle_hip_topic_prevalence on the configuration-2 corpus (50 k words, 1 M resident documents) with k = 200, set up as
tools/similar_docs_probe.py sets it up; medians of 5 in one process after a warm-up, with min - max:
  (a) HotPath.topic_prevalence on the catchword sums and on the inference entries, without labels and with 50 random labels, each with and
      without normalise: the call's wall time and its device time (the growth of ISLE_T_POST for "sums", of ISLE_T_INFER for "infer"), and
      the bytes of entries the kernels read (offsets, topics and weights, once by the row pass and once per topic tile by level 0) as a
      share of what 8 TB/s would move in the device time;
  (b) topic_top_docs(n = 10) on the same entries in the same process: the sibling that reads them where they lie;
  (c) the host path a user has without the call: the entries fetched (timed apart), then np.add.at into a (groups, k) table of doubles,
      run ONCE where it takes seconds, and the largest relative difference between its sums (a sequential order) and the device's.
One JSON line per measurement, written as it is taken; nothing is expected in advance.
  topic_prevalence_probe.py [out.jsonl] [docs]      (default: profiles/topic_prevalence_c2.jsonl, 1 000 000 documents)"""
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "topic_prevalence_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    G = 50
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
    inf = hp.infer_resident("catch", fetch_entries=False)
    shape = dict(V=V, k=k, docs=D, reps=REPS)
    out = open(out_path, "w")

    def emit(**kw):
        kw.update(shape)
        text = json.dumps(kw)
        out.write(text + "\n")
        out.flush()
        print(text, flush=True)

    entries = {"sums": int(tm["num_sums"]), "infer": int(inf["nentries"])}
    emit(what="set-up: corpus, upload, threshold, catchwords, topic model, resident inference", wall_s=time.perf_counter() - t0,
         sums_entries=entries["sums"], infer_entries=entries["infer"])
    labels = np.random.default_rng(3).integers(0, G, D).astype(np.uint32)
    fams = {"sums": "post", "infer": "infer"}
    device = {}

    for source in ("sums", "infer"):
        fam = fams[source]
        hp.topic_prevalence(source)  # first-launch costs stay out of the medians
        for lab, groups in ((None, 1), (labels, G)):
            for normalise in (False, True):
                dev = []

                def call():
                    before = hp.timing_get()[fam][0]
                    res = hp.topic_prevalence(source, lab, groups, normalise)
                    dev.append(hp.timing_get()[fam][0] - before)
                    return res

                call()
                dev.clear()
                wall, got = timed(call)
                device[source, groups, normalise] = got
                # the entries' bytes the kernels read: the row pass and level 0 each take offsets (8), topics (4) and weights (4) once (k <= one tile)
                read = 2 * (8 * (D + 1) + 8 * entries[source]) + (4 * D if lab is not None else 0) + (8 * D if normalise else 0)
                line = dict(source=source, groups=groups, labels=lab is not None, normalise=normalise, entries=entries[source], bytes_read=read,
                            share_of_8_TB_per_s=read / (float(np.median(dev)) * PEAK_BYTES_PER_MS), docs_counted=int(got["docs"].sum()))
                line.update(stats("wall_ms", wall))
                line.update(stats("device_ms", dev))
                emit(what="topic_prevalence from %s, %s, %s" % (source, "%d random labels" % G if lab is not None else "no labels",
                                                                "normalise" if normalise else "plain"), **line)
        hp.topic_top_docs(10, source)
        dev = []

        def sibling():
            before = hp.timing_get()[fam][0]
            hp.topic_top_docs(10, source)
            dev.append(hp.timing_get()[fam][0] - before)

        wall, _ = timed(sibling)
        line = dict(source=source)
        line.update(stats("wall_ms", wall))
        line.update(stats("device_ms", dev))
        emit(what="topic_top_docs(n = 10) from %s: the sibling that reads the same entries" % source, **line)

    # the host path a user has today: fetch, then np.add.at, once
    def fetch_sums():
        off, tp, va = np.empty(D + 1, np.int64), np.empty(tm["num_sums"], np.uint32), np.empty(tm["num_sums"], np.float32)
        hp._chk(hp._lib.isle_hip_get_doc_topic_sums(hp._h, off.ctypes.data, tp.ctypes.data, va.ctypes.data))
        return off, tp, va

    for source, fetch in (("sums", fetch_sums), ("infer", lambda: hp.infer_entries(D, inf["nentries"]))):
        f_ms, (off, tp, va) = timed(fetch)
        for lab, groups in ((None, 1), (labels, G)):
            t1 = time.perf_counter()
            row = np.repeat(np.arange(D, dtype=np.int64), np.diff(off))
            g = np.zeros(tp.size, np.int64) if lab is None else lab[row].astype(np.int64)
            total = np.zeros((groups, k), np.float64)
            np.add.at(total, (g, tp.astype(np.int64)), va.astype(np.float64))
            count = np.zeros((groups, k), np.uint64)
            np.add.at(count, (g, tp.astype(np.int64)), 1)
            host_ms = (time.perf_counter() - t1) * 1e3
            got = device[source, groups, False]
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(total > 0, np.abs(got["sum"] - total) / total, 0.0)
            line = dict(source=source, groups=groups, labels=lab is not None, entries=int(tp.size), np_add_at_once_ms=host_ms,
                        same_counts_as_the_device=bool(np.array_equal(count, got["count"])), largest_relative_difference_of_the_sums=float(rel.max()))
            line.update(stats("fetch_entries_ms", f_ms))
            emit(what="the host path: the entries fetched, then np.add.at of sums and counts (run once)", **line)
    emit(what="summary", several_ranks="refused by the call", config3="unmeasured: 10 M documents at k = 1000 were not run",
         part_of_a_wave_as_owner="unmeasured: a block of 64 list positions is owned by a whole wave; a part of a wave was not built",
         other_tiles="unmeasured: 1024 topics per table (k = 200 is one tile); no other tile size was timed")
    hp.close()
    out.close()


if __name__ == "__main__":
    main()
