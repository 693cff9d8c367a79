#!/usr/bin/env python3
"""Timing probe for isle_hip_similar_docs on the configuration-2 corpus (50 k words, 1 M resident documents) with k = 200, set up as
tools/top_docs_probe.py sets it up; n = 10, medians of 5 in one process after a warm-up, with min - max:
  (a) HotPath.similar_docs for Q = 1, 8, 64 queries given as rows, on the catchword sums and on the inference entries, under each measure:
      the call's wall time and its device time (the growth of ISLE_T_POST for "sums", of ISLE_T_INFER for "infer"), the candidate pairs;
  (b) the two homes of the query table, alternating, at Q = 64 (k = 200: a 51 KiB table fits both): the measurement the threshold of
      route_simdocs_table lacks;
  (c) topic_top_docs(n = 10) on the same entries in the same process: the sibling whose selection this call shares;
  (d) the host path a user has without the call: the entries fetched (timed apart), then the numpy rule of tests/simdocs_rule.py, run ONCE
      per source at Q = 8 under cosine, and compared with the device's lists.
One JSON line per measurement, written as it is taken; no ratio is expected in advance.
  similar_docs_probe.py [out.jsonl] [docs]      (default: profiles/similar_docs_c2.jsonl, 1 000 000 documents)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from isle_amd import HotPath  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tools.synth import Corpus  # noqa: E402

REPS = 5


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
    import simdocs_rule as sr
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "similar_docs_c2.jsonl")
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
    inf = hp.infer_resident("catch", fetch_entries=False)
    shape = dict(V=V, k=k, docs=D, n=10, reps=REPS)
    out = open(out_path, "w")

    def emit(**kw):
        kw.update(shape)
        text = json.dumps(kw)
        out.write(text + "\n")
        out.flush()
        print(text, flush=True)

    emit(what="set-up: corpus, upload, threshold, catchwords, topic model, resident inference", wall_s=time.perf_counter() - t0,
         sums_entries=int(tm["num_sums"]), infer_entries=int(inf["nentries"]))
    qrows = np.random.default_rng(3).choice(D, 64, replace=False).astype(np.uint64)
    fams = {"sums": "post", "infer": "infer"}

    def measure(source, Q, name, form="auto"):
        fam, dev = fams[source], []

        def call():
            before = hp.timing_get()[fam][0]
            res = hp.similar_docs(qrows[:Q], 10, source, measure=name)
            dev.append(hp.timing_get()[fam][0] - before)
            return res

        hp.simdocs_table_form(form)
        wall, got = timed(call)
        line = dict(source=source, queries=Q, measure=name, table=form, candidate_pairs=int(got["candidates"].sum()))
        line.update(stats("wall_ms", wall))
        line.update(stats("device_ms", dev))
        return line, got

    for source in ("sums", "infer"):
        hp.similar_docs(qrows[:1], 10, source)  # first-launch costs stay out of the medians
        for Q in (1, 8, 64):
            for name in sr.MEASURES:
                hp.similar_docs(qrows[:Q], 10, source, measure=name)
                line, _ = measure(source, Q, name)
                emit(what="similar_docs from %s, Q = %d, %s" % (source, Q, name), **line)
        # the table's two homes, alternating
        per = {"lds": dict(wall=[], dev=[]), "global": dict(wall=[], dev=[])}
        for form in ("lds", "global"):
            hp.simdocs_table_form(form)
            hp.similar_docs(qrows, 10, source)
        for _ in range(REPS):
            for form in ("lds", "global"):
                hp.simdocs_table_form(form)
                before = hp.timing_get()[fams[source]][0]
                t1 = time.perf_counter()
                hp.similar_docs(qrows, 10, source)
                per[form]["wall"].append((time.perf_counter() - t1) * 1e3)
                per[form]["dev"].append(hp.timing_get()[fams[source]][0] - before)
        hp.simdocs_table_form("auto")
        line = dict(source=source, queries=64, measure="cosine", table_bytes=k * 64 * 4)
        for form in per:
            line.update(stats(form + "_wall_ms", per[form]["wall"]))
            line.update(stats(form + "_device_ms", per[form]["dev"]))
        emit(what="the query table's two homes, alternating, from %s" % source, **line)
        # the sibling
        hp.topic_top_docs(10, source)
        dev = []

        def sibling():
            before = hp.timing_get()[fams[source]][0]
            hp.topic_top_docs(10, source)
            dev.append(hp.timing_get()[fams[source]][0] - before)

        wall, _ = timed(sibling)
        line = dict(source=source)
        line.update(stats("wall_ms", wall))
        line.update(stats("device_ms", dev))
        emit(what="topic_top_docs(n = 10) from %s: the sibling whose selection similar_docs shares" % source, **line)

    # the host path a user has today: fetch, then the numpy rule, once
    def fetch_sums():
        off, tp, va = np.empty(D + 1, np.int64), np.empty(tm["num_sums"], np.uint32), np.empty(tm["num_sums"], np.float32)
        hp._chk(hp._lib.isle_hip_get_doc_topic_sums(hp._h, off.ctypes.data, tp.ctypes.data, va.ctypes.data))
        return off, tp, va

    for source, fetch in (("sums", fetch_sums), ("infer", lambda: hp.infer_entries(D, inf["nentries"]))):
        f_ms, (off, tp, va) = timed(fetch)
        got = hp.similar_docs(qrows[:8], 10, source, measure="cosine")
        t1 = time.perf_counter()
        want = sr.rule(sr.Case(source, k, 10, 0, (off, tp, va), query_rows=qrows[:8]), sr.COSINE)
        rule_ms = (time.perf_counter() - t1) * 1e3
        same = all(np.array_equal(got[f].view(np.uint32) if f == "scores" else got[f], want[f]) for f in ("docs", "scores", "counts", "candidates"))
        line = dict(source=source, queries=8, measure="cosine", entries=int(tp.size), numpy_rule_once_ms=rule_ms, same_lists_as_the_rule=bool(same))
        line.update(stats("fetch_entries_ms", f_ms))
        emit(what="the host path: the entries fetched, then the numpy rule of tests/simdocs_rule.py (run once)", **line)
    emit(what="summary", several_ranks="unmeasured", config3="unmeasured: 10 M documents at k = 1000 were not run",
         two_pass_against_dense_block="unmeasured: the walk is done twice; a dense rows x Qp block compacted was not built")
    hp.close()
    out.close()


if __name__ == "__main__":
    main()
