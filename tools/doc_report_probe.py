#!/usr/bin/env python3
"""Timing probe for isle_hip_doc_report_text on the configuration-2 corpus (50 k words, 1 M documents) with k = 200, medians of 5 in
one process, for each of the four kinds ("catchwords": DocCatchword.tsv, "topic_sums": DocTopicCatchwordSums.tsv, "topic_sums_by_doc":
the same lines in resident order, "top_two": TopTwoTopicsPerDoc.txt):
  (a) HotPath.write_doc_report into a local file;
  (b) the path before the device formatter: fetching the arrays the file prints (construct_topic_model with its sums, top-two topics;
      find_catchwords with the catchword map; A is already on the host, its normalised values are computed there) and the host loops
      on them into a local file.  The host loops here are the vectorised numpy restatements of tests/test_doc_report_cpu.py, NOT the
      C++ loops of trainer_hip.h: those are timed by isle_amd/host/doc_report_main --time on a corpus given as a tdf file;
  (c) the formatter's device time: the growth of ISLE_T_POST over the write_doc_report call.
One JSON line per measurement; no ratio is expected in advance.
  doc_report_probe.py [out.jsonl] [docs]      (default: profiles/doc_report_c2.jsonl, 1 000 000 documents)"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from isle_amd import HotPath  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tools.synth import Corpus  # noqa: E402

REPS = 5
KINDS = ("catchwords", "topic_sums", "topic_sums_by_doc", "top_two")


def median_ms(fn):
    ms, last = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        last = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms, last


def main():
    from test_doc_report_cpu import catchwords_text, top_two_text, topic_sums_text
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "doc_report_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    c = Corpus(V, D, k, 1)
    cnt, rows, offs = c.A()
    hp = HotPath(0)
    hp.timing_enable(True)
    hp.upload_counts(V, cnt, rows, offs)
    info = hp.threshold(k)
    assign = c.planted()[hp.get_B()["original_cols"].astype(np.int64)].astype(np.uint32)
    r, rt = O.catchword_rank(D, k), O.model_rank_threshold(D, k)
    shape = dict(V=V, k=k, docs=D, nnz=int(offs[-1]), reps=REPS)
    lines = []

    def emit(**kw):
        kw.update(shape)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    fetch_cw_ms, fetch_cw_all, got = median_ms(lambda: hp.find_catchwords(k, r, assign=assign, fetch_thresholds=False))
    fetch_tm_ms, fetch_tm_all, tm = median_ms(lambda: hp.construct_topic_model(k, rt, D))
    left_tm_ms, left_tm_all, _ = median_ms(lambda: hp.construct_topic_model(k, rt, D, fetch_sums=False))
    emit(what="find_catchwords with the catchword map fetched", wall_ms_median=fetch_cw_ms, wall_ms=fetch_cw_all, num_catchwords=got["num_catchwords"])
    emit(what="construct_topic_model with the sums fetched / without", fetched_wall_ms_median=fetch_tm_ms, fetched_wall_ms=fetch_tm_all,
         left_wall_ms_median=left_tm_ms, left_wall_ms=left_tm_all, num_sums=tm["num_sums"])
    t0 = time.perf_counter()
    nv = O.post_normalize(offs, cnt, info["avg_doc_sz"])
    nv_ms = (time.perf_counter() - t0) * 1e3
    host = {"catchwords": lambda: catchwords_text(got["catch_topic"], offs, rows, nv),
            "topic_sums": lambda: topic_sums_text(tm["dts_off"], tm["dts_topic"], tm["dts_val"]),
            "topic_sums_by_doc": lambda: topic_sums_text(tm["dts_off"], tm["dts_topic"], tm["dts_val"], by_doc=True),
            "top_two": lambda: top_two_text(tm["top1"], tm["top2"])}
    with tempfile.TemporaryDirectory() as tmp:
        for kind in KINDS:
            hp.doc_report_size(kind)   # first-launch costs stay out of the medians
            path, host_path = os.path.join(tmp, kind + ".dev"), os.path.join(tmp, kind + ".host")
            dev_ms = []

            def write():
                before = hp.timing_get()["post"][0]
                res = hp.write_doc_report(path, kind)
                dev_ms.append(hp.timing_get()["post"][0] - before)
                return res

            def host_write():
                text = host[kind]()
                with open(host_path, "wb") as f:
                    f.write(text)
                return len(text)

            a_ms, a_all, (nbytes, nlines) = median_ms(write)
            b_ms, b_all, host_bytes = median_ms(host_write)
            same = host_bytes == nbytes and open(host_path, "rb").read() == open(path, "rb").read()
            emit(what="text of %s" % kind, kind=kind, text_bytes=nbytes, text_lines=nlines, a_write_doc_report_ms=a_ms, a_write_doc_report_all_ms=a_all,
                 b_numpy_host_loop_ms=b_ms, b_numpy_host_loop_all_ms=b_all, b_normalise_on_host_ms=nv_ms if kind == "catchwords" else 0.0,
                 c_formatter_device_ms_median=float(np.median(dev_ms)), c_formatter_device_ms=dev_ms, same_bytes_as_host_loop=bool(same))
            os.remove(path)
            os.remove(host_path)
    emit(what="summary", config3="unmeasured: 10 M documents at k = 1000 were not run")
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
