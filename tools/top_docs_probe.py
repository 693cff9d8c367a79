#!/usr/bin/env python3
"""Timing probe for isle_hip_topic_top_docs on the configuration-2 corpus (50 k words, 1 M resident documents) with k = 200, at n = 10 and
n = 256, medians of 5 in one process after a warm-up, for both resident sources:
  (a) HotPath.topic_top_docs: the call's wall time and its device time (the growth of ISLE_T_POST for "sums", of ISLE_T_INFER for "infer");
  (b) the only way there was before the call existed: the entries fetched (isle_hip_get_doc_topic_sums / isle_hip_get_infer_entries), then
      the numpy rule of tests/topdocs_rule.py on the host (a lexsort of all entries); the two parts are timed apart;
  (c) for the sums, the wall time of write_doc_report("topic_sums"), the sorted report that held the topic-major view until now.
The bins' two homes (LDS up to 64 topics, global memory beyond) are timed on equal entries through the caller's CSR: three entries per
document, k = 50 and k = 200.  What the call's interface cannot separate is one round from the other seven, so the FIRST ROUND'S SHARE of
the device time comes from a kernel trace of the same two calls, taken apart from the medians (one call each, no median):
  rocprofv3 --kernel-trace -d <dir> -- python tools/top_docs_probe.py --rounds-run
  python tools/top_docs_probe.py --rounds-read <dir> profiles/top_docs_c2.jsonl        (appends one line per k)
One JSON line per measurement; no ratio is expected in advance.
  top_docs_probe.py [out.jsonl] [docs]      (default: profiles/top_docs_c2.jsonl, 1 000 000 documents)"""
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


def median_ms(fn):
    ms, last = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        last = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms, last


def main():
    import topdocs_rule as tr
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "top_docs_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
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
    lines = []

    def emit(**kw):
        kw.update(shape)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def fetch_sums():
        off, tp, va = np.empty(D + 1, np.int64), np.empty(tm["num_sums"], np.uint32), np.empty(tm["num_sums"], np.float32)
        hp._chk(hp._lib.isle_hip_get_doc_topic_sums(hp._h, off.ctypes.data, tp.ctypes.data, va.ctypes.data))
        return off, tp, va

    sources = {"sums": ("post", tm["num_sums"], fetch_sums), "infer": ("infer", inf["nentries"], lambda: hp.infer_entries(D, inf["nentries"]))}
    for source, (fam, nentries, fetch) in sources.items():
        fetch_ms, fetch_all, (off, tp, va) = median_ms(fetch)
        for n in (10, 256):
            hp.topic_top_docs(n, source)  # first-launch costs stay out of the medians
            dev_ms = []

            def call():
                before = hp.timing_get()[fam][0]
                res = hp.topic_top_docs(n, source)
                dev_ms.append(hp.timing_get()[fam][0] - before)
                return res

            a_ms, a_all, got = median_ms(call)
            case = tr.Case(source, k, n, 0, off, tp, va.view(np.uint32), "probe")
            b_ms, b_all, want = median_ms(lambda: tr.rule(case))
            same = all(np.array_equal(got[f].view(np.uint32) if f == "values" else got[f], want[f]) for f in ("docs", "values", "counts", "topic_entries"))
            emit(what="top documents from %s at n = %d" % (source, n), source=source, n=n, entries=int(nentries), a_topic_top_docs_wall_ms=a_ms,
                 a_topic_top_docs_wall_all_ms=a_all, a_device_ms_median=float(np.median(dev_ms)), a_device_ms=dev_ms, a_device_family=fam,
                 b_fetch_entries_ms=fetch_ms, b_fetch_entries_all_ms=fetch_all, b_numpy_rule_ms=b_ms, b_numpy_rule_all_ms=b_all,
                 b_host_path_ms=fetch_ms + b_ms, same_lists_as_the_rule=bool(same))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "topic_sums")
        hp.doc_report_size("topic_sums")
        c_ms, c_all, (nbytes, nlines) = median_ms(lambda: hp.write_doc_report(path, "topic_sums"))
        emit(what="write_doc_report(topic_sums): the sorted report of all sums", c_write_doc_report_wall_ms=c_ms, c_write_doc_report_wall_all_ms=c_all,
             text_bytes=nbytes, text_lines=nlines)
    # the bins' two homes on equal entries: three topics per document, base + {0, 1, 2} kk / 3
    for kk in (50, 200):
        off, tp, va = rounds_csr(kk, D)
        for n in (10, 256):
            hp.topic_top_docs(n, (off, tp, va), num_topics=kk)
            dev_ms = []

            def call():
                before = hp.timing_get()["post"][0]
                hp.topic_top_docs(n, (off, tp, va), num_topics=kk)
                dev_ms.append(hp.timing_get()["post"][0] - before)

            w_ms, w_all, _ = median_ms(call)
            emit(what="bins in %s: the caller's CSR, 3 entries per document" % ("LDS" if kk <= 64 else "global memory"), num_topics=kk, n=n, entries=3 * D,
                 wall_with_upload_ms=w_ms, wall_with_upload_all_ms=w_all, device_ms_median=float(np.median(dev_ms)), device_ms=dev_ms,
                 first_round_share="not in this line: the call books all of its steps under one family; see the kernel trace's lines")
    emit(what="summary", several_ranks="unmeasured", config3="unmeasured: 10 M documents at k = 1000 were not run")
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


def rounds_csr(kk, D=1_000_000):
    """the caller's CSR of the bins' measurement: three topics per document, base + {0, 1, 2} kk / 3"""
    rng = np.random.default_rng(0)
    va = (rng.random(3 * D) * 4 + 1e-3).astype(np.float32)
    off = np.arange(D + 1, dtype=np.int64) * 3
    third = kk // 3
    tp = (rng.integers(0, third, D, dtype=np.uint32)[:, None] + np.arange(3, dtype=np.uint32)[None, :] * np.uint32(third)).reshape(-1)
    return off, tp, va


def rounds_run():
    """what a kernel trace is taken of: per k in (50, 200) a warm-up call and a second one, n = 10"""
    hp = HotPath(0)
    for kk in (50, 200):
        src = rounds_csr(kk)
        for _ in range(2):
            hp.topic_top_docs(10, src, num_topics=kk)
    hp.close()


def rounds_read(trace_dir, out_path):
    """the kernel trace of rounds_run -> one line per k appended to out_path: the kernels of the second call, the first round's share"""
    import csv
    import glob
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(paths[0]))))
    calls = []
    for s, e, name in rows:
        if "td_doc_k" in name:
            calls.append([])
        if calls and "td_" in name:
            short = name[name.index("td_"):].split("(")[0]
            calls[-1].append((short, (e - s) / 1e3))
    assert len(calls) == 4, len(calls)
    with open(out_path, "a") as f:
        for kk, call in ((50, calls[1]), (200, calls[3])):
            hist = [us for name, us in call if name.startswith("td_hist_k")]
            total = sum(us for _, us in call)
            assert len(hist) == 8
            line = dict(what="kernel trace of one call: bins in %s, the caller's CSR, 3 entries per document, n = 10" % ("LDS" if kk <= 64 else "global memory"),
                        num_topics=kk, n=10, entries=3_000_000, kernels_us=[[name, round(us, 2)] for name, us in call], kernels_total_us=round(total, 2),
                        hist_rounds_us=[round(us, 2) for us in hist], first_round_share_of_the_kernels=round(hist[0] / total, 4),
                        note="one call, no median; the memsets and copies between the kernels are not in the total")
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--rounds-run":
        rounds_run()
    elif len(sys.argv) > 1 and sys.argv[1] == "--rounds-read":
        rounds_read(sys.argv[2], sys.argv[3])
    else:
        main()
