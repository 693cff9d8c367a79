#!/usr/bin/env python3
"""Timing probe for isle_hip_word_doc_freq / isle_hip_prune_vocab on the configuration-2 corpus (50 k words, 1 M documents, ~108 M entries),
medians of 5 in one process after a warm-up:
  (a) word_doc_freq in both forms of the document-frequency kernel (counters in LDS over vocabulary parts / one global atomic per entry),
      the two alternating round by round: wall time and device time (the growth of ISLE_T_INGEST);
  (b) prune_vocab(min_df=5, max_df=0.5, keep_n=20000), each repetition on a fresh upload (the upload is not timed): wall and device time;
  (c) the only way there was before: A fetched (get_A), then the numpy rule of tests/vocab_rule.py on the host; the two parts timed apart.
Each kernel's achieved share of 8 TB/s is computed on its algorithmic bytes: the histogram reads 4 nnz; the compaction reads 8 nnz, makes
4 nnz of flags and 8 (nnz + 1) of positions and writes 8 nnz_new (its device time: the prune's less the histogram's in the default form).
One JSON line per measurement; no time is expected in advance.
  vocab_prune_probe.py [out.jsonl] [docs]      (default: profiles/vocab_prune_c2.jsonl, 1 000 000 documents)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from isle_amd import HotPath  # noqa: E402
from tools.synth import Corpus  # noqa: E402

REPS = 5
HBM = 8e12  # bytes per second


def main():
    import vocab_rule as vr
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocab_prune_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    cnt, rows, offs = Corpus(V, D, k, 1).A()
    cnt, rows, offs = np.asarray(cnt, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    nnz = int(rows.size)
    hp = HotPath(0)
    hp.timing_enable(True)
    hp.upload_counts(V, cnt, rows, offs)
    shape = dict(V=V, docs=D, entries=nnz, reps=REPS)
    lines = []

    def emit(**kw):
        kw.update(shape)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn):
        hp.synchronize()
        before = hp.timing_get()["ingest"][0]
        t0 = time.perf_counter()
        res = fn()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, hp.timing_get()["ingest"][0] - before, res

    # (a) the two forms of the histogram, alternating
    want_df = vr.df_of(V, rows)
    wall, dev = {"lds": [], "global": []}, {"lds": [], "global": []}
    for rep in range(REPS + 1):  # the first round is the warm-up
        for form in ("lds", "global"):
            hp.vocab_hist_form(form)
            w, d, df = timed(hp.word_doc_freq)
            assert np.array_equal(df, want_df), form
            if rep:
                wall[form].append(w)
                dev[form].append(d)
    hp.vocab_hist_form("auto")
    for form in ("lds", "global"):
        d = float(np.median(dev[form]))
        emit(what="word_doc_freq, counters in %s" % ("LDS over vocabulary parts" if form == "lds" else "global memory, one atomic per entry"), form=form,
             wall_ms_median=float(np.median(wall[form])), wall_ms=wall[form], device_ms_median=d, device_ms=dev[form], algorithmic_bytes=4 * nnz,
             share_of_8TBs=4 * nnz / (d * 1e-3) / HBM, max_df=int(want_df.max()))
    hist_ms = float(np.median(dev["lds"]))
    faster = "lds" if np.median(dev["lds"]) <= np.median(dev["global"]) else "global"

    # (b) the prune, each on a fresh upload
    case = vr.Case("c2", V, offs, rows, cnt, 5, int(np.floor(0.5 * D)), 20000, "probe", True)
    want = vr.rule(case)
    wall, dev, got = [], [], None
    for rep in range(REPS + 1):
        if rep:
            hp.upload_counts(V, cnt, rows, offs)
        w, d, got = timed(lambda: hp.prune_vocab(min_df=5, max_df=0.5, keep_n=20000))
        if rep:
            wall.append(w)
            dev.append(d)
    c2, r2, o2 = hp.get_A()
    same = bool(np.array_equal(got["kept_words"], want["kept_words"]) and np.array_equal(o2, want["offs"]) and np.array_equal(r2, want["rows"]) and
                np.array_equal(c2.view(np.uint32), want["counts"]) and got["docs_emptied"] == want["docs_emptied"])
    d = float(np.median(dev))
    nnz_new = int(got["nnz"])
    compact_bytes = 8 * nnz + 4 * nnz + 8 * (nnz + 1) + 8 * nnz_new
    emit(what="prune_vocab(min_df=5, max_df=0.5, keep_n=20000)", wall_ms_median=float(np.median(wall)), wall_ms=wall, device_ms_median=d, device_ms=dev,
         vocab_kept=int(got["vocab"]), entries_kept=nnz_new, docs_emptied=int(got["docs_emptied"]), same_as_the_numpy_rule=same,
         compaction_device_ms=d - hist_ms, compaction_algorithmic_bytes=compact_bytes, compaction_share_of_8TBs=compact_bytes / ((d - hist_ms) * 1e-3) / HBM,
         note="compaction device time = the prune's less the histogram's median (LDS form); flags, scan, pack and offsets together")

    # (c) the host way: fetch A, then the numpy rule
    hp.upload_counts(V, cnt, rows, offs)
    fetch, rule = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        fc, fr, fo = hp.get_A()
        t1 = time.perf_counter()
        vr.rule(vr.Case("c2", V, fo, fr, fc, 5, int(np.floor(0.5 * D)), 20000, "probe", True))
        t2 = time.perf_counter()
        if rep:
            fetch.append((t1 - t0) * 1e3)
            rule.append((t2 - t1) * 1e3)
    emit(what="the host way: get_A, then the numpy rule", fetch_A_ms_median=float(np.median(fetch)), fetch_A_ms=fetch, numpy_rule_ms_median=float(np.median(rule)),
         numpy_rule_ms=rule, host_path_ms=float(np.median(fetch) + np.median(rule)), note="the pruned matrix is not uploaded again in this figure")
    emit(what="summary", faster_histogram_form=faster, several_ranks="unmeasured",
         config3="unmeasured: out of the probe's scope")
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
