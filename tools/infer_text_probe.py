#!/usr/bin/env python3
"""Timing probe for isle_hip_infer_text at the configuration-2 shape of tools/infer_resident_probe.py (50 k x 200 model, 1 M resident
documents of ~100 distinct words), medians of 5 in one process, for both kinds of text ("entries": DocTopicWeights.tsv, "top": ISLEInfer's
top_topics_* files):
  (a) HotPath.infer_resident with the entries left on the device, plus HotPath.write_infer_text into a local file;
  (b) the path before the device formatter, in the same visit: infer_resident with the entries fetched, plus the host loops
      (trainer_detail::write_doc_topic_lines, run by isle_amd/host/infer_text_main on the same arrays into a local file);
  (c) the formatter's device time: the growth of ISLE_T_INFER over the write_infer_text call.
The Python infer_resident always fetches top_topic / top_weight (40 MB at 1 M documents), in (a) as in (b).  One JSON line per
measurement; no ratio is expected in advance.
  infer_text_probe.py <out.jsonl> [docs]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isle_amd import HotPath  # noqa: E402
from tools.infer_resident_probe import REPS, corpus, limit  # noqa: E402

EXE = os.path.join(ROOT, "isle_amd", "host", "infer_text_main")


def median_ms(fn, what, seconds):
    ms, last = [], None
    for _ in range(REPS):
        with limit(seconds, what):
            t0 = time.perf_counter()
            last = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms, last


def main():
    out_path = sys.argv[1]
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    rng = np.random.default_rng(0)
    with limit(300, "corpus"):
        M = rng.random((V, k), dtype=np.float32) ** 8
        M /= M.sum(0, keepdims=True)
        Mf = np.asfortranarray(M)
        offs, rows, counts = corpus(V, D, rng)
    hp = HotPath(0)
    hp.timing_enable(True)
    with limit(120, "upload"):
        hp.upload_counts(V, counts, rows, offs)
    shape = dict(V=V, k=k, docs=D, nnz=int(rows.shape[0]), reps=REPS)
    lines = []

    def emit(**kw):
        kw.update(shape)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    hp.infer_resident(Mf, docs=(0, 1000))   # first-launch costs stay out of the medians
    hp.infer_text("entries")
    hp.infer_text("top")
    infer_left, infer_left_all, _ = median_ms(lambda: hp.infer_resident(Mf, fetch_entries=False), "infer_resident", 120)
    infer_fetch, infer_fetch_all, got = median_ms(lambda: hp.infer_resident(Mf), "infer_resident + entries", 120)
    emit(what="infer_resident, entries left on the device", wall_ms_median=infer_left, wall_ms=infer_left_all, nentries=got["nentries"])
    emit(what="infer_resident, entries fetched", wall_ms_median=infer_fetch, wall_ms=infer_fetch_all,
         entry_bytes=int(got["nentries"] * 8 + (D + 1) * 8))
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("entries", "top"):
            path = os.path.join(tmp, kind + ".dev")
            dev_ms = []

            def write():
                before = hp.timing_get()["infer"][0]
                r = hp.write_infer_text(path, kind)
                dev_ms.append(hp.timing_get()["infer"][0] - before)
                return r

            text_ms, text_all, (nbytes, nlines) = median_ms(write, "write_infer_text " + kind, 300)
            src, host_out = os.path.join(tmp, kind + ".bin"), os.path.join(tmp, kind + ".host")
            arrays = ([got["offs"].astype(np.int64), got["topic"].astype(np.uint32), got["weight"].astype(np.float32)] if kind == "entries"
                      else [got["top_topic"].astype(np.int32), got["top_weight"].astype(np.float32)])
            with open(src, "wb") as f:
                for a in arrays:
                    f.write(np.ascontiguousarray(a).tobytes())
            with limit(900, "infer_text_main " + kind):
                r = subprocess.run([EXE, kind, src, str(D), "1", host_out, str(REPS)], capture_output=True, text=True, timeout=880)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-1000:])
            host_ms = float(r.stdout.split()[-1])
            same = os.path.getsize(host_out) == nbytes
            if same and nbytes <= 1 << 31:
                same = open(host_out, "rb").read() == open(path, "rb").read()
            a_ms, b_ms = infer_left + text_ms, infer_fetch + host_ms
            emit(what="text of the %s" % kind, kind=kind, text_bytes=nbytes, text_lines=nlines,
                 a_device_path_wall_ms=a_ms, a_infer_ms=infer_left, a_write_infer_text_ms=text_ms, a_write_infer_text_all_ms=text_all,
                 b_host_path_wall_ms=b_ms, b_infer_and_fetch_ms=infer_fetch, b_host_loop_ms=host_ms, ratio_b_over_a=b_ms / a_ms,
                 text_alone_ratio_host_over_device=host_ms / text_ms, c_formatter_device_ms_median=float(np.median(dev_ms)), c_formatter_device_ms=dev_ms,
                 same_bytes_as_host_loop=bool(same))
            for p in (path, src, host_out):
                os.remove(p)
    emit(what="summary", config3="unmeasured: 10 M documents at k = 1000 were not run")
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
