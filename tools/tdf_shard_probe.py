"""Full-size timing of the sharded tdf ingest in one process (isle_hip_tdf_begin_counts / _finalize_counts / _begin_window), parts = 8.
Medians of --reps runs each after a warm-up, the file in the page cache:

  (a) pass 1, the counting stream and its plan, over one eighth of the bytes (the range of rank 3 of 8) and over the whole file
  (b) pass 2, the windowed stream over the whole file, for part 0 and part 7: wall, and the device time of ISLE_T_INGEST
  (c) ingest_tdf_file of the same file in the same visit, for comparison

What it cannot show: the cost at N > 1 of all ranks reading the whole file in pass 2 (one GPU, one process).

Usage: python tools/tdf_shard_probe.py [V D k] [--reps N] [--out FILE]     (default 50000 1000000 200: config 2)
One JSON line per measurement, appended to FILE (default profiles/tdf_shard_c2.jsonl)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import isle_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[50000, 1000000, 200])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdf_shard_c2.jsonl"))
args = ap.parse_args()
V, D, k = args.shape
PARTS = 8


def emit(rec):
    line = json.dumps(dict(shape=[V, D, k], parts=PARTS, **rec))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2))


def timed(hp, fn):
    hp.timing_reset()
    t = time.perf_counter()
    info = fn()
    wall = (time.perf_counter() - t) * 1e3
    return wall, hp.timing_get()["ingest"][0], info


from tools.synth import Corpus  # noqa: E402

c = Corpus(V, D, k, 1)
text = c.tdf_bytes()
hp = isle_amd.HotPath()
hp.timing_enable(True)

with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "corpus.tdf")
    text.tofile(path)
    size = int(text.size)
    del text

    def pass1(b=None, e=None):
        with open(path, "rb", buffering=0) as f:
            hp.tdf_begin_counts(V, D)
            hp._pump(f) if b is None else hp._pump(f, b, e)
            return hp.tdf_finalize_counts(PARTS, agree_tag=size)

    def pass2(bounds, part):
        with open(path, "rb", buffering=0) as f:
            hp.tdf_begin_window(V, D, bounds[part], bounds[part + 1])
            hp._pump(f)
            return hp.tdf_finalize()

    # warm-up: first allocations, the page-locked buffers, the file in the page cache
    plan = pass1()
    bounds = plan["bounds"]
    whole = hp.ingest_tdf_file(path, V, D)
    offs = hp.get_A()[2]
    first = pass2(bounds, 0)
    emit(dict(what="identity", text_bytes=size, lines=plan["lines_global"], bounds=[int(x) for x in bounds],
              nnz_of_parts_by_whole_ingest=[int(offs[bounds[p + 1]] - offs[bounds[p]]) for p in range(PARTS)], part0_nnz=first["nnz"],
              entries_read_equal=bool(first["entries_read"] == whole["entries_read"])))
    del offs

    eighth = [timed(hp, lambda: pass1(size * 3 // PARTS, size * 4 // PARTS)) for _ in range(args.reps)]
    full = [timed(hp, pass1) for _ in range(args.reps)]
    emit(dict(what="pass1_counts_and_plan", reps=args.reps, one_eighth_wall_ms=stats([r[0] for r in eighth]), one_eighth_device_ms=stats([r[1] for r in eighth]),
              one_eighth_lines=eighth[0][2]["lines_local"], whole_file_wall_ms=stats([r[0] for r in full]), whole_file_device_ms=stats([r[1] for r in full])))
    for part in (0, PARTS - 1):
        runs = [timed(hp, lambda: pass2(bounds, part)) for _ in range(args.reps)]
        emit(dict(what="pass2_window", part=part, reps=args.reps, wall_ms=stats([r[0] for r in runs]), ingest_device_ms=stats([r[1] for r in runs]),
                  nnz=runs[0][2]["nnz"], entries_read=runs[0][2]["entries_read"]))
    runs = [timed(hp, lambda: hp.ingest_tdf_file(path, V, D)) for _ in range(args.reps)]
    emit(dict(what="ingest_tdf_file", reps=args.reps, wall_ms=stats([r[0] for r in runs]), ingest_device_ms=stats([r[1] for r in runs]), nnz=runs[0][2]["nnz"]))
    hp.close()
