"""Full-size timing of the triple feed (isle_hip_feed_*) against the paths beside it.  Medians of --reps runs each:

  (a) HotPath.upload_coo of the corpus' triples in shuffled document order, in one call and in 4 Mi-entry batches: wall, and the device
      time of the ISLE_T_INGEST family inside it; for the batched form also the feed() calls alone (wall and device time before
      feed_finalize): the kernels' share of a feed_entries call
  (b) isle_amd/host/feed_main --time on the same corpus as a tdf file: the device feed against csc_from_fed + upload of the finished
      CSC, which is what ISLETrainer::finalize_data did before the device feed (--host-reps runs: the host sort takes most of a minute)
  (c) ingest_tdf of the same corpus as text, for scale

Usage: python tools/feed_probe.py [V D k] [--reps N] [--host-reps N] [--out FILE]      (default 50000 1000000 200: config 2)
One JSON line per measurement, appended to FILE (default profiles/feed_c2.jsonl)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.synth import Corpus  # noqa: E402
import isle_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[50000, 1000000, 200])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_c2.jsonl"))
args = ap.parse_args()
V, D, k = args.shape
BATCH = 4 << 20


def emit(rec):
    rec = dict(shape=[V, D, k], **rec)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def med(xs):
    return round(float(np.median(xs)), 2)


c = Corpus(V, D, k, 1)
cnt, rows, offs = c.A()
n = len(cnt)
# triples in shuffled document order (the words of a document stay ascending: the order within a document decides nothing here)
order = np.random.default_rng(0).permutation(D)
lens = np.diff(offs)[order]
start = np.repeat(offs[:-1][order] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
src = start + np.arange(n)
docs = np.repeat(order, lens).astype(np.uint32)
words = rows[src]
counts = cnt[src].astype(np.uint32)
del start, src

hp = isle_amd.HotPath()
hp.upload_coo(V, D, docs[:100000], words[:100000], counts[:100000])  # warm-up: code object, first allocations
hp.timing_enable(True)

# ---- (a)
for batch in (None, BATCH):
    wall, dev = [], []
    for _ in range(args.reps):
        hp.timing_reset()
        t = time.perf_counter()
        fed, nnz = hp.upload_coo(V, D, docs, words, counts, batch=batch)
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(hp.timing_get()["ingest"][0])
    gc, gr, go = hp.get_A()
    same = bool(np.array_equal(go, offs) and np.array_equal(gr, rows) and np.array_equal(gc, cnt))
    emit(dict(what="upload_coo", batch=batch, entries=n, nnz=nnz, reps=args.reps, wall_ms=med(wall), ingest_device_ms=med(dev),
              copy_and_host_ms=med(np.array(wall) - np.array(dev)), identical_to_generator_csc=same))
wall, dev, fin = [], [], []
for _ in range(args.reps):
    hp.timing_reset()
    hp.feed_begin(V, D, n)
    t = time.perf_counter()
    for at in range(0, n, BATCH):
        hp.feed(docs[at:at + BATCH], words[at:at + BATCH], counts[at:at + BATCH])
    wall.append((time.perf_counter() - t) * 1e3)
    dev.append(hp.timing_get()["ingest"][0])
    t = time.perf_counter()
    hp.feed_finalize()
    fin.append((time.perf_counter() - t) * 1e3)
emit(dict(what="feed_calls_alone", batch=BATCH, calls=-(-n // BATCH), reps=args.reps, feed_calls_wall_ms=med(wall), feed_calls_kernels_ms=med(dev),
          kernels_share_of_a_feed_call=round(float(np.median(np.array(dev) / np.array(wall))), 4), feed_finalize_wall_ms=med(fin)))

# ---- (c)
text = c.tdf_bytes()
wall, dev = [], []
for _ in range(args.reps):
    hp.timing_reset()
    t = time.perf_counter()
    hp.ingest_tdf(text, V, D, max_entries=n)
    wall.append((time.perf_counter() - t) * 1e3)
    dev.append(hp.timing_get()["ingest"][0])
emit(dict(what="ingest_tdf", text_bytes=int(text.size), lines=n, reps=args.reps, wall_ms=med(wall), ingest_device_ms=med(dev)))
hp.close()

# ---- (b)
if args.host_reps > 0:
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "corpus.tdf")
        text.tofile(path)
        del text
        runs = []
        for _ in range(args.host_reps):
            r = subprocess.run([os.path.join(ROOT, "isle_amd", "host", "feed_main"), path, str(V), str(D), str(BATCH), "--time"],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("feed_main failed: " + r.stderr[-2000:])
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        emit(dict(what="feed_main", flush_entries=BATCH, reps=args.host_reps, entries=runs[0]["entries"], nnz=runs[0]["nnz"],
                  host_csc_from_fed_plus_upload_ms=med([x["host_csc_from_fed_plus_upload_s"] * 1e3 for x in runs]),
                  device_feed_ms=med([x["device_feed_s"] * 1e3 for x in runs]), device_equals_host_bit_for_bit=True))
