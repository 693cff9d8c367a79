"""Full-size timing of the tdf text stream (isle_hip_tdf_*) against the whole-text ingest.  Medians of --reps runs each, in one process
after a warm-up, the two sides of a comparison taken in turn:

  (a) in memory: ingest_tdf(bytes) against tdf_begin / tdf_write(bytes) / tdf_finalize: wall, and the device time of ISLE_T_INGEST
  (b) from a file in the page cache: the file read whole (np.fromfile) and then ingest_tdf, which is what ISLETrainer::load_data_from_file
      did before it streamed, against ingest_tdf_file
  (c) ingest_tdf_file at piece sizes of 1, 4 and 16 MiB (a size above the library's own 16 MiB cannot be asked for)
  (d) isle_amd/host/tdf_stream_main --time and --time-stream-first in turn: both walls from the C++ side, either leg first, each run
      also comparing the two matrices bit for bit; every run under a time limit of its own

Usage: python tools/tdf_stream_probe.py [V D k] [--reps N] [--keep-file PATH] [--out FILE]     (default 50000 1000000 200: config 2)
One JSON line per measurement, appended to FILE (default profiles/tdf_stream_c2.jsonl)."""
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
import isle_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[50000, 1000000, 200])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--keep-file", default=None, help="write the corpus text here and leave it (default: a temporary file)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdf_stream_c2.jsonl"))
args = ap.parse_args()
V, D, k = args.shape
MIB = 1 << 20


def emit(rec):
    rec = dict(shape=[V, D, k], **rec)
    line = json.dumps(rec)
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


def warm(hp):
    hp.ingest_tdf(b"1 1 1\n2 2 2\n", 5, 5)
    hp.tdf_begin(5, 5)
    hp.tdf_write(b"1 1 1\n2 2 2\n")
    hp.tdf_finalize()
    hp.timing_enable(True)


def file_pieces(hp, path, pieces):
    for piece in pieces:
        runs = [timed(hp, lambda: hp.ingest_tdf_file(path, V, D, _piece_bytes=piece)) for _ in range(args.reps)]
        emit(dict(what="ingest_tdf_file_by_piece", piece_mib=piece // MIB, reps=args.reps, wall_ms=stats([r[0] for r in runs]),
                  ingest_device_ms=stats([r[1] for r in runs]), nnz=runs[0][2]["nnz"]))


from tools.synth import Corpus  # noqa: E402

c = Corpus(V, D, k, 1)
cnt, rows, offs = c.A()
n = len(cnt)
text = c.tdf_bytes()
hp = isle_amd.HotPath()
warm(hp)

with tempfile.TemporaryDirectory() as tmp:
    path = args.keep_file or os.path.join(tmp, "corpus.tdf")
    text.tofile(path)

    def stream_bytes():
        hp.tdf_begin(V, D)
        hp.tdf_write(text)
        return hp.tdf_finalize(n)

    # one untimed run of each: first allocations, the page-locked buffers, the file in the page cache
    want = hp.ingest_tdf(text, V, D, max_entries=n)
    ref = hp.get_A()
    same = []
    for fn in (stream_bytes, lambda: hp.ingest_tdf_file(path, V, D, n)):
        info = fn()
        same.append(bool(info == want and all(np.array_equal(g, r) for g, r in zip(hp.get_A(), ref))))
    del ref
    emit(dict(what="identity", text_bytes=int(text.size), lines=n, nnz=want["nnz"], tdf_write_equals_ingest_tdf=same[0], ingest_tdf_file_equals_ingest_tdf=same[1]))

    # ---- (a)
    whole, stream = [], []
    for _ in range(args.reps):
        whole.append(timed(hp, lambda: hp.ingest_tdf(text, V, D, max_entries=n)))
        stream.append(timed(hp, stream_bytes))
    emit(dict(what="in_memory", reps=args.reps, ingest_tdf_wall_ms=stats([r[0] for r in whole]), ingest_tdf_device_ms=stats([r[1] for r in whole]),
              tdf_write_wall_ms=stats([r[0] for r in stream]), tdf_write_device_ms=stats([r[1] for r in stream])))
    del text

    # ---- (b)
    whole, stream = [], []
    for _ in range(args.reps):
        whole.append(timed(hp, lambda: hp.ingest_tdf(np.fromfile(path, np.uint8), V, D, max_entries=n)))
        stream.append(timed(hp, lambda: hp.ingest_tdf_file(path, V, D, n)))
    emit(dict(what="from_cached_file", reps=args.reps, read_whole_then_ingest_tdf_wall_ms=stats([r[0] for r in whole]),
              ingest_tdf_file_wall_ms=stats([r[0] for r in stream]), ingest_tdf_file_device_ms=stats([r[1] for r in stream])))

    # ---- (c)
    file_pieces(hp, path, [1 * MIB, 4 * MIB, 16 * MIB])
    hp.close()

    # ---- (d)
    runs = []
    for i in range(2 * args.reps):                      # either leg first in turn
        r = subprocess.run([os.path.join(ROOT, "isle_amd", "host", "tdf_stream_main"), path, str(V), str(D), "0", "--time-stream-first" if i % 2 else "--time"],
                           capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            raise SystemExit("tdf_stream_main failed: " + r.stderr[-2000:])
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    emit(dict(what="tdf_stream_main", reps=2 * args.reps, entries_read=runs[0]["entries_read"], nnz=runs[0]["nnz"],
              whole_read_plus_ingest_ms=stats([x["whole_read_plus_ingest_s"] * 1e3 for x in runs]), stream_ms=stats([x["stream_s"] * 1e3 for x in runs]),
              stream_equals_whole_bit_for_bit=True))
