"""Timing of the device loader of model files (isle_hip_load_model_text) against the serial host parser of isle_amd/host/model_read.h
(through isle_amd/host/model_read_main) on the same text, in the same visit.  A random model on the simplex with half its entries zero
is written by the device writer into a file of each format; the device side is HotPath.load_model_text on the bytes in memory with the
context already created: wall time of the call, upload included, and the device time booked under ISLE_T_INGEST; the host side is the
parse of the bytes in memory.  Medians of `reps` runs; the two models are compared bit for bit.  One JSON line per shape and format.
Usage: python tools/model_load_probe.py [reps [V k ...]]   (default: 5 runs of 50000 x 200 and 100000 x 1000)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import isle_amd

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dims = [int(x) for x in sys.argv[2:]] or [50000, 200, 100000, 1000]
MAIN = os.path.join(ROOT, "isle_amd", "host", "model_read_main")
tmp = tempfile.mkdtemp(prefix="model_load_probe_")
hp = isle_amd.HotPath()
for V, k in zip(dims[::2], dims[1::2]):
    rng = np.random.default_rng(V + k)
    M = rng.random((V, k), np.float32) ** 4
    M[rng.random((V, k), np.float32) < 0.5] = 0
    M /= M.sum(axis=0, keepdims=True)
    M = np.asfortranarray(M)
    for fmt in ("sparse", "dense"):
        path, out = os.path.join(tmp, "model." + fmt), os.path.join(tmp, "host.f32")
        nbytes, _ = hp.write_model(path, M, fmt)
        text = np.fromfile(path, np.uint8)
        walls, devs = [], []
        for rep in range(reps + 1):   # the first run warms up
            hp.timing_enable(1)
            hp.timing_reset()
            t = time.perf_counter()
            n = hp.load_model_text(text, V, k, fmt)
            wall = (time.perf_counter() - t) * 1e3
            if rep:
                walls.append(wall)
                devs.append(hp.timing_get()["ingest"][0])
        hp.timing_enable(0)
        r = subprocess.run([MAIN, path, str(V), str(k), fmt, "1", out, str(reps)], capture_output=True, text=True, timeout=3000)
        assert r.returncode == 0, r.stderr[-2000:]
        host_ms = float(r.stdout.split()[1])
        equal = bool(np.array_equal(np.fromfile(out, np.uint32), hp.loaded_model().ravel(order="F").view(np.uint32)))
        wall_ms = float(np.median(walls))
        print(json.dumps({"case": "load " + fmt, "shape": [V, k], "bytes": nbytes, "entries": n, "reps": reps, "device_wall_ms": round(wall_ms, 3),
                          "device_ms_ingest": round(float(np.median(devs)), 3), "device_GB_per_s": round(nbytes / wall_ms / 1e6, 2),
                          "host_parser_ms": round(host_ms, 3), "host_GB_per_s": round(nbytes / host_ms / 1e6, 3),
                          "host_over_device": round(host_ms / wall_ms, 1), "bit_equal": equal}), flush=True)
        del text
        os.remove(path)
        os.remove(out)
hp.close()
shutil.rmtree(tmp, ignore_errors=True)
