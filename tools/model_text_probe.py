"""Timing of the device text path of model files (isle_hip_model_text / isle_hip_edge_topics_text) against the host writers of the
trainer mirror (trainer_detail::write_dense_as_sparse / write_dense through isle_amd/host/model_text_main) on the same model.  A planted
corpus with the planted partition gives a resident catch model and average model of the shape asked for; the number of documents only
shapes their sparsity.  One JSON line per case: device ms (ISLE_T_POST) and launches, wall ms to the last sink call with a sink that
writes to a file on local disk and with a sink that only counts, bytes and entries; for the host side the D2H copy of the dense model
(the host writer cannot start without it) and the writer's wall time, and the ratio host / device.  Medians of `reps` runs.
Usage: python tools/model_text_probe.py [V D k pairs reps]   (default: config 3's V x k = 100000 x 1000 with 2.5 M documents, 5000 pairs)."""
import ctypes as C
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
from tools.synth import Corpus
import isle_amd
from isle_amd.hot_path import catchword_rank, model_rank_threshold

V, D, k, npairs, reps = (int(x) for x in sys.argv[1:6]) if len(sys.argv) >= 6 else (100000, 2500000, 1000, 5000, 5)
HOST_EDGE_MAX = 300_000_000   # entries up to which the edge model is also fetched and written by the host writer (once)
MAIN = os.path.join(ROOT, "isle_amd", "host", "model_text_main")
tmp = tempfile.mkdtemp(prefix="model_text_probe_")


def med(xs):
    return round(float(np.median(xs)), 3)


def device_case(hp, case, call, **extra):
    """call(consume) -> (nbytes, nentries); consume None = the size query"""
    out = {"case": case, "shape": [V, k], "docs": D}
    path = os.path.join(tmp, "dev.txt")
    for name in ("size_query", "count_sink", "file_sink"):
        walls, devs = [], []
        for rep in range(reps + 1):  # the first run warms up (buffers, file)
            hp.timing_enable(1)
            hp.timing_reset()
            if name == "file_sink":
                f = open(path, "wb")
            seen = [0]
            t = time.perf_counter()
            nb, ne = call(None if name == "size_query" else f.write if name == "file_sink" else (lambda mv: seen.__setitem__(0, seen[0] + len(mv))))
            wall = (time.perf_counter() - t) * 1e3
            if name == "file_sink":
                f.close()
            tg = hp.timing_get()["post"]
            if rep:
                walls.append(wall)
                devs.append(tg[0])
        out.update({"wall_ms_" + name: med(walls), "device_ms_" + name: med(devs), "device_ms_all_" + name: [round(d, 3) for d in devs], "launches_" + name: tg[1]})
    out.update(bytes=nb, entries=ne, **extra)
    hp.timing_enable(0)
    return out


def host_writer(model, cols, reps_host):
    """the C++ host writers on `model` (V x cols, F-order) -> {"host.sparse": ms, "host.dense": ms, "dev.sparse": ms, "dev.dense": ms}"""
    src = os.path.join(tmp, "model.f32")
    model.reshape(-1, order="F").tofile(src)
    r = subprocess.run([MAIN, src, str(V), str(cols), os.path.join(tmp, "m"), str(reps_host)], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    res = {ln.split()[0]: float(ln.split()[1]) for ln in r.stdout.splitlines() if len(ln.split()) == 2}
    for fmt in ("sparse", "dense"):
        assert open(os.path.join(tmp, "m.dev." + fmt), "rb").read() == open(os.path.join(tmp, "m.host." + fmt), "rb").read()
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    return res


t0 = time.perf_counter()
c = Corpus(V, D, k, 31337)
cnt, rows, offs = c.A_views()
hp = isle_amd.HotPath()
hp.upload_counts(V, cnt, rows, offs)
hp.threshold(k)
oc = np.empty(hp.D, np.uint64)
hp._chk(hp._lib.isle_hip_get_B(hp._h, None, None, None, oc.ctypes.data_as(C.c_void_p), None))
assign = c.planted()[oc.astype(np.int64)].astype(np.uint32)
hp.find_catchwords(k, catchword_rank(D, k), assign=assign, fetch_thresholds=False)
lib, h = hp._lib, hp._h
hp._chk(lib.isle_hip_topic_model(h, k, model_rank_threshold(D, k), None, None, None, None, None))
print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "shape": [V, k], "docs": D}), flush=True)

# the D2H copy of a dense V x k model: the fetching call minus the non-fetching call of the average model
M = np.empty((V, k), np.float32, order="F")
d2h = []
for _ in range(reps + 1):
    t = time.perf_counter()
    hp._chk(lib.isle_hip_avg_topic_model(h, k, M.ctypes.data_as(C.c_void_p)))
    a = time.perf_counter() - t
    t = time.perf_counter()
    hp._chk(lib.isle_hip_avg_topic_model(h, k, None))
    d2h.append((a - (time.perf_counter() - t)) * 1e3)
d2h_ms = med(d2h[1:])
avg = M.copy(order="F")
hp._chk(lib.isle_hip_edge_topics(h, np.repeat(np.arange(k, dtype=np.int64), 2).ctypes.data_as(C.c_void_p), k, C.c_float(1.0), M.ctypes.data_as(C.c_void_p)))
catch = M  # 1 * m + 0 * m: the resident catch model's bits

for name, which, fmt, model in (("sparse text of the catch model (M_hat_catch_sparse)", "catch", "sparse", catch),
                                ("dense text of the average model (M_hat_avg)", "avg", "dense", avg)):
    line = device_case(hp, name, lambda consume: hp._model_text_call(which, fmt, consume))
    hw = host_writer(model, k, reps)
    line.update(host_d2h_ms=d2h_ms, host_writer_ms=hw["host." + fmt], cpp_device_path_from_host_model_ms=hw["dev." + fmt])
    line["host_writer_over_device_file_sink"] = round(line["host_writer_ms"] / line["wall_ms_file_sink"], 2)
    line["host_writer_plus_d2h_over_device_file_sink"] = round((line["host_writer_ms"] + d2h_ms) / line["wall_ms_file_sink"], 2)
    print(json.dumps(line), flush=True)

rng = np.random.default_rng(3)
pairs = rng.integers(0, k, size=(npairs, 2)).astype(np.int64)
pp = pairs.ctypes.data_as(C.c_void_p)
line = device_case(hp, "edge text for %d pairs (EdgeModel_sparse)" % npairs,
                   lambda consume: hp._text_call(lambda sink, nb, ne: lib.isle_hip_edge_topics_text(h, pp, npairs, C.c_float(0.7), 0, sink, None, nb, ne), consume),
                   edge_shape=[V, npairs])
if V * npairs <= HOST_EDGE_MAX:
    t = time.perf_counter()
    E = hp.edge_topics(pairs, 0.7)
    line["host_edge_topics_with_d2h_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    hw = host_writer(E, npairs, 1)
    del E
    line["host_writer_ms"] = hw["host.sparse"]
    line["host_writer_runs"] = 1
    line["host_path_over_device_file_sink"] = round((line["host_writer_ms"] + line["host_edge_topics_with_d2h_ms"]) / line["wall_ms_file_sink"], 2)
else:
    line["host_writer_ms"] = "unmeasured (the V x n floats are %.1f GB)" % (V * npairs * 4 / 1e9)
print(json.dumps(line), flush=True)
hp.close()
shutil.rmtree(tmp, ignore_errors=True)
