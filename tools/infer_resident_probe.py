#!/usr/bin/env python3
"""Timing probe for isle_hip_infer_resident at the configuration-2 shape (50 k x 200 model, 1 M documents of ~100 distinct words, the
shape of tools/infer_probe.py): wall and ISLE_T_INFER device time of HotPath.infer_resident with and without fetching the entries,
against HotPath.infer with the dense weights fetched to the host (the only way to the full weights before), medians of 5 in one
process; the pack kernel alone (an empty document range: transpose + row flags) and the compaction by difference, each against the HBM
copy bound of its bytes.  One JSON line per measurement.
  infer_resident_probe.py <out.jsonl> [docs]"""
import contextlib
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isle_amd import HotPath  # noqa: E402

HBM_PEAK_GBS = 8000.0      # bench.py: the HBM3E figure the roofline fractions of this project are quoted against
HBM_ACHIEVABLE_GBS = 6300.0
REPS = 5


@contextlib.contextmanager
def limit(seconds, what):
    def on_alarm(signum, frame):
        raise TimeoutError("%s ran into its limit of %d s" % (what, seconds))
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def corpus(V, D, rng):
    """~100 distinct words per document, ascending: draws with replacement, sorted by (document, word), duplicates dropped."""
    lens = np.clip(rng.lognormal(np.log(100), 0.4, size=D).astype(np.int64), 20, 400)
    doc = np.repeat(np.arange(D, dtype=np.int64), lens)
    key = np.sort(doc * V + rng.integers(0, V, size=doc.shape[0]))
    key = key[np.concatenate(([True], key[1:] != key[:-1]))]
    offs = np.zeros(D + 1, np.int64)
    offs[1:] = np.cumsum(np.bincount(key // V, minlength=D))
    rows = (key % V).astype(np.uint32)
    return offs, rows, rng.integers(1, 4, size=rows.shape[0]).astype(np.float32)


def measure(hp, fn, what, seconds):
    wall, dev, last = [], [], None
    for _ in range(REPS):
        with limit(seconds, what):
            hp.timing_reset()
            t0 = time.perf_counter()
            last = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(hp.timing_get()["infer"][0])
    return dict(wall_ms_median=float(np.median(wall)), wall_ms=wall, device_ms_median=float(np.median(dev)), device_ms=dev,
                device_ms_spread=float(max(dev) - min(dev))), last


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
    shape = dict(V=V, k=k, docs=D, nnz=int(rows.shape[0]), reps=REPS, model="host array, column-major, uploaded by every call (%d MB)" % (V * k * 4 >> 20))
    lines = []

    def emit(**kw):
        kw.update(shape)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    hp.infer_resident(Mf, docs=(0, 1000))   # first-launch costs stay out of the medians
    hp.infer(M, offs[:1001], rows[:offs[1000]], counts[:offs[1000]])
    r_no, a = measure(hp, lambda: hp.infer_resident(Mf, fetch_entries=False), "infer_resident", 120)
    emit(what="infer_resident, entries left on the device", nentries=a["nentries"], nconverged=a["nconverged"], **r_no)
    r_fetch, b = measure(hp, lambda: hp.infer_resident(Mf), "infer_resident + entries", 120)
    emit(what="infer_resident, entries fetched", nentries=b["nentries"], entry_bytes=int(b["nentries"] * 8 + (D + 1) * 8), **r_fetch)
    r_host, c = measure(hp, lambda: hp.infer(M, offs, rows, counts), "infer (host pointers)", 240)
    emit(what="infer: model and documents uploaded, dense weights fetched", dense_weight_bytes=int(D * k * 4), nconverged=c["nconverged"], **r_host)
    same = all(np.array_equal(b[n], c[n]) for n in ("top_topic", "top_weight", "llh")) and b["nconverged"] == c["nconverged"]
    r_pack, _ = measure(hp, lambda: hp.infer_resident(Mf, docs=(0, 0), fetch_entries=False), "pack", 60)
    ld = (k + 3) & ~3
    pack_bytes = 2 * 4 * V * ld
    emit(what="pack kernel + row flags (empty document range)", bytes=pack_bytes, frac_of_hbm_peak=pack_bytes / (r_pack["device_ms_median"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
         frac_of_hbm_achievable=pack_bytes / (r_pack["device_ms_median"] * 1e-3) / 1e9 / HBM_ACHIEVABLE_GBS,
         note="the row-flag kernel reads the packed model once more (4 V ld bytes), not counted in bytes", **r_pack)
    comp_ms = r_no["device_ms_median"] - r_host["device_ms_median"] - r_pack["device_ms_median"]
    comp_bytes = 2 * 4 * D * k + a["nentries"] * 8   # counting pass + write pass each read the chunk's dense weights
    emit(what="compaction (count + scan + write), by difference: resident - host - pack", device_ms=comp_ms,
         noise_ms=r_no["device_ms_spread"] + r_host["device_ms_spread"] + r_pack["device_ms_spread"], bytes=int(comp_bytes),
         frac_of_hbm_peak=(comp_bytes / (comp_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if comp_ms > 0 else None,
         iteration_kernels="the same launches in both paths; the difference above also holds their run-to-run noise")
    emit(what="summary", same_bits_as_host_path=bool(same), docs_per_s_device_resident=D / r_no["device_ms_median"] * 1e3,
         docs_per_s_device_host=D / r_host["device_ms_median"] * 1e3, wall_speedup_entries_fetched=r_host["wall_ms_median"] / r_fetch["wall_ms_median"],
         config3="unmeasured: 100 k x 1000 model with resident A (10 M documents) was not run; the dense path needs 40 GB of weights there")
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
