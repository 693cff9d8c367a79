#!/usr/bin/env python3
"""Timing probe for isle_hip_compare_models / isle_hip_match_topics at the shapes of configuration 2 (50 k words, 200 x 200 topics) and
configuration 3 (100 k words, 1000 x 1000 topics), medians of 5 in one process after a warm-up, with min and max:
  (a) compare_models on two generated host models (random columns on the simplex): wall time (the two uploads included) and device
      time (the growth of ISLE_T_POST: distances, matcher; no copies), with the matrix fetched and with only the matching fetched;
  (b) the distances alone (match=False, nothing fetched but the matrix) at slices = 1 and at the rule's choice (slices = 0);
  (c) the only way there was before, on the same arrays: numpy abs(a[:, :, None] - b[:, None, :]) in blocks of words, once (configuration
      2) or once on a 100 x 100 sub-block and SCALED by the number of such blocks (configuration 3: scaled, not measured);
  (d) the achieved rate of (b): terms per second, and as a share of the FP32 vector peak of 157.3 TFLOPS counted at 2 operations a term
      (no FP64 vector figure is quoted: the guides give none);
  (e) the matcher: rounds and device time on a real pair (a small trained catch model against the same model loaded back from its
      text), on the 200 x 200 and 1000 x 1000 distance matrices of (a), and on the worst case dist[i][j] = i + j at 1000 x 1000.
One JSON line per measurement; no time is expected in advance.
  model_compare_probe.py [out.jsonl] [c2|c3|both]      (default: profiles/model_compare_c3.jsonl, both)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isle_amd import HotPath  # noqa: E402

REPS = 5
PEAK_FP32_VECTOR = 157.3e12


def simplex(rng, V, k):
    m = rng.random((V, k), np.float32)
    m /= m.sum(axis=0, keepdims=True)
    return np.asfortranarray(m, np.float32)


def host_blocks(a, b, words=256):
    """the host loop: abs differences in blocks of words, float64"""
    out = np.zeros((a.shape[1], b.shape[1]))
    for w in range(0, a.shape[0], words):
        x, y = a[w:w + words].astype(np.float64), b[w:w + words].astype(np.float64)
        out += np.abs(x[:, :, None] - y[:, None, :]).sum(axis=0)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "model_compare_c3.jsonl")
    which = sys.argv[2] if len(sys.argv) > 2 else "both"
    hp = HotPath(0)
    hp.timing_enable(True)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def series(fn):
        wall, dev, res = [], [], None
        for rep in range(REPS + 1):  # the first round is the warm-up
            hp.synchronize()
            before = hp.timing_get()["post"][0]
            t0 = time.perf_counter()
            res = fn()
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                wall.append(w)
                dev.append(hp.timing_get()["post"][0] - before)
        return dict(wall_ms_median=float(np.median(wall)), wall_ms_min=min(wall), wall_ms_max=max(wall), device_ms_median=float(np.median(dev)),
                    device_ms_min=min(dev), device_ms_max=max(dev)), res

    rng = np.random.default_rng(0)
    shapes = [s for s in (("c2", 50_000, 200), ("c3", 100_000, 1000)) if which in ("both", s[0])]
    for name, V, k in shapes:
        a, b = simplex(rng, V, k), simplex(rng, V, k)
        shape = dict(shape=name, V=V, cols_a=k, cols_b=k, reps=REPS)
        hp.model_dist_slices(0)
        t, full = series(lambda: hp.compare_models(a, b))
        emit(what="compare_models, matrix and matching fetched", rounds=full["rounds"], n_matched=full["n_matched"], **t, **shape)
        t, only = series(lambda: hp.compare_models(a, b, fetch_dist=False))
        emit(what="compare_models, only the matching fetched", rounds=only["rounds"], same_matching=bool(np.array_equal(only["match_a"], full["match_a"])), **t, **shape)
        terms = float(V) * k * k
        per_slices = {}
        for slices in (1, 0):
            hp.model_dist_slices(slices)
            t, d = series(lambda: hp.compare_models(a, b, match=False))
            per_slices[slices] = d["dist"]
            rate = terms / (t["device_ms_median"] * 1e-3)
            emit(what="distances alone, slices = %s" % ("1" if slices else "the rule's choice"), slices_asked=slices, terms=terms, terms_per_s=rate,
                 share_of_fp32_vector_peak_at_2_ops_a_term=2 * rate / PEAK_FP32_VECTOR, **t, **shape)
        hp.model_dist_slices(0)
        spread = float(np.abs(per_slices[0] - per_slices[1]).max() / per_slices[1].max())
        emit(what="slices = 1 against the rule's choice: largest difference over the largest distance", value=spread, **shape)
        t, m = series(lambda: hp.match_topics(full["dist"]))
        emit(what="match_topics on that distance matrix", rounds=m["rounds"], n_matched=m["n_matched"], **t, **shape)
        # (c) the host way
        if name == "c2":
            t0 = time.perf_counter()
            ref = host_blocks(a, b)
            host_ms = (time.perf_counter() - t0) * 1e3
            emit(what="the host way: numpy abs differences in blocks of 256 words, once", host_ms=host_ms, measured=True,
                 largest_relative_difference_to_the_device=float((np.abs(ref - full["dist"]) / ref).max()), **shape)
        else:
            t0 = time.perf_counter()
            ref = host_blocks(a[:, :100], b[:, :100])
            sub_ms = (time.perf_counter() - t0) * 1e3
            emit(what="the host way on a 100 x 100 sub-block, once, SCALED by %d blocks (scaled, not measured)" % ((k // 100) ** 2), sub_block_ms=sub_ms,
                 host_ms_scaled=sub_ms * (k // 100) ** 2, measured=False,
                 largest_relative_difference_to_the_device=float((np.abs(ref - full["dist"][:100, :100]) / ref).max()), **shape)
        del a, b
    # (e) the matcher on a real pair and on its worst case
    from isle_amd.hot_path import catchword_rank, model_rank_threshold
    from tools.synth import Corpus
    V, D, k = 5000, 30000, 20
    c = Corpus(V, D, k, 3)
    cnt, rows, offs = c.A()
    hp.upload_counts(V, cnt, rows, offs)
    hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    hp.find_catchwords(k, max(catchword_rank(D, k), 1), assign=c.planted()[oc].astype(np.uint32), fetch_thresholds=False)
    hp.construct_topic_model(k, max(model_rank_threshold(D, k), 1), D, fetch_sums=False)
    hp.load_model_text(hp.model_text("catch", "sparse"), V, k, "sparse")
    t, r = series(lambda: hp.compare_models("catch", "loaded"))
    emit(what="a trained catch model against itself loaded back from its sparse text", V=V, cols_a=k, cols_b=k, rounds=r["rounds"], n_matched=r["n_matched"],
         mean_dist=r["mean_dist"], identity=bool(np.array_equal(r["match_a"], np.arange(k))), reps=REPS, **t)
    i = np.arange(1000, dtype=np.float64)
    t, r = series(lambda: hp.match_topics(i[:, None] + i[None, :]))
    emit(what="match_topics on dist[i][j] = i + j, 1000 x 1000: the worst case", rounds=r["rounds"], n_matched=r["n_matched"], reps=REPS, **t)
    emit(what="summary", unmeasured=["resident models on both sides at these shapes (the wall times include two uploads)", "several ranks",
                                     "other tile and chunk sizes than 64 x 64 pairs and 64 words", "a k above 1000"])
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
