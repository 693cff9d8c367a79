#!/usr/bin/env python3
"""Timing probe for isle_hip_doc_signatures / isle_hip_doc_near_duplicates / isle_hip_prune_near_docs on the configuration-2 corpus (50 k
words, 1 M documents, ~108 M entries), plain and with 1 % of the documents planted as copies of earlier ones with about a tenth of their
words replaced; medians of 5 in one process after a warm-up, with the five values (min - max):
  (a) doc_signatures, keys only (what the prune computes), 16 x 4: wall time and device time (the growth of ISLE_T_INGEST), and what the
      pass reaches of the 157 TFLOPS vector figure counted in 32-bit integer operations: a hash is OPS_PER_HASH of them (the ISA of docs_mix
      on gfx950: 17 vector instructions — a 64-bit add, three 64-bit shifts, six xors, four 32-bit multiplies, two 32 x 32 -> 64 multiplies,
      two three-operand adds — counted as 26 32-bit operations, and 4 for the 64-bit minimum; the hand-round shuffle and the loop are not
      counted);
  (b) near_duplicates at 16 x 4 and threshold 4/5, with n_dropped, pairs_tested and rounds;
  (c) prune_near_docs, each repetition on a fresh upload (the upload is not timed);
  (d) the sibling, prune_docs(drop_duplicates=True), the same way;
  (e) the path a user has today: A fetched (get_A), then the numpy rule of tests/neardup_rule.py on the host — run ONCE, on the first
      `rule_docs` documents; the figure for the whole corpus is scaled from it by the entries and labelled "scaled, not measured".
One JSON line per measurement; no time is expected in advance.
  near_dups_probe.py [out.jsonl] [docs] [rule_docs]      (default: profiles/near_dups_c2.jsonl, 1 000 000 documents, 20 000)"""
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
BANDS, ROWS, NUM, DEN = 16, 4, 4, 5
OPS_PER_HASH = 30
VECTOR_PEAK = 157e12


def with_near_copies(V, cnt, rows, offs, share, seed):
    """share of the documents become copies of an earlier document with about a tenth of its words replaced -> (cnt, rows, offs, planted)"""
    rng = np.random.default_rng(seed)
    D = offs.size - 1
    planted = np.sort(rng.choice(np.arange(1, D), size=int(D * share), replace=False))
    pieces_c, pieces_r, lens = [], [], np.diff(offs).copy()
    at = 0
    for d in planted.tolist():
        pieces_c.append(cnt[offs[at]:offs[d]])
        pieces_r.append(rows[offs[at]:offs[d]])
        src = int(rng.integers(0, d))
        w = rows[offs[src]:offs[src + 1]].astype(np.int64)
        swap = rng.random(w.size) < 0.1
        w[swap] = rng.integers(0, V, size=int(swap.sum()))
        w, first = np.unique(w, return_index=True)
        pieces_r.append(w.astype(np.uint32))
        pieces_c.append(cnt[offs[src]:offs[src + 1]][first])
        lens[d] = w.size
        at = d + 1
    pieces_c.append(cnt[offs[at]:])
    pieces_r.append(rows[offs[at]:])
    new_offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(pieces_c).astype(np.float32), np.concatenate(pieces_r).astype(np.uint32), new_offs, planted


def main():
    import neardup_rule as nr
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "near_dups_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    rule_docs = min(D, int(sys.argv[3]) if len(sys.argv) > 3 else 20_000)
    cnt, rows, offs = Corpus(V, D, k, 1).A()
    cnt, rows, offs = np.asarray(cnt, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    pc, pr, po, planted = with_near_copies(V, cnt, rows, offs, 0.01, 3)
    hp = HotPath(0)
    hp.timing_enable(True)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn):
        hp.synchronize()
        before = hp.timing_get()["ingest"][0]
        t0 = time.perf_counter()
        res = fn()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, hp.timing_get()["ingest"][0] - before, res

    def series(fn, before=None):
        wall, dev, res = [], [], None
        for rep in range(REPS + 1):  # the first round is the warm-up
            if before:
                before()
            w, d, res = timed(fn)
            if rep:
                wall.append(w)
                dev.append(d)
        return dict(wall_ms_median=float(np.median(wall)), wall_ms=wall, wall_ms_min_max=[min(wall), max(wall)], device_ms_median=float(np.median(dev)),
                    device_ms=dev, device_ms_min_max=[min(dev), max(dev)]), res

    for name, (c, r, o) in (("plain", (cnt, rows, offs)), ("1 % of the documents near copies", (pc, pr, po))):
        shape = dict(corpus=name, V=V, docs=D, entries=int(r.size), bands=BANDS, rows_per_band=ROWS, reps=REPS)
        up = lambda: hp.upload_counts(V, c, r, o)  # noqa: E731
        up()
        # (a) the signature pass, keys only
        t, got = series(lambda: hp.doc_signatures(BANDS, ROWS, sig=False))
        part = nr.band_keys(nr.signatures(o[:2001], r[:int(o[2000])], BANDS * ROWS), BANDS, ROWS)
        ops = float(r.size) * BANDS * ROWS * OPS_PER_HASH
        emit(what="doc_signatures, keys only", same_as_the_numpy_rule_on_the_first_2000_documents=bool(np.array_equal(got["keys"][:, :2000], part)),
             hashes=int(r.size) * BANDS * ROWS, int32_ops_per_hash=OPS_PER_HASH, share_of_157_tflops=ops / (t["device_ms_median"] * 1e-3) / VECTOR_PEAK, **t, **shape)
        # (b) the search
        t, nd = series(lambda: hp.near_duplicates((NUM, DEN), BANDS, ROWS))
        found = int((nd["first_of"][planted] != planted).sum()) if name != "plain" else None
        emit(what="near_duplicates, threshold 4/5", n_dropped=nd["n_dropped"], pairs_tested=nd["pairs_tested"], rounds=nd["rounds"], planted=int(planted.size) if found is not None else 0,
             planted_found=found, **t, **shape)
        # (c) the prune, each on a fresh upload
        t, got = series(lambda: hp.prune_near_docs((NUM, DEN), BANDS, ROWS), before=up)
        emit(what="prune_near_docs, threshold 4/5", docs_kept=got["docs"], entries_kept=got["nnz"], n_dropped=got["n_dropped"],
             same_first_of_as_near_duplicates=bool(np.array_equal(got["first_of"], nd["first_of"])), **t, **shape)
        # (d) the sibling: exact duplicates
        t, got = series(lambda: hp.prune_docs(min_words=0, drop_duplicates=True), before=up)
        emit(what="prune_docs(min_words=0, drop_duplicates=True), the sibling", docs_kept=got["docs"], dropped_duplicate=got["dropped_duplicate"], **t, **shape)
        # (e) the path a user has today: fetch A, then the numpy rule, once, on the first rule_docs documents
        up()
        fetch = []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            fc, fr, fo = hp.get_A()
            if rep:
                fetch.append((time.perf_counter() - t0) * 1e3)
        e = int(fo[rule_docs])
        case = nr.Case("c2_first, " + name, V, fo[:rule_docs + 1], fr[:e], fc[:e], NUM, DEN, BANDS, ROWS, np.zeros((0, 2), np.uint32), "probe")
        t0 = time.perf_counter()
        want = nr.rule(case, "full")
        rule_ms = (time.perf_counter() - t0) * 1e3
        hp.upload_counts(V, fc[:e], fr[:e], fo[:rule_docs + 1])
        part = hp.near_duplicates((NUM, DEN), BANDS, ROWS)
        same = bool(np.array_equal(part["first_of"], want["first_of"]) and np.array_equal(part["parent"], want["parent"]) and
                    (part["pairs_tested"], part["rounds"]) == (want["pairs_tested"], want["rounds"]))
        emit(what="the host way: get_A, then the numpy rule on the first %d documents (once)" % rule_docs, fetch_A_ms_median=float(np.median(fetch)), fetch_A_ms=fetch,
             numpy_rule_ms_once=rule_ms, rule_docs=rule_docs, rule_entries=e, device_equals_the_rule_there=same,
             numpy_rule_ms_whole_corpus=rule_ms * r.size / max(e, 1), numpy_rule_ms_whole_corpus_is="scaled, not measured", **shape)
    keys_bytes = 8 * BANDS * D
    emit(what="summary", derived_not_measured=dict(keys_bytes=keys_bytes, note="device memory beyond A: 8 bands D bytes of keys (128 MB at config 2, 1.3 GB at config 3: "
                                                   "10 M documents) plus the sort's twin buffers"),
         unmeasured=["config 3", "the alternative dealing of the signature pass (a lane per entry, H minima in registers or LDS)", "the narrow form at size",
                     "a merge in the place of the bisection in the intersection", "several ranks"])
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
