#!/usr/bin/env python3
"""Timing probe for isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs on the configuration-2 corpus (50 k words, 1 M
documents, ~108 M entries), plain and with 1 % of the columns overwritten by copies of other columns (tools/dup_probe.py's way), medians
of 5 in one process after a warm-up:
  (a) doc_lengths: wall time and device time (the growth of ISLE_T_INGEST);
  (b) doc_duplicates with the full 64-bit hash on the whole corpus, and in both forms of the hash on its first `narrow_docs` documents:
      the narrow form needs as many rounds as a run holds distinct contents, a quarter of the documents, and each round reads a counter
      back, so on the whole corpus it would measure a million synchronisations and nothing else;
  (c) prune_docs(min_words=5, drop_duplicates=True), each repetition on a fresh upload (the upload is not timed): wall and device time;
  (d) the only way there was before: A fetched (get_A), then the numpy rule of tests/docs_rule.py on the host; the two parts timed apart.
One JSON line per measurement; no time is expected in advance.
  docs_prune_probe.py [out.jsonl] [docs] [narrow_docs]      (default: profiles/docs_prune_c2.jsonl, 1 000 000 documents, 20 000)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from isle_amd import HotPath  # noqa: E402
from tools.dup_probe import with_duplicates  # noqa: E402
from tools.synth import Corpus  # noqa: E402

REPS = 5


def main():
    import docs_rule as dr
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "docs_prune_c2.jsonl")
    V, k, D = 50_000, 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    narrow_docs = min(D, int(sys.argv[3]) if len(sys.argv) > 3 else 20_000)
    cnt, rows, offs = Corpus(V, D, k, 1).A()
    plain = dict(V=V, D=D, vals=np.asarray(cnt, np.float32), rows=np.asarray(rows, np.uint32), offs=np.asarray(offs, np.int64))
    copied = with_duplicates(plain, 0.01)[0]
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
        return dict(wall_ms_median=float(np.median(wall)), wall_ms=wall, device_ms_median=float(np.median(dev)), device_ms=dev), res

    for name, A in (("plain", plain), ("1 % of the columns copies", copied)):
        c, r, o = A["vals"], A["rows"], A["offs"]
        shape = dict(corpus=name, V=V, docs=D, entries=int(r.size), reps=REPS)
        case = dr.Case("c2", V, o, r, c, 5, 0, 0, 0, 1, "probe")
        up = lambda: hp.upload_counts(V, c, r, o)  # noqa: E731
        up()
        # (a)
        t, (words, tokens) = series(hp.doc_lengths)
        w_want, t_want = dr.lengths(o, c)
        emit(what="doc_lengths", same_as_the_numpy_rule=bool(np.array_equal(words, w_want) and np.array_equal(tokens, t_want)), **t, **shape)
        # (b) the full hash on the whole corpus
        hp.doc_hash_form("full")
        t, dup = series(hp.doc_duplicates)
        emit(what="doc_duplicates, 64-bit hash", n_duplicates=dup["n_duplicates"], **t, **shape)
        # ... and both forms on the first narrow_docs documents
        e = int(o[narrow_docs])
        hp.upload_counts(V, c[:e], r[:e], o[:narrow_docs + 1])
        first = {}
        for form in ("full", "narrow"):
            hp.doc_hash_form(form)
            t, dup = series(hp.doc_duplicates)
            first[form] = dup["first_of"]
            emit(what="doc_duplicates on the first %d documents, %s hash" % (narrow_docs, "64-bit" if form == "full" else "2-bit"), form=form,
                 n_duplicates=dup["n_duplicates"], **t, **dict(shape, docs=narrow_docs, entries=e))
        hp.doc_hash_form("auto")
        assert np.array_equal(first["full"], first["narrow"])
        # (c) the prune, each on a fresh upload
        t, got = series(lambda: hp.prune_docs(min_words=5, drop_duplicates=True), before=up)
        c2, r2, o2 = hp.get_A()
        want = dr.rule(case)
        same = bool(np.array_equal(got["kept_docs"], want["kept_docs"]) and np.array_equal(got["first_of"], want["first_of"]) and np.array_equal(o2, want["offs"]) and
                    np.array_equal(r2, want["rows"]) and np.array_equal(c2.view(np.uint32), want["counts"]) and
                    [got["dropped_short"], got["dropped_long"], got["dropped_duplicate"]] == want["dropped"])
        emit(what="prune_docs(min_words=5, drop_duplicates=True)", docs_kept=got["docs"], entries_kept=got["nnz"], dropped_short=got["dropped_short"],
             dropped_duplicate=got["dropped_duplicate"], same_as_the_numpy_rule=same, **t, **shape)
        # (d) the host way: fetch A, then the numpy rule
        up()
        fetch, rule = [], []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            fc, fr, fo = hp.get_A()
            t1 = time.perf_counter()
            dr.rule(dr.Case("c2", V, fo, fr, fc, 5, 0, 0, 0, 1, "probe"))
            t2 = time.perf_counter()
            if rep:
                fetch.append((t1 - t0) * 1e3)
                rule.append((t2 - t1) * 1e3)
        emit(what="the host way: get_A, then the numpy rule", fetch_A_ms_median=float(np.median(fetch)), fetch_A_ms=fetch, numpy_rule_ms_median=float(np.median(rule)),
             numpy_rule_ms=rule, host_path_ms=float(np.median(fetch) + np.median(rule)), note="the pruned matrix is not uploaded again in this figure", **shape)
    emit(what="summary", unmeasured=["a lane or a run of entries per document instead of a wave, in the hash pass and in the copy", "the narrow form's width",
                                     "the narrow form on the whole corpus", "several ranks"])
    hp.close()
    with open(out_path, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
