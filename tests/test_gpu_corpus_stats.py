"""The trainer's corpus diagnostics on the device (isle_hip_log_combinatorial / isle_hip_distinct_top_five, HotPath.log_combinatorial /
HotPath.distinct_top_five_sets).

Checker: numpy in this file.  Log-combinatorial: the table is built as the reference builds it (the running sum in double with math.log,
the C library's log, stored as float32), and every document's value is formed by fp32 element-wise steps in the reference's entry order,
vectorised across documents; the results must be bit-equal.  Top five: the normalised values avg_doc_sz * (count / doc_sum) in fp32,
each qualifying document's 5 largest with multiplicity, the tuples sorted by np.lexsort; the device's sorted tuples must be bit-equal
and every count must equal the reference's loop, transliterated in test_corpus_stats_cpu.literal.
"""
import ctypes as C
import io
import math

import numpy as np
import pytest

from isle_amd import IsleHipError
from isle_amd.hot_path import catchword_rank, model_rank_threshold
from test_corpus_stats_cpu import literal

pytestmark = pytest.mark.gpu
MS = (2, 3, 5, 10, 20, 50, 100, 200, 500)


def log_fact(nmax):
    lf = np.zeros(nmax + 1, np.float32)
    x = 0.0
    for i in range(nmax):
        x = float(np.float32(x + math.log(i + 1)))   # (float)((double)log_fact[i] + log(i + 1))
        lf[i + 1] = x
    return lf


def log_comb_checker(cnt, offs):
    cnt = np.asarray(cnt, np.float32)
    offs = np.asarray(offs, np.int64)
    D = offs.size - 1
    ci = cnt.astype(np.int64)                                       # (int)count
    cs = np.concatenate([[0], np.cumsum(ci)])
    N = cs[offs[1:]] - cs[offs[:-1]]
    lf = log_fact(int(N.max()) if D else 0)
    lens = np.diff(offs)
    order = np.argsort(-lens, kind="stable")                         # longest first: the documents still walking form a prefix
    L, S = lens[order], offs[:-1][order]
    acc = np.zeros(D, np.float32)
    for j in range(int(L[0]) if D else 0):
        act = int(np.searchsorted(-L, -j, side="left"))             # documents with more than j entries
        acc[:act] -= lf[ci[S[:act] + j]]
    out = np.empty(D, np.float32)
    out[order] = acc + lf[N[order]]
    return out


def top5_checker(cnt, offs):
    """-> (sorted tuples float32 (n, 5), {m: count})."""
    cnt = np.asarray(cnt, np.float32)
    offs = np.asarray(offs, np.int64)
    D = offs.size - 1
    lens = np.diff(offs)
    tokens = int(cnt.astype(np.uint64).sum())
    avg = np.float32(tokens // max(int((lens > 0).sum()), 1))      # src/sparseMatrix.cpp:98, integer division
    cs = np.concatenate([[0.0], np.cumsum(cnt.astype(np.float64))])
    dsum = (cs[offs[1:]] - cs[offs[:-1]]).astype(np.float32)        # integer sums: exact
    doc = np.repeat(np.arange(D), lens)
    nv = avg * (cnt / dsum[doc])                                     # fp32, as post_normalize_k
    order = np.lexsort((-nv, doc))                                   # per document, value descending
    q = offs[:-1][lens >= 5]
    T = nv[order][q[:, None] + np.arange(5)]
    T = T[np.lexsort((T[:, 4], T[:, 3], T[:, 2], T[:, 1], T[:, 0]))]
    run = np.concatenate([[0], np.cumsum(np.any(T[1:] != T[:-1], axis=1))]).tolist() if len(T) else []
    return T, {m: literal(run, m) for m in MS}


def check(hp, cnt, offs, tuples=True):
    got = hp.log_combinatorial()
    want = log_comb_checker(cnt, offs)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))    # bit for bit
    t5 = hp.distinct_top_five_sets(m=MS, fetch_quintuples=tuples)
    T, counts = top5_checker(cnt, offs)
    assert t5["num_quintuples"] == len(T)
    assert int(t5["run_lengths"].sum()) == len(T)
    if tuples:
        assert t5["quintuples"].shape == T.shape
        assert np.array_equal(t5["quintuples"].view(np.uint32), T.view(np.uint32))
    assert t5["counts"] == counts
    return got, t5


def build_A(V, docs):
    """docs: list of (rows, counts) per document -> CSC (counts, rows, offs)."""
    offs = np.zeros(len(docs) + 1, np.int64)
    for d, (r, _) in enumerate(docs):
        offs[d + 1] = offs[d] + len(r)
    rows = np.concatenate([np.asarray(r, np.uint32) for r, _ in docs]) if docs else np.zeros(0, np.uint32)
    cnt = np.concatenate([np.asarray(c, np.float32) for _, c in docs]) if docs else np.zeros(0, np.float32)
    assert rows.size == 0 or rows.max() < V
    return cnt, rows, offs


def synth_docs(V, D, K, seed):
    from tools.synth import Corpus
    cnt, rows, offs = Corpus(V, D, K, seed).A()
    return [(rows[offs[d]:offs[d + 1]].copy(), cnt[offs[d]:offs[d + 1]].copy()) for d in range(D)]


def planted_docs(V, rng):
    """Groups of documents that share a count profile (so their top-five tuples are equal) with group sizes around every m, and the
    edge cases: empty, single-entry, 4 and exactly 5 entries, one document of more than 32 768 entries with a large word count."""
    docs = []
    sizes = [1, 2, 3, 4, 5, 6, 9, 10, 11, 19, 20, 21, 49, 50, 51, 99, 100, 101, 199, 200, 201, 499, 500, 501, 650]
    for g, size in enumerate(sizes):
        L = 5 + g % 7
        prof = np.sort(rng.integers(1, 9, size=L))[::-1].astype(np.float32)
        for _ in range(size):
            docs.append((np.sort(rng.choice(V, L, replace=False)), rng.permutation(prof)))
    docs += [(np.zeros(0, np.uint32), np.zeros(0, np.float32))] * 3
    docs += [([int(w)], [float(c)]) for w, c in zip(rng.choice(V, 40), rng.integers(1, 50, 40))]
    docs += [(np.sort(rng.choice(V, 4, replace=False)), rng.integers(1, 5, 4)) for _ in range(30)]
    docs += [(np.sort(rng.choice(V, 5, replace=False)), rng.integers(1, 5, 5)) for _ in range(30)]
    docs.append((np.arange(0, 40000), rng.integers(1, 6, 40000)))        # > 32 768 entries, N_d ~ 120 000: the table is read from HBM
    rng.shuffle(docs)
    return docs


def tdf_text(cnt, rows, offs):
    doc = np.repeat(np.arange(offs.size - 1), np.diff(offs)) + 1
    buf = io.BytesIO()
    np.savetxt(buf, np.stack([doc, rows.astype(np.int64) + 1, cnt.astype(np.int64)], axis=1), fmt="%d")
    return buf.getvalue()


@pytest.fixture(scope="module")
def planted():
    V = 50000
    rng = np.random.default_rng(21)
    docs = synth_docs(V, 6000, 20, 4) + planted_docs(V, rng)
    return (V,) + build_A(V, docs)


def test_planted_corpus_through_upload(hp, planted):
    V, cnt, rows, offs = planted
    hp.upload_counts(V, cnt, rows, offs)
    lc, t5 = check(hp, cnt, offs)
    lens = np.diff(offs)
    assert (lc[lens == 0] == 0).all()                                 # an empty document gives 0
    assert (lc[lens == 1] == 0).all()                                 # a single entry: log N! - log N!
    assert lens.max() > 32768
    assert t5["counts"][500] >= 1 and t5["counts"][2] > t5["counts"][500]   # the counts are not trivial


def test_planted_corpus_through_ingest(hp, planted):
    V, cnt, rows, offs = planted
    D = offs.size - 1
    r = hp.ingest_tdf(tdf_text(cnt, rows, offs), V, D)
    assert r["nnz"] == cnt.size
    check(hp, cnt, offs)


@pytest.mark.parametrize("V,D,K,seed", [(3000, 20000, 20, 5), (8000, 40000, 50, 6)])
def test_synthetic_corpora_both_ways(hp, V, D, K, seed):
    from tools.synth import Corpus
    c = Corpus(V, D, K, seed)
    cnt, rows, offs = c.A()
    hp.upload_counts(V, cnt, rows, offs)
    a = check(hp, cnt, offs)
    hp.ingest_tdf(c.tdf_bytes(), V, D)
    b = check(hp, cnt, offs, tuples=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1]["counts"] == b[1]["counts"]


def test_no_document_qualifies(hp):
    rng = np.random.default_rng(3)
    V = 100
    docs = [(np.sort(rng.choice(V, int(n), replace=False)), rng.integers(1, 7, int(n))) for n in rng.integers(0, 5, 500)]
    cnt, rows, offs = build_A(V, docs)
    hp.upload_counts(V, cnt, rows, offs)
    _, t5 = check(hp, cnt, offs)
    assert t5["num_quintuples"] == 0 and t5["quintuples"].shape == (0, 5)
    assert set(t5["counts"].values()) == {0}


def downstream(hp, c, V, D, k, diagnostics):
    cnt, rows, offs = c.A()
    hp.upload_counts(V, cnt, rows, offs)
    if diagnostics:
        hp.log_combinatorial()
        hp.distinct_top_five_sets(fetch_quintuples=True)
    hp.threshold(k)
    if diagnostics:
        hp.distinct_top_five_sets()
    oc = hp.get_B()["original_cols"].astype(np.int64)
    assign = c.planted()[oc].astype(np.uint32)
    cw = hp.find_catchwords(k, catchword_rank(D, k), assign=assign)
    if diagnostics:
        hp.log_combinatorial()
        hp.distinct_top_five_sets()
    tm = hp.construct_topic_model(k, model_rank_threshold(D, k), D)
    return cw, tm


def test_diagnostics_leave_catchwords_and_topic_model_unchanged(hp):
    from tools.synth import Corpus
    V, D, k = 4000, 20000, 20
    c = Corpus(V, D, k, 8)
    cw0, tm0 = downstream(hp, c, V, D, k, False)
    cw1, tm1 = downstream(hp, c, V, D, k, True)
    assert cw0["thresholds"].tobytes() == cw1["thresholds"].tobytes()
    assert cw0["catch_topic"].tobytes() == cw1["catch_topic"].tobytes()
    assert cw0["num_catchwords"] == cw1["num_catchwords"]
    for key in ("model_threshold", "top1", "top2", "dts_off", "dts_topic", "dts_val"):
        assert tm0[key].tobytes() == tm1[key].tobytes(), key
    np.testing.assert_allclose(tm1["model"], tm0["model"], rtol=2e-5, atol=0)   # fp32 atomics: the order of additions varies


def test_argument_errors(hp):
    from isle_amd import HotPath
    fresh = HotPath(0)
    try:
        with pytest.raises(IsleHipError, match="no count matrix"):
            fresh.log_combinatorial()
        with pytest.raises(IsleHipError, match="no count matrix"):
            fresh.distinct_top_five_sets()
    finally:
        fresh.close()
    cnt, rows, offs = build_A(10, [([1, 2, 3, 4, 5], [1, 2, 3, 4, 5]), ([2, 3], [1, 1])])
    hp.upload_counts(10, cnt, rows, offs)
    with pytest.raises(IsleHipError, match=r"m\[1\] = 1"):
        hp.distinct_top_five_sets(m=(2, 1))
    with pytest.raises(IsleHipError, match="m\\[0\\] = -3"):
        hp.distinct_top_five_sets(m=(-3,))
    lib, h = hp._lib, hp._h
    assert lib.isle_hip_log_combinatorial(h, None, None) != 0
    assert "null out" in lib.isle_hip_last_error(h).decode()
    ms = np.array([2], np.int32)
    assert lib.isle_hip_distinct_top_five(h, 1, ms.ctypes.data_as(C.c_void_p), None, None, None, None, None) != 0
    assert lib.isle_hip_distinct_top_five(h, -1, None, None, None, None, None, None) != 0
    assert lib.isle_hip_distinct_top_five(h, 0, None, None, None, None, None, None) == 0   # nothing asked: valid
    check(hp, cnt, offs)                                              # the context is still usable


def test_config2_size(hp):
    """Config 2 size (50 000 words x 1 M documents) under the same asserts."""
    from tools.synth import Corpus
    V, D = 50000, 1000000
    cnt, rows, offs = Corpus(V, D, 200, 11).A()
    hp.upload_counts(V, cnt, rows, offs)
    check(hp, cnt, offs)
