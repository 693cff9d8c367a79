"""UMass topic coherence on the device (isle_hip_topic_coherence, HotPath.topic_coherence).

Checker: brute force in this file.  The rows of A that belong to the distinct top words are binarised into a |U| x D scipy.sparse
matrix X and X X^T gives every D(w) (diagonal) and D(w_a, w_b).  The counts must be EQUAL; the coherence is then evaluated in fp64
in the stated order (i ascending, then j ascending) with math.log — the C library's log, which the library calls too (numpy's
vectorised log may differ from it in the last bit) — and must be bit-equal.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from isle_amd import IsleHipError
from isle_amd.hot_path import catchword_rank, model_rank_threshold, top_words

pytestmark = pytest.mark.gpu
EPS = 1e-5


def brute(V, rows, offs, tw, eps=EPS):
    """-> (coherence (n,), doc_freq (n, M), co_doc_freq (n, M(M-1)/2)) for the top-word table tw."""
    tw = np.asarray(tw, np.int64)
    n, M = tw.shape
    rows = np.asarray(rows, np.int64)
    offs = np.asarray(offs, np.int64)
    D = offs.shape[0] - 1
    U = np.unique(tw)
    lut = np.full(V, -1, np.int64)
    lut[U] = np.arange(U.size)
    sel = np.flatnonzero(lut[rows] >= 0)
    doc = np.searchsorted(offs, sel, side="right") - 1
    X = sp.csr_matrix((np.ones(sel.size, np.int64), (lut[rows[sel]], doc)), shape=(U.size, D))
    G = (X @ X.T).tocsr()
    loc = lut[tw]
    df = np.asarray(G[loc.ravel(), loc.ravel()]).ravel().reshape(n, M).astype(np.uint64)
    ii, jj = [], []
    for i in range(1, M):
        for j in range(i):
            ii.append(i)
            jj.append(j)
    ii, jj = np.array(ii, np.int64), np.array(jj, np.int64)
    if ii.size:
        co = np.asarray(G[loc[:, ii].ravel(), loc[:, jj].ravel()]).ravel().reshape(n, ii.size).astype(np.uint64)
    else:
        co = np.zeros((n, 0), np.uint64)
    coh = np.empty(n, np.float64)
    for t in range(n):
        s, undefined = 0.0, False
        for p in range(ii.size):
            dij, dj = int(co[t, p]), int(df[t, jj[p]])
            if dj == 0:
                undefined = True
                continue
            s += math.log(float(dij) + eps) - math.log(float(dj))
        coh[t] = math.nan if undefined else s
    return coh, df, co


def check(hp, V, rows, offs, tw, eps=EPS):
    got = hp.topic_coherence(tw, eps=eps)
    coh, df, co = brute(V, rows, offs, tw, eps)
    np.testing.assert_array_equal(got["doc_freq"], df)
    np.testing.assert_array_equal(got["co_doc_freq"], co)
    assert np.array_equal(np.isnan(got["coherence"]), np.isnan(coh))
    ok = ~np.isnan(coh)
    assert np.array_equal(got["coherence"][ok].view(np.uint64), coh[ok].view(np.uint64))  # bit for bit
    return got


def upload(hp, V, counts, rows, offs):
    hp.upload_counts(V, counts, rows, offs)


def hand_A(V, docs):
    """Count matrix from a list of word-id collections (one per document): counts 1, rows ascending."""
    offs = np.zeros(len(docs) + 1, np.int64)
    rows = []
    for d, w in enumerate(docs):
        w = np.unique(np.asarray(w, np.int64))
        rows.append(w)
        offs[d + 1] = offs[d] + w.size
    rows = np.concatenate(rows).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    return np.ones(rows.size, np.float32), rows, offs


def device_model_top_words(hp, V, D, k, seed, Ms):
    """Corpus A on the device, thresholded; catchwords + topic model with the planted partition; top words of the model."""
    from tools.synth import Corpus
    c = Corpus(V, D, k, seed)
    cnt, rows, offs = c.A()
    upload(hp, V, cnt, rows, offs)
    hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    assign = c.planted()[oc].astype(np.uint32)
    hp.find_catchwords(k, catchword_rank(D, k), assign=assign, fetch_thresholds=False)
    model = hp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)["model"]
    return cnt, rows, offs, model, {M: top_words(model, M) for M in Ms}


@pytest.mark.parametrize("V,D,k,seed", [(3000, 12000, 10, 2), (5000, 30000, 20, 3)])
def test_counts_and_coherence_on_the_device_topic_model(hp, V, D, k, seed):
    cnt, rows, offs, model, tws = device_model_top_words(hp, V, D, k, seed, (5, 10))
    for M, tw in tws.items():
        assert tw.shape == (k, M)
        got = check(hp, V, rows, offs, tw)
        assert np.isfinite(got["coherence"]).mean() > 0.9
    # the same counts through the helper on the flat column-major buffer (what get_basic_model writes)
    np.testing.assert_array_equal(top_words(model.ravel(order="F"), 5, vocab_size=V), tws[5])


def test_shared_words_and_identical_topics(hp):
    from tools.synth import Corpus
    V, D = 3000, 12000
    cnt, rows, offs = Corpus(V, D, 10, 4).A()
    upload(hp, V, cnt, rows, offs)
    freq = np.bincount(rows.astype(np.int64), minlength=V)
    hot = np.argsort(-freq, kind="stable")[:12]                  # the most frequent words, in many topics at once
    rng = np.random.default_rng(1)
    topics = []
    for t in range(60):
        w = list(rng.choice(hot, 3, replace=False)) + list(rng.choice(V, 3, replace=False))
        while len(set(w)) < 6:
            w = list(rng.choice(hot, 3, replace=False)) + list(rng.choice(V, 3, replace=False))
        topics.append(w)
    topics += [topics[0], topics[0], topics[5], list(hot[:6]), list(hot[:6])]   # identical topics
    tw = np.array(topics, np.uint32)
    got = check(hp, V, rows, offs, tw)
    assert got["coherence"][60] == got["coherence"][0] == got["coherence"][61]
    assert got["coherence"][63] == got["coherence"][64]


@pytest.mark.parametrize("M", [1, 2, 32])
def test_M_1_2_32(hp, M):
    from tools.synth import Corpus
    V, D = 3000, 12000
    cnt, rows, offs = Corpus(V, D, 10, 5).A()
    upload(hp, V, cnt, rows, offs)
    freq = np.bincount(rows.astype(np.int64), minlength=V)
    present = np.flatnonzero(freq > 0)
    rng = np.random.default_rng(M)
    tw = np.stack([rng.choice(present[:400] if t % 2 else present, M, replace=False) for t in range(40)]).astype(np.uint32)
    got = check(hp, V, rows, offs, tw)
    if M == 1:
        assert (got["coherence"] == 0.0).all() and got["co_doc_freq"].shape == (40, 0)
    assert got["co_doc_freq"].shape == (40, M * (M - 1) // 2)


def test_word_in_no_document(hp):
    rng = np.random.default_rng(3)
    V, D = 60, 300
    docs = [rng.choice(50, rng.integers(0, 20), replace=False) for _ in range(D)]   # words 50..59 occur nowhere
    cnt, rows, offs = hand_A(V, docs)
    upload(hp, V, cnt, rows, offs)
    tw = np.array([[1, 2, 3, 4],
                   [55, 2, 3, 4],      # absent word first: a denominator -> NaN
                   [1, 2, 3, 55],      # absent word last: never a denominator -> finite (ln eps terms)
                   [1, 57, 3, 4],      # absent word in a denominator -> NaN
                   [56, 57, 58, 59],   # nothing present -> NaN
                   [0, 1, 2, 3]], np.uint32)
    got = check(hp, V, rows, offs, tw)
    nan = np.isnan(got["coherence"])
    assert list(nan) == [False, True, False, True, True, False]
    assert got["doc_freq"][2, 3] == 0 and (got["co_doc_freq"][2, 3:6] == 0).all()
    single = hp.topic_coherence(np.array([[55]], np.uint32))   # M = 1: no denominator at all
    assert single["coherence"][0] == 0.0 and single["doc_freq"][0, 0] == 0


def test_tiled_counters(hp):
    """2000 topics x 20 random words: about 5000 distinct words and 370 000 distinct pairs, far beyond one LDS tile of counters
    (under 30 000 u32), so the pairs are counted over many passes."""
    from tools.synth import Corpus
    V, D = 5000, 30000
    cnt, rows, offs = Corpus(V, D, 20, 6).A()
    upload(hp, V, cnt, rows, offs)
    rng = np.random.default_rng(7)
    tw = np.stack([rng.choice(V, 20, replace=False) for _ in range(2000)]).astype(np.uint32)
    got = check(hp, V, rows, offs, tw)
    assert np.isfinite(got["coherence"]).sum() > 0


def test_global_lookup_table_above_the_bitmap_bound(hp):
    """V = 300 000 > 131 072: the membership bitmap does not fit in LDS and the word -> local id table in HBM is used."""
    rng = np.random.default_rng(8)
    V, D = 300000, 3000
    pool = np.sort(rng.choice(V, 4000, replace=False))
    pool[-1] = V - 1
    docs = [rng.choice(pool, rng.integers(1, 120), replace=False) for _ in range(D)]
    cnt, rows, offs = hand_A(V, docs)
    upload(hp, V, cnt, rows, offs)
    hi = pool[pool > 200000]
    tw = np.stack([np.concatenate([rng.choice(hi, 3, replace=False), rng.choice(pool[:2000], 3, replace=False)]) for _ in range(300)])
    tw[0, 0] = V - 1
    got = check(hp, V, rows, offs, tw.astype(np.uint32))
    assert got["doc_freq"][0, 0] > 0


def test_hit_list_overflow_empty_documents_and_one_document(hp):
    """A document holding every word of U (|U| >= 1000, more hits than a wave's list holds) takes the slower path; empty documents
    count nothing; a corpus of ONE document."""
    rng = np.random.default_rng(9)
    V = 2000
    docs = [np.arange(V), [], np.arange(0, V, 2), [], rng.choice(V, 30, replace=False), np.arange(500, 1700)]
    cnt, rows, offs = hand_A(V, docs)
    upload(hp, V, cnt, rows, offs)
    tw = np.stack([rng.choice(1500, 8, replace=False) for _ in range(400)]).astype(np.uint32)
    assert np.unique(tw).size >= 1000
    check(hp, V, rows, offs, tw)
    cnt1, rows1, offs1 = hand_A(V, [np.arange(V)])
    upload(hp, V, cnt1, rows1, offs1)
    got = check(hp, V, rows1, offs1, tw)
    assert (got["doc_freq"] == 1).all() and (got["co_doc_freq"] == 1).all()


def test_config2_size(hp):
    """Config 2 size (50 000 words x 1 M documents, k = 200), top words of the device's own topic model."""
    V, D, k = 50000, 1000000, 200
    cnt, rows, offs, model, tws = device_model_top_words(hp, V, D, k, 11, (5,))
    check(hp, V, rows, offs, tws[5])


def test_two_calls_are_bit_identical(hp):
    from tools.synth import Corpus
    V, D = 5000, 30000
    cnt, rows, offs = Corpus(V, D, 20, 12).A()
    upload(hp, V, cnt, rows, offs)
    rng = np.random.default_rng(13)
    tw = np.stack([rng.choice(V, 10, replace=False) for _ in range(500)]).astype(np.uint32)
    a, b = hp.topic_coherence(tw), hp.topic_coherence(tw)
    for key in ("coherence", "doc_freq", "co_doc_freq"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_argument_errors(hp):
    from isle_amd import HotPath
    fresh = HotPath(0)
    try:
        with pytest.raises(IsleHipError, match="no count matrix"):
            fresh.topic_coherence(np.array([[1, 2]], np.uint32))
    finally:
        fresh.close()

    two = HotPath(0)
    try:
        def exchange(kind, a, count):
            raise AssertionError("no collective expected")
        two.comm_init_host(2, 0, exchange)
        cnt, rows, offs = hand_A(10, [[1, 2], [2, 3]])
        two.upload_counts(10, cnt, rows, offs)
        with pytest.raises(IsleHipError, match="single-rank"):
            two.topic_coherence(np.array([[1, 2]], np.uint32))
    finally:
        two.close()

    cnt, rows, offs = hand_A(10, [[1, 2], [2, 3]])
    upload(hp, 10, cnt, rows, offs)
    with pytest.raises(IsleHipError, match="num_topics"):
        hp.topic_coherence(np.zeros((0, 3), np.uint32))
    with pytest.raises(IsleHipError, match="M = 0"):
        hp.topic_coherence(np.zeros((2, 0), np.uint32))
    with pytest.raises(IsleHipError, match="M = 33"):
        hp.topic_coherence(np.arange(33, dtype=np.uint32)[None, :] % 10)
    with pytest.raises(IsleHipError, match="vocab"):
        hp.topic_coherence(np.array([[1, 10]], np.uint32))
    with pytest.raises(IsleHipError, match="repeats"):
        hp.topic_coherence(np.array([[1, 2], [3, 3]], np.uint32))
    ok = hp.topic_coherence(np.array([[1, 2], [2, 3]], np.uint32))   # the context is still usable
    assert np.isfinite(ok["coherence"]).all()
