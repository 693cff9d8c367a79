"""The cluster-average topic model, on-device top-word selection and topic diversity (isle_hip_avg_topic_model,
isle_hip_model_top_words, isle_hip_topic_diversity; HotPath.avg_topic_model / model_top_words / topic_diversity).

Checkers: numpy in this file.  The average model is certified entry by entry against fp64 sums of the same fp32 normalised values
nv = avg * (cnt / doc_sum) (post_normalize_k's formula): |m - m64| <= 2^-22 |m64|, exact zeros, NaN columns exactly for empty
clusters, and bitwise identical repeats.  Top words must be bit-equal to hot_path.top_words (the trainer's rule); diversity must match
an fp64 restatement within 1e-10 relative.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from isle_amd import IsleHipError
from isle_amd.hot_path import catchword_rank, model_rank_threshold, top_words

pytestmark = pytest.mark.gpu
BOUND = 2.0 ** -22


def setup_post(hp, V, D, k, seed, assign_fn=None):
    """A uploaded and thresholded, a partition on B's columns, catchwords and the catch model.  -> dict for the checkers."""
    from tools.synth import Corpus
    c = Corpus(V, D, k, seed)
    cnt, rows, offs = c.A()
    hp.upload_counts(V, cnt, rows, offs)
    info = hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    assign = (c.planted()[oc] % k).astype(np.uint32) if assign_fn is None else assign_fn(oc, c)
    cl = np.full(D, -1, np.int64)
    cl[oc] = assign
    hp.find_catchwords(k, max(catchword_rank(D, k), 1), assign=assign, fetch_thresholds=False)
    catch = hp.construct_topic_model(k, max(model_rank_threshold(D, k), 1), D, fetch_sums=False)["model"]
    doc_sum = np.add.reduceat(cnt.astype(np.float64), offs[:-1]) if cnt.size else np.zeros(D)
    doc_sum[np.diff(offs) == 0] = 1.0
    lens = np.diff(offs)
    nv = np.float32(info["avg_doc_sz"]) * (cnt / np.repeat(doc_sum.astype(np.float32), lens))
    assert nv.dtype == np.float32
    return dict(V=V, D=D, k=k, cnt=cnt, rows=rows, offs=offs, cl=cl, nv=nv, catch=catch)


def avg_model_fp64(s):
    V, D, k = s["V"], s["D"], s["k"]
    A = sp.csc_matrix((s["nv"].astype(np.float64), s["rows"].astype(np.int64), s["offs"]), shape=(V, D))
    keep = np.flatnonzero(s["cl"] >= 0)
    H = sp.csc_matrix((np.ones(keep.size), (keep, s["cl"][keep])), shape=(D, k))
    S = np.asarray((A @ H).todense())
    with np.errstate(invalid="ignore", divide="ignore"):
        return S / S.sum(axis=0), np.bincount(s["cl"][keep], minlength=k)


def catch_bytes(hp, k):
    """The resident catch model's exact bytes: edge topics (t, t) with primary ratio 1 are 1 * m + 0 * m = m."""
    pairs = np.repeat(np.arange(k, dtype=np.int64), 2).reshape(-1, 2)
    return hp.edge_topics(pairs, primary_ratio=1.0)


def certify(M, M64, sizes):
    empty = sizes == 0
    assert np.array_equal(np.isnan(M).all(axis=0), empty)
    assert not np.isnan(M[:, ~empty]).any()
    m, m64 = M[:, ~empty].astype(np.float64), M64[:, ~empty]
    assert np.array_equal(m == 0, m64 == 0)
    err = np.abs(m - m64)
    worst = float((err / np.where(m64 > 0, m64, 1.0)).max()) if m.size else 0.0
    assert (err <= BOUND * np.abs(m64)).all(), worst
    return worst


@pytest.mark.parametrize("V,D,k,seed", [(1000, 8000, 10, 1), (3001, 12000, 70, 2), (20000, 200000, 200, 3)])
def test_avg_model_certificate(hp, V, D, k, seed):
    s = setup_post(hp, V, D, k, seed)
    before = catch_bytes(hp, k)
    M = hp.avg_topic_model(k)
    M64, sizes = avg_model_fp64(s)
    certify(M, M64, sizes)
    M2 = hp.avg_topic_model(k)
    assert M.tobytes() == M2.tobytes()                              # bitwise reproducible
    assert catch_bytes(hp, k).tobytes() == before.tobytes()         # the catch model is untouched
    assert before.tobytes() == np.asfortranarray(s["catch"]).tobytes()
    np.testing.assert_allclose(M[:, sizes > 0].astype(np.float64).sum(axis=0), 1.0, rtol=1e-5)


def test_avg_model_empty_clusters_are_nan(hp):
    V, D, k = 2000, 6000, 6

    def assign_fn(oc, c):
        a = (c.planted()[oc] % 4).astype(np.uint32)   # topics 0..3 populated, 5 empty
        a[:3] = 4                                     # topic 4: three documents
        return a

    s = setup_post(hp, V, D, k, 5, assign_fn)
    M = hp.avg_topic_model(k)
    M64, sizes = avg_model_fp64(s)
    assert sizes[5] == 0 and sizes[4] == 3
    certify(M, M64, sizes)
    assert np.isnan(M[:, 5]).all() and not np.isnan(M[:, :5]).any()
    d = hp.topic_diversity(k, "avg")
    assert np.isnan(d["dist"][5]) and np.isfinite(d["dist"][:5]).all()
    check_diversity(M, d)


def check_diversity(M, got):
    M = M.astype(np.float64)
    fin = np.isfinite(M).all(axis=0)
    abar = M[:, fin].sum(axis=1) / fin.sum()
    dist = ((M - abar[:, None]) ** 2).sum(axis=0)
    assert np.array_equal(np.isnan(got["dist"]), ~fin)
    np.testing.assert_allclose(got["dist"][fin], dist[fin], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got["avg"], dist[fin].mean(), rtol=1e-10, atol=0)


@pytest.mark.parametrize("V,D,k,seed", [(1000, 8000, 10, 1), (3001, 12000, 70, 2)])
def test_top_words_and_diversity_of_resident_models(hp, V, D, k, seed):
    s = setup_post(hp, V, D, k, seed)
    A = hp.avg_topic_model(k)
    for name, M in (("catch", s["catch"]), ("avg", A)):
        for n in (1, 5, 10, 32):
            ids, w = hp.model_top_words(n, name, with_weights=True)
            ref = top_words(M, n)
            np.testing.assert_array_equal(ids, ref)
            got_w = w.view(np.uint32)
            exp_w = M[ref.astype(np.int64), np.arange(k)[:, None]].view(np.uint32)
            np.testing.assert_array_equal(got_w, exp_w)
        check_diversity(M, hp.topic_diversity(k, name))
    np.testing.assert_array_equal(hp.model_top_words(10, A), top_words(A, 10))   # the same model from the host


def test_top_words_of_host_models(hp):
    rng = np.random.default_rng(7)
    V, k = 777, 67
    M = rng.integers(0, 5, (V, k)).astype(np.float32) / 4     # many ties
    M[:, 3] = 0.0                                             # all zero
    M[:, 4] = np.nan                                          # empty cluster
    M[::3, 5] = np.nan                                        # NaN among weights
    M[:, 6] = -0.0
    M[10, 6] = 0.0
    M[:, 7] = rng.random(V, dtype=np.float32)
    M[500:, 8] = 1.0                                          # ties late in the column
    for n in (1, 2, 10, 31, 32):
        ids, w = hp.model_top_words(n, M, with_weights=True)
        ref = top_words(M, n)
        np.testing.assert_array_equal(ids, ref)
        assert w.view(np.uint32).tobytes() == M[ref.astype(np.int64), np.arange(k)[:, None]].view(np.uint32).tobytes()
    small = rng.integers(0, 3, (20, 9)).astype(np.float32)
    small[:, 2] = np.nan
    np.testing.assert_array_equal(hp.model_top_words(20, small), top_words(small, 20))   # n = V
    big = rng.random((70001, 3), dtype=np.float32)
    big[::7, 1] = 0.5
    np.testing.assert_array_equal(hp.model_top_words(32, big), top_words(big, 32))


def test_argument_errors(hp):
    M = np.ones((20, 3), np.float32)
    for n in (0, 33, 21):
        with pytest.raises(IsleHipError):
            hp.model_top_words(n, M)
    from tools.synth import Corpus
    c = Corpus(500, 2000, 5, 4)
    cnt, rows, offs = c.A()
    hp.upload_counts(500, cnt, rows, offs)                     # a new A: no model of any kind
    for name in ("catch", "avg"):
        with pytest.raises(IsleHipError):
            hp.model_top_words(5, name)
        with pytest.raises(IsleHipError):
            hp.topic_diversity(5, name)
    with pytest.raises(IsleHipError):
        hp.avg_topic_model(5)                                  # before catchwords
    hp.threshold(5)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    hp.find_catchwords(5, max(catchword_rank(2000, 5), 1), assign=(c.planted()[oc] % 5).astype(np.uint32), fetch_thresholds=False)
    with pytest.raises(IsleHipError):
        hp.avg_topic_model(4)                                  # not the catchword pass's num_topics
    with pytest.raises(IsleHipError):
        hp.model_top_words(5, "avg")                           # catchwords alone make no average model
    hp.avg_topic_model(5, fetch=False)
    hp.model_top_words(5, "avg")
    with pytest.raises(IsleHipError):
        hp.topic_diversity(4, "avg")
