"""The heaviest words of edge topics selected on the device from the model's two columns (HotPath.edge_top_words ->
isle_hip_edge_top_words, tw_select_k's edge source in isle_amd/csrc/avg_model.hip): the ids are those hot_path.top_words gives on the
stored edge model and the weights are that model's entries, bit for bit.  Host models use entries that are multiples of 2^-10 and the
ratio 0.75, so that numpy's float32 0.75 m_p + 0.25 m_s is the exact answer whatever the order of rounding."""
import numpy as np
import pytest

from isle_amd import hot_path as H
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu

WG = 256     # tw_select_k's workgroup


def same_floats(got, want):
    np.testing.assert_array_equal(got, want)                                    # NaN == NaN here
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(np.signbit(got)[ok], np.signbit(want)[ok])    # -0 is not +0


@pytest.fixture(scope="module")
def catch_model(hp):
    """The resident catch model of the corpus of test_gpu_post.py, made once."""
    from test_gpu_post import _setup
    V, D, k = 3000, 12000, 10
    s = _setup(hp, V, D, k, 2)
    O = s["O"]
    hp.find_catchwords(k, O.catchword_rank(D, k), assign=s["assign"], fetch_thresholds=False)
    tm = hp.construct_topic_model(k, O.model_rank_threshold(D, k), D, fetch_sums=False)
    pairs = np.array([[0, 1], [1, 0], [3, 3], [0, 1], [9, 4], [2, 7], [7, 2], [5, 5]], np.int64)
    return dict(k=k, V=V, model=tm["model"], pairs=pairs, edge=hp.edge_topics(pairs, 0.7))


@pytest.mark.parametrize("n", [1, 20, 32])
def test_catch_model(hp, catch_model, n):
    pairs, E = catch_model["pairs"], catch_model["edge"]
    ids, w = hp.edge_top_words(pairs, n)                                         # ratio 0.7, the resident catch model
    assert ids.dtype == np.uint32 and ids.shape == (len(pairs), n) and w.dtype == np.float32 and w.shape == ids.shape
    np.testing.assert_array_equal(ids, H.top_words(E, n))
    same_floats(w, E[ids.astype(np.int64), np.arange(len(pairs))[:, None]])
    ids3, w3 = hp.edge_top_words(np.concatenate([pairs, np.full((len(pairs), 1), 5)], axis=1), n)   # (n_edge, 3) as select_edge_pairs returns
    np.testing.assert_array_equal(ids3, ids)
    same_floats(w3, w)
    np.testing.assert_array_equal(hp.model_top_words(min(n, 10)), H.top_words(catch_model["model"], min(n, 10)))


def exact_model(V, cols, seed):
    """Multiples of 2^-10, mostly zero, zeros of both signs; the last column NaN, the one before it nearly empty."""
    g = np.random.default_rng(seed)
    M = (g.integers(-8, 200, (V, cols)) * (g.random((V, cols)) < 0.3)).astype(np.float32) / np.float32(1024)
    M[g.random((V, cols)) < 0.2] = np.float32(-0.0)
    M[:, cols - 2] = 0
    M[V // 2, cols - 2] = np.float32(3 / 1024)
    M[:, cols - 1] = np.nan
    return np.asfortranarray(M)


def exact_edge(M, pairs):
    return (np.float32(0.75) * M[:, pairs[:, 0]] + np.float32(0.25) * M[:, pairs[:, 1]]).astype(np.float32)


def exact_pairs(cols):
    nan, sparse = cols - 1, cols - 2
    return np.array([[0, 1], [1, 0], [2, 2], [sparse, sparse], [sparse, 0], [nan, 0], [0, nan], [nan, nan], [0, 1]], np.int64)


@pytest.mark.parametrize("V,n", [(20, 20), (21, 20), (32, 32), (33, 32), (WG - 1, 20), (WG, 20), (WG + 1, 20), (5 * WG + 3, 1), (5 * WG + 3, 32)])
def test_host_models_with_exact_arithmetic(hp, V, n):
    cols = 6
    M = exact_model(V, cols, V * 100 + n)
    pairs = exact_pairs(cols)
    E = exact_edge(M, pairs)
    ids, w = hp.edge_top_words(pairs, n, primary_ratio=0.75, model=M)
    want = H.top_words(E, n)
    np.testing.assert_array_equal(ids, want)
    same_floats(w, E[want.astype(np.int64), np.arange(len(pairs))[:, None]])
    # the nearly empty column against itself: one non-zero entry, then zero ties (of both signs) decided by id
    assert ids[3, 0] == V // 2 and ids[3, 1:].tolist() == [i for i in range(V) if i != V // 2][:n - 1]
    # a NaN column as primary, as secondary and as both: every entry NaN, ids ascending
    for e in (5, 6, 7):
        assert ids[e].tolist() == list(range(n)) and np.isnan(w[e]).all()
    # isle_hip_model_top_words on the same model gives what it gave before
    np.testing.assert_array_equal(hp.model_top_words(n, model=M), H.top_words(M, n))


def test_signed_zeros(hp):
    V = 40
    M = np.zeros((V, 2), np.float32, order="F")
    M[::2, 0] = -0.0
    M[1::3, 1] = -0.0
    M[7, 0] = M[30, 1] = np.float32(-1 / 1024)
    pairs = np.array([[0, 1], [1, 0], [0, 0]], np.int64)
    E = exact_edge(M, pairs)
    ids, w = hp.edge_top_words(pairs, 32, primary_ratio=0.75, model=M)
    np.testing.assert_array_equal(ids, H.top_words(E, 32))      # +0 and -0 tie: ids ascending, the negative entries last or absent
    same_floats(w, E[ids.astype(np.int64), np.arange(3)[:, None]])


def test_no_edge_topics_and_errors(hp, catch_model):
    k, V = catch_model["k"], catch_model["V"]
    ids, w = hp.edge_top_words(np.zeros((0, 2), np.int64), 5)
    assert ids.shape == (0, 5) and w.shape == (0, 5)
    M = exact_model(50, 4, 1)
    ids, w = hp.edge_top_words(np.zeros((0, 3), np.int64), 5, model=M)
    assert ids.shape == (0, 5)
    for bad in ([[0, k]], [[-1, 0]], [[0, 1], [k + 5, 1]]):
        with pytest.raises(IsleHipError, match="topic id"):
            hp.edge_top_words(np.array(bad, np.int64), 5)
    with pytest.raises(IsleHipError, match="topic id"):
        hp.edge_top_words(np.array([[0, 4]]), 5, model=M)
    for n in (0, 33):
        with pytest.raises(IsleHipError, match="min\\(vocab, 32\\)"):
            hp.edge_top_words(np.array([[0, 1]]), n)
    with pytest.raises(IsleHipError, match="min\\(vocab, 32\\)"):
        hp.edge_top_words(np.array([[0, 1]]), 21, model=exact_model(20, 4, 2))
    ids, _ = hp.edge_top_words(catch_model["pairs"], 3)           # the context is usable after the refusals
    np.testing.assert_array_equal(ids, H.top_words(catch_model["edge"], 3))
