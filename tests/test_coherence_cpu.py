"""The top_words helper (isle_amd.hot_path.top_words): the trainer's rule — heaviest first, the lower word id first among equal weights —
on a V x k topic model and on an edge model, as a 2-D array or as the flat column-major buffer the C++ getters write."""
import numpy as np
import pytest

from isle_amd.hot_path import top_words


def rule(col, n):
    return sorted(range(col.shape[0]), key=lambda w: (-col[w], w))[:n]


def test_ties_go_to_the_lower_word_id():
    m = np.array([[0.1, 0.0],
                  [0.3, 0.0],
                  [0.3, 0.5],
                  [0.0, 0.5],
                  [0.3, 0.0]], np.float32)
    np.testing.assert_array_equal(top_words(m, 3), [[1, 2, 4], [2, 3, 0]])
    np.testing.assert_array_equal(top_words(m, 5), [[1, 2, 4, 0, 3], [2, 3, 0, 1, 4]])
    assert top_words(m, 9).shape == (2, 5)          # at most V words
    assert top_words(m, 3).dtype == np.uint32


def test_random_models_with_many_ties_match_the_rule():
    rng = np.random.default_rng(0)
    V, k = 300, 7
    m = (rng.integers(0, 6, size=(V, k)) / 5.0).astype(np.float32)   # few distinct weights: ties everywhere
    m[:, 3] = 0.0                                                    # an all-zero topic
    got = top_words(m, 10)
    for t in range(k):
        assert list(got[t]) == rule(m[:, t].astype(np.float64), 10)


def test_nan_topic_sorts_last():
    m = np.full((6, 2), np.nan, np.float32)
    m[:, 1] = [0, 1, 2, 3, 4, 5]
    m[2, 1] = np.nan
    np.testing.assert_array_equal(top_words(m, 3), [[0, 1, 2], [5, 4, 3]])


def test_edge_model_shapes():
    """An edge model is V x n_edge column-major (isle_hip_edge_topics, get_edge_model): 2-D in any memory order, or flat with vocab_size."""
    rng = np.random.default_rng(1)
    V, n = 50, 9
    E = np.asfortranarray(rng.random((V, n)).astype(np.float32))
    ref = np.array([rule(E[:, e].astype(np.float64), 5) for e in range(n)], np.uint32)
    np.testing.assert_array_equal(top_words(E, 5), ref)
    np.testing.assert_array_equal(top_words(np.ascontiguousarray(E), 5), ref)
    np.testing.assert_array_equal(top_words(E.ravel(order="F"), 5, vocab_size=V), ref)
    with pytest.raises(ValueError):
        top_words(E.ravel(order="F"), 5)
