"""tests/feed_rule.py against tests/ingest_rule.py: the same triples, without zero counts (which tdf refuses), printed as tdf text and
taken through the byte-level rule of tdf ingest give the same matrix, bit for bit.  Also what the feed tests rely on in the base corpus."""
import numpy as np
import pytest

from feed_rule import BASE_D, BASE_V, base_corpus, feed_rule
from ingest_rule import ingest_rule, text_from_entries


def _nonzero(t):
    d, w, c = t
    keep = c != 0
    return d[keep], w[keep], c[keep]


def _edges(V, D, seed):
    rng = np.random.default_rng(seed)
    n = 200
    d = rng.integers(0, D, n)
    w = rng.integers(0, V, n)
    d[:4] = [0, D - 1, 0, D - 1]
    w[:4] = [0, V - 1, V - 1, 0]
    d[4:8], w[4:8] = d[:4], w[:4]                                  # repeated pairs, other counts
    return d, w, rng.integers(1, 1000, n)


CASES = {
    "base": lambda: _nonzero(base_corpus()) + (BASE_V, BASE_D),
    "V1": lambda: (np.array([3, 0, 3, 9]), np.zeros(4, np.int64), np.array([5, 6, 7, 8]), 1, 10),
    "D1": lambda: (np.zeros(5, np.int64), np.array([4, 0, 49, 4, 7]), np.array([1, 2, 3, 4, 5]), 50, 1),
    "V257-D65537": lambda: _edges(257, 65537, 1) + (257, 65537),
    "V256-D255": lambda: _edges(256, 255, 2) + (256, 255),
    "empty-documents": lambda: (np.array([7, 5, 22, 20, 7]), np.array([1, 2, 3, 4, 1]), np.array([9, 8, 7, 6, 5]), 6, 40),
    "largest-count": lambda: (np.array([1, 1]), np.array([2, 2]), np.array([4294967295, 3], np.uint64), 5, 3),
    "no-entries": lambda: (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 4, 6),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_feed_rule_equals_the_tdf_rule_on_the_same_triples(name):
    d, w, c, V, D = CASES[name]()
    d, w, c = np.asarray(d, np.uint64), np.asarray(w, np.uint64), np.asarray(c, np.uint64)
    text = text_from_entries(d + np.uint64(1), w + np.uint64(1), c) if len(d) else b""
    status, counts, rows, offs, entries_read = ingest_rule(text, V, D)
    assert status == "ok" and entries_read == len(d)
    gc, gr, go = feed_rule(d, w, c, D)
    assert gc.dtype == np.float32 and gr.dtype == np.uint32 and go.dtype == np.int64 and len(go) == D + 1
    np.testing.assert_array_equal(go, offs)
    np.testing.assert_array_equal(gr, rows)
    np.testing.assert_array_equal(gc.view(np.uint32), counts.view(np.uint32))


def test_zero_counts_take_no_part_and_the_first_offered_wins():
    d, w, c = [2, 2, 2, 0], [1, 1, 1, 3], [0, 7, 9, 0]
    counts, rows, offs = feed_rule(d, w, c, 3)
    assert counts.tolist() == [7.0] and rows.tolist() == [1] and offs.tolist() == [0, 0, 0, 1]
    assert feed_rule([1], [0], [4294967295], 2)[0][0] == np.float32(4294967296.0)


def test_the_base_corpus_shows_what_the_feed_tests_need():
    d, w, c = base_corpus()
    assert 5900 <= len(d) <= 6100 and int(d.max()) < BASE_D and int(w.max()) < BASE_V
    key = d.astype(np.int64) * BASE_V + w
    nz = c != 0
    uniq, first_at, n_of = np.unique(key[nz], return_index=True, return_counts=True)
    rep = uniq[n_of > 1]
    assert 0.04 * len(d) <= len(rep) <= 0.06 * len(d)
    for k in rep[:50]:                                            # the repeats carry different counts: "first wins" is observable
        assert len(set(c[nz][key[nz] == k].tolist())) > 1
    assert 0.015 * len(d) <= int((~nz).sum()) <= 0.03 * len(d)
    zero_first = [k for k in np.unique(key[~nz]) if nz[key == k].any() and not nz[np.flatnonzero(key == k)[0]]]
    assert len(zero_first) >= 20                                  # a zero count ahead of the pair's non-zero entry
    counts, rows, offs = feed_rule(d, w, c, BASE_D)
    assert len(counts) == len(uniq) == 5600 and (counts > 0).all()
