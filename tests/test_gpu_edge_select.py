"""Edge-topic pair selection on the device (HotPath.select_edge_pairs -> isle_hip_select_edge_pairs, isle_amd/csrc/edge_select.hip)
against the statement of the rule, hot_path.select_edge_pairs: the triples, the candidate count and the threshold, all exactly.
Sizes sit at the edges of the kernels: the block of ep_count_k (256) and its capped grid, k^2 either side of 2048 bins and of the
scan's carry at 2^20, counts either side of the radix sort's digits (2^8, 2^16)."""
import numpy as np
import pytest

from isle_amd import hot_path as H
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu

BLOCK = 256                       # ep_count_k's workgroup
FULL_GRID = 256 * 8 * BLOCK       # its grid is capped at 8 workgroups per CU; an MI355X has 256 CUs


def rule(top1, top2, max_edge_topics, min_docs):
    """(triples, candidates, threshold or None) by hot_path.select_edge_pairs."""
    every = H.select_edge_pairs(top1, top2, 1 << 62, min_docs)
    want = H.select_edge_pairs(top1, top2, max_edge_topics, min_docs)
    cut = every.shape[0] > max(int(max_edge_topics), 0)
    return want, every.shape[0], (int(every[max(int(max_edge_topics), 0), 2]) if cut else None)


def check(hp, top1, top2, k, max_edge_topics, min_docs=H.EDGE_TOPIC_MIN_DOCS):
    top1, top2 = np.asarray(top1, np.int32), np.asarray(top2, np.int32)
    want, cand, thr = rule(top1, top2, max_edge_topics, min_docs)
    got, info = hp.select_edge_pairs(max_edge_topics, min_docs, top1=top1, top2=top2, num_topics=k)
    assert got.dtype == np.int64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert info["candidates"] == cand
    assert info["threshold"] == thr
    return got, info


def draw(n, k, seed):
    """Skewed ids with some -1, so that counts tie and some documents have no pair."""
    g = np.random.default_rng(seed)
    t = [np.minimum((k * g.random(n) ** 3).astype(np.int32), k - 1) for _ in range(2)]
    for a in t:
        a[g.random(n) < 0.07] = -1
    return t


def from_counts(pairs_counts, seed=0):
    """Documents, shuffled, with the given number of documents per pair."""
    p = np.repeat(np.array([pc[0] for pc in pairs_counts], np.int32), [pc[2] for pc in pairs_counts])
    s = np.repeat(np.array([pc[1] for pc in pairs_counts], np.int32), [pc[2] for pc in pairs_counts])
    o = np.random.default_rng(seed).permutation(p.size)
    return p[o], s[o]


@pytest.mark.parametrize("n", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, FULL_GRID + 1])
def test_document_counts(hp, n):
    t1, t2 = draw(n, 7, n)
    check(hp, t1, t2, 7, 20)


def test_documents_without_a_pair(hp):
    n = 1000
    none = np.full(n, -1, np.int32)
    t1, _ = draw(n, 5, 1)
    got, info = check(hp, none, none, 5, 10)
    assert got.shape[0] == 0 and info["candidates"] == 0 and info["threshold"] is None
    check(hp, np.abs(t1), none, 5, 10)
    check(hp, none, np.abs(t1), 5, 10)
    half = np.where(np.arange(n) % 2 == 0, -1, np.abs(t1)).astype(np.int32)     # one member of a pair -1
    got, _ = check(hp, np.abs(t1), half, 5, 100)
    assert got[:, 2].sum() == n // 2


@pytest.mark.parametrize("k", [1, 2, 45, 46, 1024, 1025])
def test_bins_at_the_edges_of_the_scan(hp, k):
    t1, t2 = draw(5000, k, k)
    if k >= 1024:   # the first, the last and a middle bin, and bins either side of the scan's carry at 2^20
        extra = [(0, 0, 3), (k - 1, k - 1, 4), (k // 2, k // 3, 5)] + [(b // k, b % k, 6) for b in ((1 << 20) - 1, 1 << 20) if b < k * k]
        e1, e2 = from_counts(extra)
        t1, t2 = np.concatenate([t1, e1]), np.concatenate([t2, e2])
    got, _ = check(hp, t1, t2, k, 1 << 30)
    if k >= 1024:
        have = {(int(p), int(s)) for p, s, _ in got}
        assert {(0, 0), (k - 1, k - 1), (k // 2, k // 3)} <= have
    check(hp, t1, t2, k, 17)


@pytest.mark.parametrize("c", [255, 256, 65535, 65536])
def test_counts_at_the_sort_digit_edges(hp, c):
    """Counts c + 1, c, c - 1 and 1: the largest sort key is c (8, 9, 16, 17 bits), and a 16-bit counter would wrap."""
    t1, t2 = from_counts([(3, 1, c), (0, 2, c + 1), (2, 2, c - 1), (1, 0, 1), (2, 0, c)], seed=c)
    got, _ = check(hp, t1, t2, 4, 10)
    assert got[:, 2].tolist() == [c + 1, c, c, c - 1, 1]
    assert [tuple(x) for x in got[1:3, :2].tolist()] == [(2, 0), (3, 1)]       # equal counts: (primary, secondary) ascending
    check(hp, t1, t2, 4, 2)          # the cut falls between the equal counts


def test_hot_bin(hp):
    t1, t2 = from_counts([(6, 2, 200000), (2, 6, 11), (0, 0, 1)])
    got, _ = check(hp, t1, t2, 9, 5)
    assert got[0].tolist() == [6, 2, 200000]


def test_ties_and_the_cut(hp):
    k = 12
    pairs = [(p, s) for p in range(k) for s in range(k)]
    g = np.random.default_rng(4)
    tied = [pairs[i] for i in g.permutation(len(pairs))[:40]]
    spec = [(p, s, 9) for p, s in tied] + [(11, 11, 30), (0, 0, 20), (5, 5, 2), (7, 1, 1)]
    spec = list({(p, s): (p, s, c) for p, s, c in spec}.values())
    t1, t2 = from_counts(spec, seed=5)
    ncand = len(spec)
    n9 = sum(1 for x in spec if x[2] == 9)
    got, info = check(hp, t1, t2, k, 2 + n9 // 2)           # the cut inside the group of equal counts
    kept = [tuple(x) for x in got[2:, :2].tolist()]
    assert kept == sorted((p, s) for p, s, c in spec if c == 9)[:len(kept)] and info["threshold"] == 9
    for m in (0, ncand - 1, ncand, ncand + 1):
        got, info = check(hp, t1, t2, k, m)
        assert got.shape[0] == min(m, ncand)
        assert (info["threshold"] is None) == (m >= ncand)
    assert check(hp, t1, t2, k, 0)[1]["threshold"] == 30


@pytest.mark.parametrize("min_docs", [1, 2, 31, 10 ** 6])
def test_min_docs(hp, min_docs):
    t1, t2 = from_counts([(1, 2, 30), (2, 1, 2), (0, 0, 1), (3, 3, 1), (2, 2, 2)])
    got, info = check(hp, t1, t2, 4, 3, min_docs)
    assert info["candidates"] == {1: 5, 2: 3, 31: 0, 10 ** 6: 0}[min_docs]


def test_errors(hp):
    import isle_amd
    k = 6
    t1, t2 = draw(3000, k, 9)
    bad = t2.copy()
    bad[1234] = k
    bad[2000] = k + 3
    with pytest.raises(IsleHipError, match="document 1234"):
        hp.select_edge_pairs(10, top1=t1, top2=bad, num_topics=k)
    low = t1.copy()
    low[77] = -2
    with pytest.raises(IsleHipError, match="document 77"):
        hp.select_edge_pairs(10, top1=low, top2=t2, num_topics=k)
    with pytest.raises(IsleHipError, match="8192"):
        hp.select_edge_pairs(10, top1=t1, top2=t2, num_topics=8193)
    with pytest.raises(IsleHipError, match="num_topics"):
        hp.select_edge_pairs(10, top1=t1, top2=t2, num_topics=0)
    with pytest.raises(IsleHipError, match="max_edge_topics"):
        hp.select_edge_pairs(-1, top1=t1, top2=t2, num_topics=k)
    for a, b in ((t1, None), (None, t2)):
        with pytest.raises(IsleHipError, match="null"):
            hp.select_edge_pairs(10, top1=a, top2=b, num_topics=k)
    fresh = isle_amd.HotPath()
    try:
        with pytest.raises(IsleHipError, match="isle_hip_topic_model"):
            fresh.select_edge_pairs(10, num_topics=k)
    finally:
        fresh.close()
    check(hp, t1, t2, k, 10)      # the context is usable after the refusals


def test_resident_pairs_of_the_topic_model(hp):
    """On the corpus of test_gpu_post.py: the selection over the resident top-two topics, nothing fetched for it."""
    from test_gpu_post import _setup
    V, D, k = 3000, 12000, 10
    s = _setup(hp, V, D, k, 2)
    O = s["O"]
    hp.find_catchwords(k, O.catchword_rank(D, k), assign=s["assign"], fetch_thresholds=False)
    tm = hp.construct_topic_model(k, O.model_rank_threshold(D, k), D, fetch_sums=False)
    got, info = hp.select_edge_pairs(25)
    want, cand, thr = rule(tm["top1"], tm["top2"], 25, H.EDGE_TOPIC_MIN_DOCS)
    np.testing.assert_array_equal(got, want)
    assert info == dict(candidates=cand, threshold=thr) and got.shape[0] > 0
    pairs, _ = O.post_edge_topics(tm["model"], tm["top1"], tm["top2"], 25)
    np.testing.assert_array_equal(got[:, :2], np.asarray(pairs)[:, :2])
    with pytest.raises(IsleHipError, match="resident"):
        hp.select_edge_pairs(25, num_topics=k + 1)
