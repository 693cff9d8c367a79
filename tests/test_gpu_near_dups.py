"""isle_hip_doc_signatures / isle_hip_doc_jaccard / isle_hip_doc_near_duplicates / isle_hip_prune_near_docs on the device
(isle_amd/csrc/near_dups.hip) held to the rule of tests/neardup_rule.py with ==, in both forms of the band key: signatures, band keys, the
exact set sizes of the case's pairs, parent, first_of and the three counters; after the prune offsets, rows and count bits of A.  The
cases sit on documents of 0, 1, 63, 64, 65 and 5000 entries under every lane-ownership edge of the signature kernel (H = 1, 63, 64, 65
and 128), on the threshold and the length filter, on groups that alternate three dissimilar word sets, on a chain across bands, on 70 000
copies of one document and on the sort's and the scan's tiles.  A refused call leaves everything as it was; after an accepted prune the
context is the one a fresh upload of the pruned matrix gives."""
import ctypes as C

import numpy as np
import pytest

import neardup_rule as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ndp():
    """a context of this module's own: the key's form is a setting of the context"""
    from isle_amd import HotPath
    h = HotPath(0)
    yield h
    h.close()


def upload(ndp, c, doc_offset=0, docs_global=0):
    ndp.upload_counts(c.V, c.counts, c.rows, c.offs, doc_offset=doc_offset, docs_global=docs_global)


def same_A(ndp, offs, rows, bits):
    cnt, r, o = ndp.get_A()
    return np.array_equal(o, offs) and np.array_equal(r, rows) and np.array_equal(cnt.view(np.uint32), np.asarray(bits).view(np.uint32))


@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("case", nr.CASES, ids=lambda c: c.name)
def test_every_call_equals_the_rule(ndp, case, form):
    want = nr.rule(case, form, doc_offset=11)
    D = case.offs.size - 1
    th = (case.num, case.den)
    ndp.neardup_key_form(form)
    try:
        upload(ndp, case, doc_offset=11, docs_global=D + 30)
        got = ndp.doc_signatures(case.bands, case.rows_per_band)
        assert got["sig"].dtype == np.uint64 and np.array_equal(got["sig"], want["sig"])
        assert got["keys"].shape == (case.bands, D) and np.array_equal(got["keys"], want["keys"])
        assert np.array_equal(ndp.doc_signatures(case.bands, case.rows_per_band, sig=False)["keys"], want["keys"])     # the prune's path: keys alone
        inter, uni = ndp.doc_jaccard(case.pairs[:, 0], case.pairs[:, 1])
        assert np.array_equal(inter, want["inter"]) and np.array_equal(uni, want["uni"])
        nd = ndp.near_duplicates(th, case.bands, case.rows_per_band)
        assert np.array_equal(nd["parent"], want["parent"]) and np.array_equal(nd["first_of"], want["first_of"])
        assert (nd["n_dropped"], nd["pairs_tested"], nd["rounds"]) == (want["n_dropped"], want["pairs_tested"], want["rounds"])
        assert (nd["num"], nd["den"]) == th
        assert same_A(ndp, case.offs, case.rows, case.counts)                          # none of the three changes anything resident
        assert ndp.a_doc_offset == 11 and ndp._counts_shape() == (case.V, D, case.rows.size, 11, D + 30)
        pr = ndp.prune_near_docs(th, case.bands, case.rows_per_band)
        assert pr["docs"] == want["docs"] and pr["nnz"] == want["nnz"] and pr["docs_global"] == want["docs"] and pr["n_dropped"] == want["n_dropped"]
        assert np.array_equal(pr["kept_docs"], want["kept_docs"]) and pr["kept_docs"].dtype == np.uint32
        assert np.array_equal(pr["parent"], want["parent"]) and np.array_equal(pr["first_of"], want["first_of"])
        assert same_A(ndp, want["offs"], want["rows"], want["counts"])
        assert ndp._counts_shape() == (case.V, want["docs"], want["nnz"], 0, want["docs"])     # one rank: its documents are the corpus
        words, _ = ndp.doc_lengths()                                                   # the pruned matrix's own lengths: the kept documents'
        assert np.array_equal(words, np.diff(case.offs)[want["keep"]])
    finally:
        ndp.neardup_key_form("auto")


@pytest.mark.parametrize("name", ["equal_sets_1x1", "equal_sets_13x5", "equal_sets_pool"])
def test_num_equal_den_gives_the_same_first_of_in_both_forms(ndp, name):
    case = nr.BY_NAME[name]
    upload(ndp, case)
    got = {}
    try:
        for form in nr.FORMS:
            ndp.neardup_key_form(form)
            got[form] = ndp.near_duplicates((case.num, case.den), case.bands, case.rows_per_band)["first_of"]
    finally:
        ndp.neardup_key_form("auto")
    assert np.array_equal(got["full"], got["narrow"]) and np.array_equal(got["full"], nr.rule(case, "full")["first_of"])


def test_a_float_threshold_becomes_a_fraction(ndp):
    case = nr.BY_NAME["lengths_16x4"]
    upload(ndp, case)
    got = ndp.near_duplicates()                                                        # 0.8, 16 x 4
    assert (got["num"], got["den"]) == (4, 5) and np.array_equal(got["first_of"], nr.rule(case, "full")["first_of"])
    assert ndp.near_duplicates(0.333)["den"] == 1000 and ndp.near_duplicates(1.0)["num"] == 1


def test_refused_calls_leave_everything_as_it_was(ndp):
    from isle_amd import IsleHipError
    case = nr.BY_NAME["lengths_16x4"]
    D = case.offs.size - 1
    upload(ndp, case, doc_offset=7, docs_global=D + 9)
    bad = [((0, 5), 16, 4), ((6, 5), 16, 4), ((1, 65536), 16, 4), ((4, 5), 0, 4), ((4, 5), 65, 1), ((4, 5), 16, 0), ((4, 5), 16, 9), ((4, 5), 17, 8)]
    for th, bands, rpb in bad:
        for call, who in ((ndp.near_duplicates, "doc_near_duplicates"), (ndp.prune_near_docs, "prune_near_docs")):
            with pytest.raises(IsleHipError) as e:
                call(th, bands, rpb)
            assert str(e.value) == "isle_hip error -1: " + nr.check_args(who, True, th[0], th[1], bands, rpb) and nr.check_args(who, True, th[0], th[1], bands, rpb)
    for bands, rpb in ((0, 4), (65, 1), (16, 9), (17, 8)):
        with pytest.raises(IsleHipError) as e:
            ndp.doc_signatures(bands, rpb)
        assert str(e.value) == "isle_hip error -1: " + nr.check_args("doc_signatures", True, 1, 1, bands, rpb)
    for a, b, at in (([0, D], [0, 0], 1), ([0, 1, 2], [1, 2, D + 5], 2), ([0xFFFFFFFF], [0], 0)):
        with pytest.raises(IsleHipError) as e:
            ndp.doc_jaccard(a, b)
        assert str(e.value) == "isle_hip error -1: " + nr.bad_pair(at, a[at], b[at], D)
    with pytest.raises(IsleHipError, match="unknown form"):
        ndp._chk(ndp._lib.isle_hip_neardup_key_form(ndp._h, 3))
    assert same_A(ndp, case.offs, case.rows, case.counts)
    assert ndp.a_doc_offset == 7 and ndp._counts_shape() == (case.V, D, case.rows.size, 7, D + 9)
    inter, uni = ndp.doc_jaccard([], [])                                               # no pair: nothing to do
    assert inter.size == 0 and uni.size == 0


def test_no_count_matrix_is_refused_by_name():
    from isle_amd import HotPath, IsleHipError
    h = HotPath(0)
    one = np.zeros(1, np.uint32)
    p = one.ctypes.data_as(C.c_void_p)
    try:
        for call, who in ((lambda: h._lib.isle_hip_doc_signatures(h._h, 16, 4, None, None), "doc_signatures"),
                          (lambda: h._lib.isle_hip_doc_jaccard(h._h, 1, p, p, None, None), "doc_jaccard"),
                          (lambda: h._lib.isle_hip_doc_near_duplicates(h._h, 4, 5, 16, 4, None, None, None, None, None), "doc_near_duplicates"),
                          (lambda: h._lib.isle_hip_prune_near_docs(h._h, 4, 5, 16, 4, None, None, None, None, None, None, None), "prune_near_docs")):
            with pytest.raises(IsleHipError) as e:
                h._chk(call())
            assert str(e.value) == "isle_hip error -1: %s: no count matrix" % who
    finally:
        h.close()


@pytest.fixture(scope="module")
def corpus():
    """a synthetic corpus with a tenth of its documents planted as near copies of earlier ones (one word in twenty replaced)"""
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    c = Corpus(V, D, k, seed=6)
    cnt, rows, offs = c.A()
    cnt, rows, offs = np.asarray(cnt, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    rng = np.random.default_rng(2)
    docs = [(rows[offs[d]:offs[d + 1]].astype(np.int64), cnt[offs[d]:offs[d + 1]]) for d in range(D)]
    for d in rng.choice(np.arange(100, D), size=D // 10, replace=False):
        w, x = docs[int(rng.integers(0, d))]
        keep = rng.random(w.size) >= 0.05
        docs[d] = (w[keep], x[keep])
    o2, r2, c2 = nr.dr.csc(V, docs)
    return nr.Case("synth", V, o2, r2, c2, 4, 5, 16, 4, np.zeros((0, 2), np.uint32), "pipeline"), k


def test_after_a_prune_the_context_is_a_fresh_upload_of_the_pruned_matrix(ndp, corpus):
    from isle_amd import HotPath, IsleHipError
    from isle_amd.hot_path import catchword_rank, model_rank_threshold
    case, k = corpus
    want = nr.rule(case, "full")
    D = case.offs.size - 1
    assert 200 < want["n_dropped"] < D // 2
    # a whole downstream stage on the unpruned A first: the prune has to void it
    upload(ndp, case)
    ndp.threshold(k)
    Dk = ndp.shape()[1]
    ndp.find_catchwords(k, catchword_rank(D, k), assign=(np.arange(Dk) % k).astype(np.uint32), fetch_thresholds=False)
    ndp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
    got = ndp.prune_near_docs((4, 5))
    assert np.array_equal(got["kept_docs"], want["kept_docs"]) and same_A(ndp, want["offs"], want["rows"], want["counts"])
    with pytest.raises(IsleHipError, match="isle_hip_catchwords"):      # as after any new A: no topic model without a new catchword pass
        ndp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
    fresh = HotPath(0)
    try:
        fresh.upload_counts(case.V, want["counts"].view(np.float32), want["rows"], want["offs"])
        assert ndp._counts_shape() == fresh._counts_shape() and ndp.avg_doc_sz() == fresh.avg_doc_sz()
        wa, ta = ndp.doc_lengths()
        wb, tb = fresh.doc_lengths()
        assert np.array_equal(wa, wb) and np.array_equal(ta, tb)
        assert ndp.threshold(k) == fresh.threshold(k) and ndp.shape() == fresh.shape()
        Ba, Bb = ndp.get_B(), fresh.get_B()
        for f in ("vals", "rows", "offs", "original_cols", "zetas"):
            assert np.array_equal(np.asarray(Ba[f]).view(np.uint8), np.asarray(Bb[f]).view(np.uint8)), f
    finally:
        fresh.close()
