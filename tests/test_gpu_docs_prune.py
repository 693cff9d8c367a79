"""isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs on the device (isle_amd/csrc/docs.hip) held to the rule of
tests/docs_rule.py bit for bit, in both forms of the document hash: A goes up with upload_counts and comes back with get_A; lengths,
first_of, kept_docs, the counts (compared as their 32 bits), rows and offsets are compared with ==.  The narrow form cuts the hash to two
bits, so every run of equal keys holds many unequal documents and equality of content alone decides; one case alternates three contents
within every run, so that several rounds are needed and the third X must find the first.  The other cases sit on the sort's and the scan's
tiles, on documents of 63, 64, 65 and 5000 entries, on empty documents at both ends and in a run of 2000, and on 70 000 copies of one
document.  A refused prune leaves everything as it was; after an accepted one the context is the one a fresh upload of the pruned matrix
gives."""
import ctypes as C

import numpy as np
import pytest

import docs_rule as dr
import vocab_rule as vr

pytestmark = pytest.mark.gpu
FORMS = ("full", "narrow")


@pytest.fixture(scope="module")
def dp():
    """a context of this module's own: the hash's form is a setting of the context"""
    from isle_amd import HotPath
    h = HotPath(0)
    yield h
    h.close()


def upload(hp, c, doc_offset=0, docs_global=0):
    hp.upload_counts(c.V, c.counts, c.rows, c.offs, doc_offset=doc_offset, docs_global=docs_global)


def prune(hp, c):
    return hp.prune_docs(min_words=c.min_words, max_words=c.max_words or None, min_tokens=c.min_tokens, max_tokens=c.max_tokens or None, drop_duplicates=bool(c.dups))


def same_A(hp, offs, rows, bits):
    cnt, r, o = hp.get_A()
    return np.array_equal(o, offs) and np.array_equal(r, rows) and np.array_equal(cnt.view(np.uint32), np.asarray(bits).view(np.uint32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", dr.CASES, ids=lambda c: c.name)
def test_prune_equals_the_rule_bit_for_bit(dp, case, form):
    from isle_amd import IsleHipError
    want = dr.rule(case, doc_offset=11)
    D = case.offs.size - 1
    dp.doc_hash_form(form)
    try:
        upload(dp, case, doc_offset=11, docs_global=D + 30)
        words, tokens = dp.doc_lengths()
        assert words.dtype == np.uint32 and tokens.dtype == np.uint64
        assert np.array_equal(words, want["words"]) and np.array_equal(tokens, want["tokens"])
        dup = dp.doc_duplicates()
        assert np.array_equal(dup["first_of"], want["all_first_of"]) and dup["n_duplicates"] == want["n_duplicates"]
        assert same_A(dp, case.offs, case.rows, case.counts)              # neither changes anything resident
        if want["text"]:
            with pytest.raises(IsleHipError) as e:
                prune(dp, case)
            assert "isle_hip error -1: " + want["text"] == str(e.value)
            assert same_A(dp, case.offs, case.rows, case.counts)          # a refused call leaves A as it was
            assert dp.a_doc_offset == 11 and dp._counts_shape()[4] == D + 30
            return
        got = prune(dp, case)
        assert got["docs"] == want["docs"] and got["nnz"] == want["nnz"] and got["docs_global"] == want["docs_global"]
        assert np.array_equal(got["kept_docs"], want["kept_docs"]) and got["kept_docs"].dtype == np.uint32
        assert np.array_equal(got["first_of"], want["first_of"])
        assert [got["dropped_short"], got["dropped_long"], got["dropped_duplicate"]] == want["dropped"]
        assert same_A(dp, want["offs"], want["rows"], want["counts"])
        assert dp._counts_shape() == (case.V, want["docs"], want["nnz"], 0, want["docs"])   # one rank: its documents are the corpus
        if case.aim == "identity":
            assert same_A(dp, case.offs, case.rows, case.counts) and np.array_equal(got["kept_docs"], 11 + np.arange(D))
        # the pruned matrix's own lengths: the kept documents'
        w2, t2 = dp.doc_lengths()
        assert np.array_equal(w2, want["words"][want["keep"]]) and np.array_equal(t2, want["tokens"][want["keep"]])
        if case.dups:
            assert dp.doc_duplicates()["n_duplicates"] == 0
    finally:
        dp.doc_hash_form("auto")


def test_arguments_refused_before_anything_runs(dp):
    from isle_amd import IsleHipError
    c = dr.BY_NAME["equality"]
    upload(dp, c)
    with pytest.raises(ValueError):
        dp.prune_docs(min_words=-1)
    with pytest.raises(ValueError):
        dp.prune_docs(max_tokens=0)
    nd = C.c_uint64()
    rc = dp._lib.isle_hip_prune_docs(dp._h, 0, 0, 0, 0, 2, C.byref(nd), None, None, None, None, None)    # drop_duplicates outside {0, 1}
    assert rc == -1 and dp._lib.isle_hip_last_error(dp._h).decode() == dr.check_args(0, 0, 0, 0, 2)
    with pytest.raises(IsleHipError, match="unknown form"):
        dp._chk(dp._lib.isle_hip_doc_hash_form(dp._h, 3))
    assert same_A(dp, c.offs, c.rows, c.counts)


def test_no_count_matrix_is_refused():
    from isle_amd import HotPath, IsleHipError
    h = HotPath(0)
    try:
        for call, who in ((lambda: h._chk(h._lib.isle_hip_doc_lengths(h._h, None, None)), "doc_lengths"),
                          (lambda: h._chk(h._lib.isle_hip_doc_duplicates(h._h, None, None)), "doc_duplicates"),
                          (lambda: h._chk(h._lib.isle_hip_prune_docs(h._h, 1, 0, 0, 0, 0, None, None, None, None, None, None)), "prune_docs")):
            with pytest.raises(IsleHipError) as e:
                call()
            assert str(e.value) == "isle_hip error -1: %s: no count matrix" % who
    finally:
        h.close()


@pytest.fixture(scope="module")
def corpus():
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    c = Corpus(V, D, k, seed=6)
    cnt, rows, offs = c.A()
    cnt, rows, offs = np.asarray(cnt, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    words, tokens = dr.lengths(offs, cnt)
    lo, hi = int(np.percentile(words, 10)), int(np.percentile(tokens, 90))
    return dr.Case("synth", V, offs, rows, cnt, lo, 0, 0, hi, 1, "pipeline"), k, c


def test_a_refused_prune_leaves_everything_as_it_was(dp, corpus):
    from isle_amd import IsleHipError
    case, k, _ = corpus
    upload(dp, case)
    dp.threshold(k)
    shape, B, avg = dp.shape(), dp.get_B(), dp.avg_doc_sz()
    with pytest.raises(IsleHipError, match="no document kept"):
        dp.prune_docs(min_words=case.V + 1, drop_duplicates=True)
    with pytest.raises(IsleHipError, match="min_tokens = 9 > max_tokens = 8"):
        dp.prune_docs(min_tokens=9, max_tokens=8)
    assert dp.shape() == shape and dp.avg_doc_sz() == avg and same_A(dp, case.offs, case.rows, case.counts)
    B2 = dp.get_B()
    assert all(np.array_equal(np.asarray(B[f]).view(np.uint8), np.asarray(B2[f]).view(np.uint8)) for f in ("vals", "rows", "offs", "original_cols", "zetas"))


def test_after_a_prune_the_context_is_a_fresh_upload_of_the_pruned_matrix(dp, corpus):
    from isle_amd import HotPath, IsleHipError
    from isle_amd.hot_path import catchword_rank, model_rank_threshold
    case, k, synth = corpus
    want = dr.rule(case)
    assert 0 < want["docs"] < case.offs.size - 1 and want["dropped"][0] > 0 and want["dropped"][1] > 0
    D = case.offs.size - 1
    # a whole downstream stage on the unpruned A first: the prune has to void it
    upload(dp, case)
    dp.threshold(k)
    oc = dp.get_B()["original_cols"].astype(np.int64)
    dp.find_catchwords(k, catchword_rank(D, k), assign=synth.planted()[oc].astype(np.uint32), fetch_thresholds=False)
    dp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
    got = prune(dp, case)
    assert np.array_equal(got["kept_docs"], want["kept_docs"]) and same_A(dp, want["offs"], want["rows"], want["counts"])
    with pytest.raises(IsleHipError, match="isle_hip_catchwords"):      # as after any new A: no topic model without a new catchword pass
        dp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
    fresh = HotPath(0)
    try:
        fresh.upload_counts(case.V, want["counts"].view(np.float32), want["rows"], want["offs"])
        assert dp.avg_doc_sz() == fresh.avg_doc_sz()
        assert np.array_equal(dp.log_combinatorial().view(np.uint32), fresh.log_combinatorial().view(np.uint32))
        ta, tb = dp.threshold(k), fresh.threshold(k)
        assert ta == tb and dp.shape() == fresh.shape() and dp.shape()[1] <= want["docs"]
        Ba, Bb = dp.get_B(), fresh.get_B()
        for f in ("vals", "rows", "offs", "original_cols", "zetas"):
            assert np.array_equal(np.asarray(Ba[f]).view(np.uint8), np.asarray(Bb[f]).view(np.uint8)), f
    finally:
        fresh.close()


def test_prune_docs_removes_what_prune_vocab_emptied(dp):
    c = vr.BY_NAME["documents_lose"]
    dp.upload_counts(c.V, c.counts, c.rows, c.offs)
    empty_before = int((np.diff(c.offs) == 0).sum())
    emptied = dp.prune_vocab(min_df=c.min_df)["docs_emptied"]
    assert emptied > 0 and empty_before > 0
    _, _, offs = dp.get_A()
    got = dp.prune_docs(min_words=1)
    assert got["dropped_short"] == emptied + empty_before and got["dropped_long"] == 0 and got["dropped_duplicate"] == 0
    assert np.array_equal(got["kept_docs"], np.flatnonzero(np.diff(offs) > 0)) and got["docs"] == c.offs.size - 1 - emptied - empty_before
    w, _ = dp.doc_lengths()
    assert (w > 0).all()
