"""isle_hip_word_doc_freq / isle_hip_prune_vocab on the device (isle_amd/csrc/vocab.hip) held to the rule of tests/vocab_rule.py bit for bit:
A goes up with upload_counts and comes back with get_A; df, kept_words, the counts (compared as their 32 bits), rows and offsets are
compared with ==.  The cases sit on the scan's tile edges (nnz = 0 with documents, 4095, 4096, 4097, 2 x 4096 + 1), on the edges of the LDS
parts of the document-frequency kernel in both of its forms, on a head word in every one of 70 000 documents (a 16-bit counter anywhere
would wrap) and on the documents a compaction can get wrong: empty ones at both ends and in a long run, documents that lose all, the first
or the last of their entries, one document holding the whole vocabulary.  A refused prune leaves everything as it was; after an accepted
one the context is the one a fresh upload of the pruned matrix gives."""
import numpy as np
import pytest

import vocab_rule as vr

pytestmark = pytest.mark.gpu
FORMS = ("lds", "global")


@pytest.fixture(scope="module")
def vp():
    """a context of this module's own: the histogram's form is a setting of the context"""
    from isle_amd import HotPath
    h = HotPath(0)
    yield h
    h.close()


def upload(hp, c):
    hp.upload_counts(c.V, c.counts, c.rows, c.offs)


def prune(hp, c):
    return hp.prune_vocab(min_df=c.min_df, max_df=c.max_df or None, keep_n=c.keep_n or None)


def same_A(hp, offs, rows, bits):
    cnt, r, o = hp.get_A()
    return np.array_equal(o, offs) and np.array_equal(r, rows) and np.array_equal(cnt.view(np.uint32), np.asarray(bits).view(np.uint32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", vr.DEVICE, ids=lambda c: c.name)
def test_prune_equals_the_rule_bit_for_bit(vp, case, form):
    from isle_amd import IsleHipError
    want = vr.rule(case)
    vp.vocab_hist_form(form)
    try:
        upload(vp, case)
        assert np.array_equal(vp.word_doc_freq(), want["df"])
        assert same_A(vp, case.offs, case.rows, case.counts)              # word_doc_freq changes nothing resident
        if want["text"]:
            with pytest.raises(IsleHipError) as e:
                prune(vp, case)
            assert "isle_hip error -1: " + want["text"] == str(e.value)
            assert same_A(vp, case.offs, case.rows, case.counts)          # a refused call leaves A as it was
            return
        got = prune(vp, case)
        assert np.array_equal(got["df"], want["df"]) and got["df"].dtype == np.uint32
        assert np.array_equal(got["kept_words"], want["kept_words"]) and got["vocab"] == want["vocab"]
        assert got["nnz"] == want["nnz"] and got["docs_emptied"] == want["docs_emptied"]
        assert same_A(vp, want["offs"], want["rows"], want["counts"])
        if case.aim == "identity":
            assert same_A(vp, case.offs, case.rows, case.counts)
        # the pruned matrix's own frequencies: the kept words', in the new numbering
        assert np.array_equal(vp.word_doc_freq(), want["df"][want["kept_words"]])
    finally:
        vp.vocab_hist_form("auto")


def test_the_float_max_df_is_a_share_of_the_corpus(vp):
    c = vr.BY_NAME["counts"]
    D = c.offs.size - 1
    upload(vp, c)
    got = vp.prune_vocab(min_df=2, max_df=0.25)
    want = vr.rule(c._replace(min_df=2, max_df=int(np.floor(0.25 * D)), keep_n=0))
    assert np.array_equal(got["kept_words"], want["kept_words"]) and same_A(vp, want["offs"], want["rows"], want["counts"])
    with pytest.raises(ValueError):
        vp.prune_vocab(max_df=1.5)


def test_no_count_matrix_is_refused():
    from isle_amd import HotPath, IsleHipError
    h = HotPath(0)
    try:
        with pytest.raises(IsleHipError, match="no count matrix"):
            h.word_doc_freq()
        with pytest.raises(IsleHipError, match="no count matrix"):
            h.prune_vocab()
    finally:
        h.close()


@pytest.fixture(scope="module")
def corpus():
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    c = Corpus(V, D, k, seed=6)
    cnt, rows, offs = c.A()
    return vr.Case("synth", V, np.asarray(offs, np.int64), np.asarray(rows, np.uint32), np.asarray(cnt, np.float32), 5, D // 2, 1000, "pipeline", True), k, c


def test_a_refused_prune_leaves_everything_as_it_was(vp, corpus):
    from isle_amd import IsleHipError
    case, k, _ = corpus
    upload(vp, case)
    vp.threshold(k)
    shape, B, avg = vp.shape(), vp.get_B(), vp.avg_doc_sz()
    with pytest.raises(IsleHipError, match="no word kept"):
        vp.prune_vocab(min_df=case.offs.size - 1, max_df=case.offs.size - 1)
    assert vp.shape() == shape and vp.avg_doc_sz() == avg and same_A(vp, case.offs, case.rows, case.counts)
    B2 = vp.get_B()
    assert all(np.array_equal(np.asarray(B[f]).view(np.uint8), np.asarray(B2[f]).view(np.uint8)) for f in ("vals", "rows", "offs", "original_cols", "zetas"))


def test_after_a_prune_the_context_is_a_fresh_upload_of_the_pruned_matrix(vp, corpus):
    from isle_amd import HotPath, IsleHipError
    from isle_amd.hot_path import catchword_rank, model_rank_threshold
    case, k, synth = corpus
    want = vr.rule(case)
    assert 0 < want["vocab"] < case.V and want["nnz"] < case.rows.size
    D = case.offs.size - 1
    # a whole downstream stage on the unpruned A first: the prune has to void it
    upload(vp, case)
    vp.threshold(k)
    oc = vp.get_B()["original_cols"].astype(np.int64)
    vp.find_catchwords(k, catchword_rank(D, k), assign=synth.planted()[oc].astype(np.uint32), fetch_thresholds=False)
    vp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
    got = prune(vp, case)
    assert np.array_equal(got["kept_words"], want["kept_words"]) and same_A(vp, want["offs"], want["rows"], want["counts"])
    with pytest.raises(IsleHipError, match="isle_hip_catchwords"):      # as after any new A: no topic model without a new catchword pass
        vp.construct_topic_model(k, model_rank_threshold(D, k), D, fetch_sums=False)
    fresh = HotPath(0)
    try:
        fresh.upload_counts(want["vocab"], want["counts"].view(np.float32), want["rows"], want["offs"])
        assert vp.avg_doc_sz() == fresh.avg_doc_sz()
        assert np.array_equal(vp.log_combinatorial().view(np.uint32), fresh.log_combinatorial().view(np.uint32))
        ta, tb = vp.threshold(k), fresh.threshold(k)
        assert ta == tb and vp.shape() == fresh.shape() and vp.shape()[0] == want["vocab"]
        Ba, Bb = vp.get_B(), fresh.get_B()
        for f in ("vals", "rows", "offs", "original_cols", "zetas"):
            assert np.array_equal(np.asarray(Ba[f]).view(np.uint8), np.asarray(Bb[f]).view(np.uint8)), f
    finally:
        fresh.close()
