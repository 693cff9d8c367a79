"""coherence.hip, corpus_stats.hip and avg_model.hip at their kernel edges against the plain references of tests/diag_cases.py: hit-list
and tile edges of the document frequencies, the LDS / HBM table switch of the log-combinatorial, lanes, ties and block cuts of the top-five
sets, the exact accumulator of the average model (bit for bit where every column total is below 2^53, the derived bound beyond), top-word
selection at empty wave ranges, ties and special values, and diversity inside its derived bound.  test_diag_cases_cpu.py asserts, without
a GPU, that every input here reaches the edge it was built for and would fail under the wrong rule.

Every case runs twice and must return the same bytes.  At the end of the module the error / bound ratios are printed
(profiles/diag_certificate.md holds a measured run); DIAG_CERT_REPORT=<path> writes them as JSON."""
import json
import os
import time

import numpy as np
import pytest

import diag_cases as dc
import stages_certificate as sc
from diag_cases import F, build
from isle_amd import IsleHipError
from isle_amd.hot_path import top_words
from test_corpus_stats_cpu import literal

pytestmark = pytest.mark.gpu

COH_CASES = dc.coherence_cases()
LC_CASES = dc.log_comb_cases()
T5_CASES = dc.top_five_cases()
TW_CASES = dc.top_words_cases()
STATS = {}
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def certificate_summary():
    yield STATS
    wall = time.time() - _T0
    for name, s in sorted(STATS.items()):
        print("diag certificate, %s: %s" % (name, ", ".join("%s %.3g" % kv if isinstance(kv[1], float) else "%s %s" % kv for kv in sorted(s.items()))))
    print("diag certificate: %.1f s" % wall)
    path = os.environ.get("DIAG_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(STATS, wall_seconds=wall), f, indent=1, sort_keys=True)


def _upload(hp, case):
    hp.upload_counts(case["V"], case["cnt"], case["rows"], case["offs"])


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _usable(hp):
    """The context still answers after a refusal."""
    case = dc.lc_case("wave-sum")
    _upload(hp, case)
    assert np.array_equal(_bits(hp.log_combinatorial()), _bits(dc.log_comb_reference(case)))


# ---- coherence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COH_CASES))
def test_coherence_case(hp, name):
    case = build(COH_CASES[name])
    coh, df, co = dc.coh_reference(case)
    _upload(hp, case)
    got = hp.topic_coherence(case["tw"])
    again = hp.topic_coherence(case["tw"])
    for key in ("coherence", "doc_freq", "co_doc_freq"):
        assert got[key].tobytes() == again[key].tobytes(), key
    bad = np.argwhere(got["doc_freq"] != df)
    assert bad.size == 0, "%s: %d word counts differ, first (topic %d, word %d): %d vs %d" % (
        name, len(bad), bad[0][0], bad[0][1], got["doc_freq"][tuple(bad[0])], df[tuple(bad[0])])
    bad = np.argwhere(got["co_doc_freq"] != co)
    assert bad.size == 0, "%s: %d pair counts differ, first (topic %d, pair %d): %d vs %d" % (
        name, len(bad), bad[0][0], bad[0][1], got["co_doc_freq"][tuple(bad[0])], co[tuple(bad[0])])
    nan = np.isnan(coh)
    assert np.array_equal(np.isnan(got["coherence"]), nan)
    assert np.array_equal(got["coherence"][~nan].view(np.uint64), coh[~nan].view(np.uint64))   # bit for bit
    STATS[("coherence " + name)] = dict(counters=int(dc.coh_plan(case["tw"])["N"]), tile=int(dc.coh_tile(case["V"])), pairs_counted=int(co.sum()))


# ---- log-combinatorial -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC_CASES))
def test_log_combinatorial_case(hp, name):
    case = build(LC_CASES[name])
    want = dc.log_comb_reference(case)
    _upload(hp, case)
    got, again = hp.log_combinatorial(), hp.log_combinatorial()
    assert got.tobytes() == again.tobytes()
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, "%s: %d documents differ in their bits, first %d: %r vs %r" % (name, bad.size, bad[0], got[bad[0]], want[bad[0]])
    STATS["log-combinatorial " + name] = dict(table_entries=int(dc.doc_words(case).max()) + 1)


def test_log_combinatorial_refuses_a_count_of_2_31(hp):
    _upload(hp, dc.lc_case("refuse"))
    with pytest.raises(IsleHipError, match=r"error -1: log_combinatorial: a document holds 2147483648 words"):
        hp.log_combinatorial()
    _usable(hp)


# ---- top five --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T5_CASES))
def test_top_five_case(hp, name):
    case = build(T5_CASES[name])
    ref = dc.top5_reference(case)
    _upload(hp, case)
    got = hp.distinct_top_five_sets(m=dc.MS, fetch_quintuples=True)
    again = hp.distinct_top_five_sets(m=dc.MS, fetch_quintuples=True)
    assert got["quintuples"].tobytes() == again["quintuples"].tobytes() and got["run_lengths"].tobytes() == again["run_lengths"].tobytes()
    assert got["counts"] == again["counts"]
    assert got["num_quintuples"] == len(ref["tuples"])
    bad = np.argwhere(_bits(got["quintuples"]) != _bits(ref["tuples"]))
    assert bad.size == 0, "%s: %d tuple entries differ, first at sorted position %d: %s vs %s" % (
        name, len(bad), bad[0][0], got["quintuples"][bad[0][0]], ref["tuples"][bad[0][0]])
    assert got["run_lengths"].tolist() == ref["runs"]
    assert got["counts"] == {m: literal(ref["run_ids"], m) for m in dc.MS}
    STATS["top-five " + name] = dict(tuples=len(ref["tuples"]), runs=len(ref["runs"]))


# ---- the average model, its top words and its diversity ----------------------------------------------------------------------------
def _avg_model(hp, case):
    """A uploaded, B by thresholding (checked against the plain reference), the partition installed by the catchword pass."""
    _upload(hp, case)
    info = hp.threshold(case["k"])
    sc.assert_same_B(hp.get_B(), case["B"], "B of the average-model case")
    assert info["avg_doc_sz"] == case["B"]["avg"]
    k = case["topics"]
    hp.find_catchwords(k, case["r"], assign=case["assign"], fetch_thresholds=False)
    return hp.avg_topic_model(k)


@pytest.mark.parametrize("name", dc.AVG_CASES)
def test_average_model_case(hp, name):
    case = dc.avg_case(name)
    ref = dc.avg_reference(case)
    k, V = case["topics"], case["V"]
    M = _avg_model(hp, case)
    assert M.tobytes() == hp.avg_topic_model(k).tobytes()
    res = dc.certify_avg(np.ascontiguousarray(M), case, ref)
    print("average model %s: %s, error / bound %.4g, %d entries with q >= 2^32" % (name, res["mode"], res["ratio"], ref["n_hi"]))
    s = STATS.setdefault("average-model " + name, {})
    s.update(mode=res["mode"], model=res["ratio"], entries_hi=ref["n_hi"])
    # the resident model through the two readers
    for n in sorted({1, min(V, 32)}):
        ids, w = hp.model_top_words(n, "avg", with_weights=True)
        ids2, w2 = hp.model_top_words(n, "avg", with_weights=True)
        assert ids.tobytes() == ids2.tobytes() and w.tobytes() == w2.tobytes()
        want = top_words(M, n)
        assert np.array_equal(ids, want)
        assert np.array_equal(_bits(w), _bits(M[want.astype(np.int64), np.arange(k)[:, None]]))
    dref = dc.diversity_reference(M)
    d = hp.topic_diversity(k, "avg")
    d2 = hp.topic_diversity(k, "avg")
    assert d["dist"].tobytes() == d2["dist"].tobytes() and (d["avg"] == d2["avg"] or dref["kp"] == 0)
    s["diversity"] = dc.certify_diversity(d, dref)
    print("diversity of it: error / bound %.4g" % s["diversity"])


def test_the_accumulator_range_refusal_is_behind_thresholdings(hp):
    """vmax 2^e >= 2^64 needs normalised values more than 2^40 apart.  The corpus that would reach it (one document of 1024 entries of
    count 2^30 and one of count 1, and a single-entry document) has an average document size of about 2^39, which thresholding refuses
    before a partition can exist, and avg_topic_model asks for the partition: the refusal inside k_avg_model cannot be reached through
    the entry with a hand-built corpus."""
    docs = [[(w, 2 ** 30) for w in range(1024)] + [(1024, 1)], [(0, 7)]]
    case = dc.csc_of_counts(1025, docs)
    _upload(hp, case)
    with pytest.raises(IsleHipError, match=r"error -1: threshold: average document size .* too large"):
        hp.threshold(1)
    with pytest.raises(IsleHipError):
        hp.avg_topic_model(1)
    _usable(hp)


# ---- top words -------------------------------------------------------------------------------------------------------------------
def _check_top_words(M, n, ids, w, what):
    want = top_words(M, n)
    bad = np.argwhere(ids != want)
    assert bad.size == 0, "%s, n = %d: column %d: %s vs %s" % (what, n, bad[0][0], ids[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    assert np.array_equal(_bits(w), _bits(M[want.astype(np.int64), np.arange(M.shape[1])[:, None]])), "%s, n = %d: weights" % (what, n)


@pytest.mark.parametrize("name", sorted(TW_CASES))
def test_top_words_case(hp, name):
    case = build(TW_CASES[name])
    M = case["M"]
    for n in case["ns"]:
        ids, w = hp.model_top_words(n, M, with_weights=True)
        ids2, w2 = hp.model_top_words(n, M, with_weights=True)
        assert ids.tobytes() == ids2.tobytes() and w.tobytes() == w2.tobytes()
        _check_top_words(M, n, ids, w, name)


@pytest.mark.parametrize("ratio", dc.EDGE_RATIOS)
def test_edge_top_words_case(hp, ratio):
    M = dc.edge_model(ratio)
    pairs = np.array(dc.EDGE_PAIRS, np.int64)
    E = dc.edge_columns(M, dc.EDGE_PAIRS, ratio)
    lo, hi = dc.EDGE_TIE_WORDS
    for n in dc.tw_edge_case()["ns"]:
        ids, w = hp.edge_top_words(pairs, n, primary_ratio=ratio, model=M)
        ids2, w2 = hp.edge_top_words(pairs, n, primary_ratio=ratio, model=M)
        assert ids.tobytes() == ids2.tobytes() and w.tobytes() == w2.tobytes()
        _check_top_words(E, n, ids, w, "edge columns at ratio %g" % ratio)
        assert ids[0, 0] == lo and (n == 1 or ids[0, 1] == hi)


# ---- diversity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.DIV_CASES)
def test_diversity_case(hp, name):
    case = dc.div_case(name)
    M, V, k = case["M"], case["V"], case["k"]
    assert hp.load_model_text(dc.dense_text(M), V, k, format="dense") == V * k
    L = hp.loaded_model()
    assert np.array_equal(np.isnan(L), np.isnan(M)) and np.array_equal(_bits(L)[~np.isnan(M)], _bits(M)[~np.isnan(M)])
    ref = dc.diversity_reference(M)
    d, d2 = hp.topic_diversity(k, "loaded"), hp.topic_diversity(k, "loaded")
    assert d["dist"].tobytes() == d2["dist"].tobytes() and (d["avg"] == d2["avg"] or ref["kp"] == 0)
    ratio = dc.certify_diversity(d, ref)
    print("diversity %s: k' = %d, error / bound %.4g" % (name, ref["kp"], ratio))
    STATS["diversity " + name] = dict(finite_topics=ref["kp"], diversity=ratio)
