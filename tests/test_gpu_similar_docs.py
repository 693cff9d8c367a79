"""The documents most similar to a query document, scored and selected on the device (isle_hip_similar_docs; HotPath.similar_docs;
isle_amd/csrc/similar_docs.hip and the selection of topic_docs.hip) against the rule of tests/simdocs_rule.py, bit for bit: documents, score
bits, counts, candidate counts and the unused slots.  Every case of the table runs through the caller's CSR under all three measures and
under both homes of the query table (the two cases either side of the LDS threshold under "auto" as well); the refusals answer ISLE_E_ARG with
their texts and leave the context usable; the two resident sources run on the small trained corpus of tests/test_gpu_top_docs.py
(V = 2000, D = 6000, k = 6) with a handful of rows as queries and equal the rule applied to the arrays the getters return, and nothing
resident changes.  tests/test_simdocs_rule_cpu.py holds the rule itself to fractions and to a brute-force sort.
Weights in the table stay >= 2^-60 or are exactly 0, so that no fp32 product is subnormal: WHAT SUBNORMAL PRODUCTS DO IS NOT CERTIFIED."""
import numpy as np
import pytest

import simdocs_rule as sr
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu
RUNS = [(c, name, form) for c in sr.CASES for name in sr.MEASURES for form in c.forms]


def same(got, want, what):
    assert got["docs"].dtype == np.uint32 and got["scores"].dtype == np.float32 and got["docs"].shape == want["docs"].shape, what
    assert np.array_equal(got["counts"], want["counts"]), (what, "counts")
    assert np.array_equal(got["candidates"], want["candidates"]), (what, "candidates")
    assert np.array_equal(got["docs"], want["docs"]), (what, "docs")
    assert np.array_equal(got["scores"].view(np.uint32), want["scores"]), (what, "scores")  # the unused slots included: 0xffffffff / +0.0


@pytest.fixture(scope="module")
def rules():
    """the rule of a (case, measure), computed once and left unchanged"""
    memo = {}

    def get(case, measure):
        key = (case.name, measure)
        if key not in memo:
            memo[key] = sr.rule(case, sr.MEASURES[measure])
        return memo[key]

    return get


def call(hp, c, measure, **kw):
    args = dict(source=c.source_arg(), measure=measure, num_topics=c.num_topics, doc_base=c.doc_base,
                exclude=c.given_exclude)
    args.update(kw)
    return hp.similar_docs(c.queries_arg(), c.n, **args)


@pytest.fixture()
def sd(hp):
    yield hp
    hp.simdocs_table_form("auto")


@pytest.mark.parametrize("case,measure,form", RUNS, ids=["%s-%s-%s" % (c.name, m, f) for c, m, f in RUNS])
def test_every_case_of_the_table_is_the_rule(sd, rules, case, measure, form):
    sd.simdocs_table_form(form)
    want = rules(case, measure)
    same(call(sd, case, measure), want, case.name)
    if case.aim in ("tie", "query_rows"):
        same(call(sd, case, measure), want, case.name + " again")  # a second call: the same arrays


def test_the_refusals_name_their_reason_and_leave_the_context_usable(sd, rules):
    probe = sr.BY_NAME["zero_weights"]
    for r in sr.REFUSALS:
        kw = dict(source=sr.GOOD_ROWS, queries=sr.GOOD_QUERIES, n=5, measure="cosine", num_topics=3, doc_base=0)
        kw.update(r.kw)
        queries, n = kw.pop("queries"), kw.pop("n")
        with pytest.raises(IsleHipError) as e:
            sd.similar_docs(queries, n, **kw)
        assert "isle_hip error -1" in str(e.value) and "similar_docs: " in str(e.value) and r.text in str(e.value), (r.name, str(e.value))
        same(call(sd, probe, "cosine"), rules(probe, "cosine"), "after " + r.name)
    z = np.zeros(8, np.uint32)
    zp = z.ctypes.data
    off = np.zeros(2, np.int64)
    lib, h = sd._lib, sd._h
    with pytest.raises(IsleHipError, match="similar_docs: unknown source 7"):
        sd._chk(lib.isle_hip_similar_docs(h, 7, 0, 1, 1, 0, 0, None, None, None, 1, None, off.ctypes.data, None, None, None, zp, zp, zp, None))
    with pytest.raises(IsleHipError, match="similar_docs: null docs / scores / counts"):
        sd._chk(lib.isle_hip_similar_docs(h, 2, 0, 1, 1, 0, 0, None, None, None, 1, None, off.ctypes.data, None, None, None, None, None, None, None))
    with pytest.raises(IsleHipError, match="simdocs_table_form: unknown form 3"):
        sd.simdocs_table_form(3)
    for form in ("lds", "global", "auto"):
        sd.simdocs_table_form(form)
        same(call(sd, probe, "dot"), rules(probe, "dot"), "at the end, " + form)


# ---- the resident sources ------------------------------------------------------------------------------------------------------------------------
V, D, K, SEED = 2000, 6000, 6, 5
QUERY_ROWS = [0, 17, 2999, 17, 5676]


@pytest.fixture(scope="module")
def trained(hp):
    """ingest, threshold, solver, k-means, catchwords, topic model on the small corpus; "sums" before the topic model and "infer" before
    infer_resident are refused on the way"""
    from tools.synth import Corpus
    from oracle import oracle as O
    c = Corpus(V, D, K, SEED)
    hp.ingest_tdf(c.tdf_bytes(), V, D)
    hp.threshold(K)
    hp.compute_block_ks(K, seed=1)
    g = hp.kmeans_init_on_projected_space(K, rng_seed=1)
    lp = hp.run_lloyds_on_projected_space(K, g["C_lowd"])
    hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
    hp.run_lloyds(K, fetch_centers=False)
    hp.find_catchwords(K, O.catchword_rank(D, K), fetch_thresholds=False)
    with pytest.raises(IsleHipError, match="similar_docs: run isle_hip_topic_model first"):
        hp.similar_docs(QUERY_ROWS, 5, "sums", num_topics=K)
    with pytest.raises(IsleHipError, match="similar_docs: no resident result"):
        hp.similar_docs(QUERY_ROWS, 5, "infer", num_topics=K)
    tm = hp.construct_topic_model(K, O.model_rank_threshold(D, K), D)
    return dict(tm=tm, corpus=c)


def test_sums_is_the_rule_on_the_fetched_sums(hp, trained):
    tm = trained["tm"]
    assert tm["num_sums"] > 1000
    before = hp.doc_report_text("topic_sums_by_doc")
    top_before = hp.topic_top_docs(10, "sums")
    rows = (tm["dts_off"], tm["dts_topic"], tm["dts_val"])
    for measure in sr.MEASURES:
        for n, base in ((10, 0), (256, 77)):
            want = sr.rule(sr.Case("sums", K, n, base, rows, query_rows=QUERY_ROWS), sr.MEASURES[measure])
            got = hp.similar_docs(QUERY_ROWS, n, "sums", measure=measure, doc_base=base)  # num_topics: the topic model's
            same(got, want, "sums %s n=%d" % (measure, n))
            same(hp.similar_docs(QUERY_ROWS, n, "sums", measure=measure, num_topics=K, doc_base=base), want, "sums again")
    assert int(got["candidates"].max()) > 256
    assert hp.doc_report_text("topic_sums_by_doc") == before
    top_after = hp.topic_top_docs(10, "sums")
    assert all(top_after[k].tobytes() == top_before[k].tobytes() for k in top_before)
    off = np.empty(D + 1, np.int64)
    tp = np.empty(tm["num_sums"], np.uint32)
    va = np.empty(tm["num_sums"], np.float32)
    hp._chk(hp._lib.isle_hip_get_doc_topic_sums(hp._h, off.ctypes.data, tp.ctypes.data, va.ctypes.data))
    assert off.tobytes() == tm["dts_off"].tobytes() and tp.tobytes() == tm["dts_topic"].tobytes() and va.tobytes() == tm["dts_val"].tobytes()
    with pytest.raises(IsleHipError, match="num_topics = 7, the resident topic model has 6 topics"):
        hp.similar_docs(QUERY_ROWS, 5, "sums", num_topics=K + 1)
    with pytest.raises(IsleHipError, match=r"query_rows\[4\] = 6000 is not below the 6000 rows"):
        hp.similar_docs([0, 1, 2, 3, D], 5, "sums")


def test_infer_is_the_rule_on_the_fetched_entries(hp, trained):
    b, e = 123, 5800
    inf = hp.infer_resident("catch", docs=(b, e), min_weight=0.05)
    assert inf["nentries"] > 1000
    text = hp.infer_text("entries", base=b + 1)
    top_before = hp.topic_top_docs(10, "infer", doc_base=b)
    rows = (inf["offs"], inf["topic"], inf["weight"])
    for measure in sr.MEASURES:
        for n in (10, 256):
            want = sr.rule(sr.Case("infer", K, n, b, rows, query_rows=QUERY_ROWS), sr.MEASURES[measure])
            same(hp.similar_docs(QUERY_ROWS, n, "infer", measure=measure, doc_base=b), want, "infer %s n=%d" % (measure, n))
    ex = np.array([b, 0xFFFFFFFF, b + 2999, 5, b + 17], np.uint32)
    want = sr.rule(sr.Case("infer", K, 10, b, rows, query_rows=QUERY_ROWS, exclude=ex), sr.COSINE)
    same(hp.similar_docs(QUERY_ROWS, 10, "infer", num_topics=K, doc_base=b, exclude=ex), want, "infer with exclude")
    assert hp.infer_text("entries", base=b + 1) == text
    again = hp.infer_entries(e - b, inf["nentries"])
    assert all(x.tobytes() == inf[name].tobytes() for x, name in zip(again, ("offs", "topic", "weight")))
    top_after = hp.topic_top_docs(10, "infer", doc_base=b)
    assert all(top_after[k].tobytes() == top_before[k].tobytes() for k in top_before)
    with pytest.raises(IsleHipError, match="num_topics = 2, the resident inference result has 6 topics"):
        hp.similar_docs(QUERY_ROWS, 5, "infer", num_topics=2, doc_base=b)
    same(hp.similar_docs(QUERY_ROWS, 10, "infer", doc_base=b, exclude=ex), want, "infer after a refusal")


def test_after_a_new_count_matrix_both_sources_are_refused(hp, trained):
    cnt, rows, offs = trained["corpus"].A()
    hp.upload_counts(V, cnt, rows, offs)
    with pytest.raises(IsleHipError, match="similar_docs: no resident result"):
        hp.similar_docs(QUERY_ROWS, 5, "infer", num_topics=K)
    with pytest.raises(IsleHipError, match="similar_docs: run isle_hip_topic_model first"):
        hp.similar_docs(QUERY_ROWS, 5, "sums", num_topics=K)
