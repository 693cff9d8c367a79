"""The n heaviest documents of every topic selected on the device (isle_hip_topic_top_docs; HotPath.topic_top_docs;
isle_amd/csrc/topic_docs.hip) against the rule of tests/topdocs_rule.py, bit for bit: documents, value bits, counts, the topics' entry
counts and the unused slots.  Every case of the table runs through the caller's CSR; the refusals answer ISLE_E_ARG with their texts and
leave the context usable; the two resident sources run on a small trained corpus (V = 2000, D = 6000, k = 6: ingest, threshold, solver,
k-means, catchwords, topic model) and equal the rule applied to the arrays the getters return, and nothing resident changes.
tests/test_topdocs_rule_cpu.py holds the rule itself to a brute-force sort."""
import numpy as np
import pytest

import topdocs_rule as tr
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu
DEVICE_CASES = [c for c in tr.CASES if c.device]


def same(got, want, what):
    assert got["docs"].dtype == np.uint32 and got["values"].dtype == np.float32 and got["docs"].shape == want["docs"].shape, what
    assert np.array_equal(got["counts"], want["counts"]), (what, "counts")
    assert np.array_equal(got["topic_entries"], want["topic_entries"]), (what, "topic_entries")
    assert np.array_equal(got["docs"], want["docs"]), (what, "docs")
    assert np.array_equal(got["values"].view(np.uint32), want["values"]), (what, "values")  # the unused slots included: 0xffffffff / +0.0


def call(hp, c, n=None):
    return hp.topic_top_docs(c.n if n is None else n, (c.off, c.topic, c.values), num_topics=c.num_topics, doc_base=c.doc_base)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: c.name)
def test_every_case_of_the_table_is_the_rule(hp, case):
    same(call(hp, case), tr.rule(case), case.name)


def test_the_refusals_name_their_reason_and_leave_the_context_usable(hp):
    probe = tr.BY_NAME["absent_topic_and_fewer_than_n"]
    for r in tr.REFUSALS:
        with pytest.raises(IsleHipError) as e:
            hp.topic_top_docs(r.n, (r.off, r.topic, r.values), num_topics=r.num_topics, doc_base=r.doc_base)
        assert "isle_hip error -1" in str(e.value) and r.text in str(e.value), (r.name, str(e.value))
        same(call(hp, probe), tr.rule(probe), "after " + r.name)
    for c in tr.CASES:
        if not c.device:  # n = 300: the host statement alone has no limit
            with pytest.raises(IsleHipError, match=r"n = 300 not in \[1, 256\]"):
                call(hp, c)
    with pytest.raises(IsleHipError, match="num_topics = 0 < 1"):
        hp.topic_top_docs(5, (probe.off[:1], [], []), num_topics=0)
    with pytest.raises(IsleHipError, match="unknown source 7"):
        z = np.zeros(4, np.uint32)
        hp._chk(hp._lib.isle_hip_topic_top_docs(hp._h, 7, 1, 1, 0, 0, None, None, None, z.ctypes.data, z.ctypes.data, z.ctypes.data, None))
    with pytest.raises(IsleHipError, match="null docs"):
        hp._chk(hp._lib.isle_hip_topic_top_docs(hp._h, 2, 1, 1, 0, 0, None, None, None, None, None, None, None))
    same(call(hp, probe), tr.rule(probe), "at the end")


# ---- the resident sources ------------------------------------------------------------------------------------------------------------------------
V, D, K, SEED = 2000, 6000, 6, 5


def as_case(name, off, topic, value, k, n, doc_base):
    return tr.Case(name, k, n, doc_base, off, topic, np.ascontiguousarray(value, np.float32).view(np.uint32), "resident")


@pytest.fixture(scope="module")
def trained(hp):
    """ingest, threshold, solver, k-means, catchwords, topic model on the small corpus; "sums" before the topic model is refused on the way"""
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
    with pytest.raises(IsleHipError, match="topic_top_docs: run isle_hip_topic_model first"):
        hp.topic_top_docs(5, "sums", num_topics=K)
    tm = hp.construct_topic_model(K, O.model_rank_threshold(D, K), D)
    return dict(tm=tm, corpus=c)


def test_sums_is_the_rule_on_the_fetched_sums(hp, trained):
    tm = trained["tm"]
    assert tm["num_sums"] > 1000 and (tm["dts_val"] > 0).all()
    before = hp.doc_report_text("topic_sums_by_doc")
    for n, base in ((10, 0), (256, 77)):
        want = tr.rule(as_case("sums", tm["dts_off"], tm["dts_topic"], tm["dts_val"], K, n, base))
        got = hp.topic_top_docs(n, "sums", doc_base=base)                          # num_topics: the topic model's
        same(got, want, "sums n=%d" % n)
        same(hp.topic_top_docs(n, "sums", num_topics=K, doc_base=base), want, "sums again")  # a second call: the same arrays
    assert int(got["counts"].max()) == 256                                           # a topic with more than 256 documents
    assert hp.doc_report_text("topic_sums_by_doc") == before
    off = np.empty(D + 1, np.int64)
    tp = np.empty(tm["num_sums"], np.uint32)
    va = np.empty(tm["num_sums"], np.float32)
    hp._chk(hp._lib.isle_hip_get_doc_topic_sums(hp._h, off.ctypes.data, tp.ctypes.data, va.ctypes.data))
    assert off.tobytes() == tm["dts_off"].tobytes() and tp.tobytes() == tm["dts_topic"].tobytes() and va.tobytes() == tm["dts_val"].tobytes()
    with pytest.raises(IsleHipError, match="num_topics = 7, the resident topic model has 6 topics"):
        hp.topic_top_docs(5, "sums", num_topics=K + 1)


def test_infer_is_the_rule_on_the_fetched_entries(hp, trained):
    b, e = 123, 5800
    inf = hp.infer_resident("catch", docs=(b, e), min_weight=0.05)
    assert inf["nentries"] > 1000
    text = hp.infer_text("entries", base=b + 1)
    for n in (10, 256):
        want = tr.rule(as_case("infer", inf["offs"], inf["topic"], inf["weight"], K, n, b))
        same(hp.topic_top_docs(n, "infer", doc_base=b), want, "infer n=%d" % n)     # num_topics: the model's columns
        same(hp.topic_top_docs(n, "infer", num_topics=K, doc_base=b), want, "infer again")
    assert hp.infer_text("entries", base=b + 1) == text
    again = hp.infer_entries(e - b, inf["nentries"])
    assert all(x.tobytes() == inf[name].tobytes() for x, name in zip(again, ("offs", "topic", "weight")))
    with pytest.raises(IsleHipError, match="entry .* has topic . >= num_topics 2"):   # the device check reads the resident entries too
        hp.topic_top_docs(5, "infer", num_topics=2, doc_base=b)
    same(hp.topic_top_docs(256, "infer", doc_base=b), want, "infer after a refusal")


def test_infer_after_a_new_count_matrix_is_refused(hp, trained):
    cnt, rows, offs = trained["corpus"].A()
    hp.upload_counts(V, cnt, rows, offs)
    with pytest.raises(IsleHipError, match="topic_top_docs: no resident result"):
        hp.topic_top_docs(5, "infer", num_topics=K)
    with pytest.raises(IsleHipError, match="topic_top_docs: run isle_hip_topic_model first"):
        hp.topic_top_docs(5, "sums", num_topics=K)
