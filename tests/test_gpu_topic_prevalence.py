"""Topic prevalence by group of documents, summed on the device (isle_hip_topic_prevalence; HotPath.topic_prevalence;
isle_amd/csrc/topic_prevalence.hip) against the rule of tests/prevalence_rule.py: == on the integers (docs, unlabelled, count, dominant) and on
the bits of the doubles (sum).  Every case of the table runs through the caller's CSR in both tile forms and with both settings of normalise,
and a second call gives the same bits; the refusals found on the device name the first offender, the others their reason, and all leave the
context usable; the two resident sources run on the small trained corpus of tests/test_gpu_top_docs.py (V = 2000, D = 6000, k = 6) and equal
the rule applied to the arrays the getters return, and nothing resident changes; under a two-rank host-staged communicator the call is
refused on both ranks before any collective (tests/rank_launch.py).  tests/test_prevalence_rule_cpu.py holds the rule itself to fractions,
and shows that the cases marked `order` differ from a sequential sum, so that the comparison of bits here tests the order of summation."""
import numpy as np
import pytest

import prevalence_rule as pr
import rank_launch
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu
_FAILED = []


def same(got, want, what):
    assert got["docs"].dtype == np.uint64 and got["count"].dtype == np.uint64 and got["sum"].dtype == np.float64, what
    assert got["sum"].shape == want["sum"].shape and got["mean"].shape == want["sum"].shape, what
    assert np.array_equal(got["docs"], want["docs"]), (what, "docs")
    assert got["unlabelled"] == int(want["unlabelled"][0]), (what, "unlabelled")
    assert np.array_equal(got["count"], want["count"]), (what, "count")
    assert np.array_equal(got["dominant"], want["dominant"]), (what, "dominant")
    assert np.array_equal(got["sum"].view(np.uint64), want["sum"]), (what, "sum")
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = got["sum"] / got["docs"].astype(np.float64)[:, None]
    assert got["mean"].tobytes() == mean.tobytes() and np.isnan(got["mean"][got["docs"] == 0]).all(), (what, "mean")


def call(hp, c, normalise):
    return hp.topic_prevalence(c.source_arg(), c.groups, c.num_groups, bool(normalise), c.num_topics)


@pytest.fixture()
def tp(hp):
    yield hp
    hp.prevalence_tile_form("auto")


@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c.name)
def test_every_case_of_the_table_is_the_rule_in_both_forms(tp, case):
    for normalise in (0, 1):
        want = pr.rule(case, normalise)
        for form in pr.FORMS:
            tp.prevalence_tile_form(form)
            same(call(tp, case, normalise), want, (case.name, normalise, form))
        same(call(tp, case, normalise), want, (case.name, normalise, "again"))  # a second call: the same bits


def test_num_groups_and_num_topics_default_to_what_the_arrays_hold(tp):
    c = pr.BY_NAME["three_groups_0_64_65"]
    want = pr.rule(c, 0)
    same(tp.topic_prevalence(c.source_arg(), c.groups), want, "defaults")  # the largest label that is not NONE + 1; the largest topic + 1
    one = pr.BY_NAME["one_group_65"]
    same(tp.topic_prevalence(one.source_arg()), pr.rule(one, 0), "no labels")
    with pytest.raises(ValueError, match="groups: 3 labels for the 65 rows"):
        tp.topic_prevalence(one.source_arg(), [0, 0, 0])


def test_the_refusals_name_the_first_offender_and_leave_the_context_usable(tp):
    probe = pr.BY_NAME["three_groups_0_64_65"]
    want = pr.rule(probe, 1)
    for form in pr.FORMS:
        tp.prevalence_tile_form(form)
        for r in pr.REFUSALS:
            text = pr.first_fault_text(r)
            assert text
            with pytest.raises(IsleHipError) as e:
                call(tp, r, 0)
            assert "isle_hip error -1" in str(e.value) and text in str(e.value), (r.name, str(e.value))
            same(call(tp, probe, 1), want, "after " + r.name)
    good = pr.BY_NAME["one_group_65"]
    src = good.source_arg()
    for kw, text in ((dict(num_groups=2), "null groups with num_groups = 2"),
                     (dict(num_topics=0), r"num_topics = 0 not in \[1, 8192\]"),
                     (dict(num_topics=8193), r"num_topics = 8193 not in \[1, 8192\]"),
                     (dict(groups=np.zeros(65, np.uint32), num_groups=0), "num_groups = 0 < 1"),
                     (dict(normalise=2), "normalise = 2, not 0 or 1"),
                     (dict(num_topics=4), "has topic 4 >= num_topics 4")):
        args = dict(source=src, num_topics=good.num_topics)
        args.update(kw)
        with pytest.raises(IsleHipError, match="topic_prevalence: .*" + text):
            tp.topic_prevalence(**args)
    z = np.zeros(8, np.uint64)
    zp = z.ctypes.data
    lib, h = tp._lib, tp._h
    with pytest.raises(IsleHipError, match="topic_prevalence: unknown source 7"):
        tp._chk(lib.isle_hip_topic_prevalence(h, 7, 1, 0, None, None, None, None, 1, 0, zp, None, zp, zp, zp))
    with pytest.raises(IsleHipError, match="topic_prevalence: 2049 groups x 8192 topics are more than 16777216 cells"):  # (refused before anything is read)
        tp._chk(lib.isle_hip_topic_prevalence(h, 2, 8192, 0, None, None, None, zp, 2049, 0, zp, None, zp, zp, zp))
    with pytest.raises(IsleHipError, match="topic_prevalence: null docs / count / dominant / sum"):
        tp._chk(lib.isle_hip_topic_prevalence(h, 2, 1, 0, None, None, None, None, 1, 0, zp, None, zp, zp, None))
    with pytest.raises(IsleHipError, match="topic_prevalence: null doc_offsets with 3 rows"):
        tp._chk(lib.isle_hip_topic_prevalence(h, 2, 1, 3, None, None, None, None, 1, 0, zp, None, zp, zp, zp))
    with pytest.raises(IsleHipError, match="topic_prevalence: doc_offsets descend at row 1"):
        tp.topic_prevalence((np.array([0, 2, 1, 3]), np.array([0, 1, 0]), np.ones(3, np.float32)), num_topics=2)
    with pytest.raises(IsleHipError, match="prevalence_tile_form: unknown form 3"):
        tp.prevalence_tile_form(3)
    same(call(tp, probe, 1), want, "at the end")  # (the form is still the last one set)


# ---- the resident sources ------------------------------------------------------------------------------------------------------------------------
V, D, K, SEED = 2000, 6000, 6, 5


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
    with pytest.raises(IsleHipError, match="topic_prevalence: run isle_hip_topic_model first"):
        hp.topic_prevalence("sums", num_topics=K)
    with pytest.raises(IsleHipError, match="topic_prevalence: no resident result"):
        hp.topic_prevalence("infer", num_topics=K)
    tm = hp.construct_topic_model(K, O.model_rank_threshold(D, K), D)
    return dict(tm=tm, corpus=c)


def labels_for(rows, G, seed):
    lab = np.random.RandomState(seed).randint(0, G, rows).astype(np.uint32)
    lab[::13] = pr.NONE
    return lab


def test_sums_is_the_rule_on_the_fetched_sums(tp, trained):
    tm = trained["tm"]
    assert tm["num_sums"] > 1000
    before = tp.doc_report_text("topic_sums_by_doc")
    rows = (tm["dts_off"], tm["dts_topic"], tm["dts_val"])
    lab = labels_for(D, 50, 1)
    for form in pr.FORMS:
        tp.prevalence_tile_form(form)
        for normalise in (0, 1):
            same(tp.topic_prevalence("sums", normalise=bool(normalise)), pr.rule(pr.Case("sums", K, rows), normalise), ("sums", normalise, form))
            same(tp.topic_prevalence("sums", lab, 50, bool(normalise), K), pr.rule(pr.Case("sums50", K, rows, lab, 50), normalise), ("sums50", normalise, form))
    assert tp.doc_report_text("topic_sums_by_doc") == before
    off = np.empty(D + 1, np.int64)
    tpc = np.empty(tm["num_sums"], np.uint32)
    va = np.empty(tm["num_sums"], np.float32)
    tp._chk(tp._lib.isle_hip_get_doc_topic_sums(tp._h, off.ctypes.data, tpc.ctypes.data, va.ctypes.data))
    assert off.tobytes() == tm["dts_off"].tobytes() and tpc.tobytes() == tm["dts_topic"].tobytes() and va.tobytes() == tm["dts_val"].tobytes()
    with pytest.raises(IsleHipError, match="num_topics = 7, the resident topic model has 6 topics"):
        tp.topic_prevalence("sums", num_topics=K + 1)
    with pytest.raises(ValueError, match="groups: 5 labels for the 6000 rows"):
        tp.topic_prevalence("sums", np.zeros(5, np.uint32))


def test_infer_is_the_rule_on_the_fetched_entries(tp, trained):
    b, e = 123, 5800
    inf = tp.infer_resident("catch", docs=(b, e), min_weight=0.05)
    assert inf["nentries"] > 1000
    text = tp.infer_text("entries", base=b + 1)
    rows = (inf["offs"], inf["topic"], inf["weight"])
    lab = labels_for(e - b, 7, 2)
    for form in pr.FORMS:
        tp.prevalence_tile_form(form)
        for normalise in (0, 1):
            same(tp.topic_prevalence("infer", normalise=bool(normalise)), pr.rule(pr.Case("infer", K, rows), normalise), ("infer", normalise, form))
            same(tp.topic_prevalence("infer", lab, None, bool(normalise)), pr.rule(pr.Case("infer7", K, rows, lab, 7), normalise), ("infer7", normalise, form))
    assert tp.infer_text("entries", base=b + 1) == text
    again = tp.infer_entries(e - b, inf["nentries"])
    assert all(x.tobytes() == inf[name].tobytes() for x, name in zip(again, ("offs", "topic", "weight")))
    with pytest.raises(IsleHipError, match="num_topics = 2, the resident inference result has 6 topics"):
        tp.topic_prevalence("infer", num_topics=2)
    same(tp.topic_prevalence("infer"), pr.rule(pr.Case("infer", K, rows), 0), "infer after a refusal")


def test_after_a_new_count_matrix_both_sources_are_refused(hp, trained):
    cnt, rows, offs = trained["corpus"].A()
    hp.upload_counts(V, cnt, rows, offs)
    with pytest.raises(IsleHipError, match="topic_prevalence: no resident result"):
        hp.topic_prevalence("infer", num_topics=K)
    with pytest.raises(IsleHipError, match="topic_prevalence: run isle_hip_topic_model first"):
        hp.topic_prevalence("sums", num_topics=K)


# ---- several ranks: refused before any collective -----------------------------------------------------------------------------------------------
def _worker(hp, rank, world, res):
    c = pr.BY_NAME["one_group_65"]
    try:
        hp.topic_prevalence(c.source_arg(), num_topics=c.num_topics)
        res["text"] = np.array("accepted")
    except IsleHipError as e:
        res["text"] = np.array(str(e))
    # a collective call behind the refusal: had a rank entered a collective of its own, this one would not pair up
    top = hp.topic_top_docs(3, c.source_arg(), num_topics=c.num_topics, doc_base=rank * c.rows)
    res["top.docs"], res["top.entries"] = top["docs"], top["topic_entries"]


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("topic_prevalence_ranks"))
    job = lambda: rank_launch.launch("topic prevalence W2", "prevalence_W2", 2, tmp, rank_launch.module_command("test_gpu_topic_prevalence", 2))
    return rank_launch.launch_each([(2, "W2", job)], _FAILED)


def test_two_ranks_are_refused_on_both_ranks_before_any_collective(two_ranks):
    ranks = rank_launch.ranks_of(two_ranks, 2)
    assert len(ranks) == 2
    c = pr.BY_NAME["one_group_65"]
    for res in ranks:
        assert "isle_hip error -1" in str(res["text"]) and "topic_prevalence: 2 ranks: a bit-equal sum across ranks" in str(res["text"])
        assert res["top.entries"].tolist() == (2 * np.bincount(c.topic, minlength=c.num_topics)).tolist()  # both ranks' rows: the collective paired up
        assert res["top.docs"].tobytes() == ranks[0]["top.docs"].tobytes()
