"""threshold.hip and post.hip at their kernel edges against the plain reference of tests/stages_certificate.py (lists and sorts, written
from the reference's source; no oracle library).  Thresholding: zetas, offsets, rows, values, original columns and the scalars, bit for
bit.  Downstream: thresholds, catchwords, document-topic sums, rank thresholds and the two heaviest topics bit for bit; the topic model
inside certify_model's derived bound, the edge topics inside certify_edge's.  test_stages_certificate_cpu.py asserts, without a GPU, that
every input here reaches the edge it was built for and would fail under the wrong rule.

At the end of the module the largest error / bound per case is printed (profiles/stages_certificate.md holds a measured run)."""
import json
import os
import time

import numpy as np
import pytest

import stages_certificate as sc
from stages_certificate import F, build, post_reference

pytestmark = pytest.mark.gpu

TH_CASES = sc.threshold_cases()
STATS = {}
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def certificate_summary():
    yield STATS
    wall = time.time() - _T0
    for name, s in sorted(STATS.items()):
        print("stages certificate, %s: model error / bound %.3g, edge error / bound %.3g" % (name, s.get("model", 0.0), s.get("edge", 0.0)))
    print("stages certificate: %.1f s" % wall)
    path = os.environ.get("STAGES_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(STATS, wall_seconds=wall), f, indent=1, sort_keys=True)


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _threshold(hp, case, **kw):
    hp.upload_counts(case["V"], case["cnt"], case["rows"], case["offs"], doc_offset=case.get("doc_offset", 0))
    info = hp.threshold(case["k"], **kw)
    return info, hp.get_B()


def _check_threshold(hp, case, name):
    want = sc.ref_threshold(case["V"], case["cnt"], case["rows"], case["offs"], case["k"], doc_base=case.get("doc_offset", 0))
    info, got = _threshold(hp, case)
    sc.assert_same_B(got, want, name)
    assert info["docs_kept"] == want["D"] and info["nnz_kept"] == want["nnz"]
    assert info["entries_above_threshold"] == want["entries_above"] and info["avg_doc_sz"] == want["avg"]
    return want, got


@pytest.mark.parametrize("name", sorted(TH_CASES))
def test_threshold_case(hp, name):
    """T-round, T-zeta, T-lanes, T-scan (D = 4097 with a non-zero doc_offset, which upload_counts accepts on a single rank), T-stride."""
    case = build(TH_CASES[name])
    want, got = _check_threshold(hp, case, name)
    if case.get("doc_offset"):
        assert got["original_cols"].min() >= case["doc_offset"]


def test_threshold_sampled_lanes(hp):
    """T-sampled: every kept column is the same document's column of the unsampled B, entries_above_threshold is the unsampled nnz, and
    the kept set is the CPU port's (the key draw is host code on both sides)."""
    from tools.synth import Corpus
    case = sc.t_lanes_case()
    full = sc.ref_threshold(case["V"], case["cnt"], case["rows"], case["offs"], case["k"])
    info, got = _threshold(hp, case, sample_rate=sc.SAMPLED_RATE, sample_seed=sc.SAMPLED_SEED)
    port = Corpus.from_csc(case["V"], len(case["offs"]) - 1, case["cnt"], case["rows"], case["offs"]).threshold(
        case["k"], sample_rate=sc.SAMPLED_RATE, sample_seed=sc.SAMPLED_SEED)
    assert np.array_equal(got["original_cols"], port["original_cols"]) and 0 < got["D"] < full["D"]
    assert info["entries_above_threshold"] == full["nnz"] and info["docs_kept"] == got["D"] and info["nnz_kept"] == got["nnz"]
    assert np.array_equal(_bits(got["zetas"]), _bits(full["zetas"]))
    col_of = {int(d): j for j, d in enumerate(full["original_cols"])}
    for j, d in enumerate(got["original_cols"]):
        jf = col_of[int(d)]
        a, b = slice(got["offs"][j], got["offs"][j + 1]), slice(full["offs"][jf], full["offs"][jf + 1])
        assert np.array_equal(got["rows"][a], full["rows"][b]) and np.array_equal(_bits(got["vals"][a]), _bits(full["vals"][b]))
    kept = set(int(d) for d in got["original_cols"])
    assert {(l["n"], l["pattern"]) for l in case["lanes"] if l["n"] >= 63 and l["doc"] in kept} == sc.SAMPLED_LANES_KEPT


# ---- downstream ------------------------------------------------------------------------------------------------------------------
def _post_upload(hp, case):
    """A on the device, B by thresholding (checked), -> number of documents of A."""
    info, got = _threshold(hp, case)
    sc.assert_same_B(got, case["B"], "B of the downstream case")
    return len(case["offs"]) - 1


def _check_post(hp, case, name, r=None, rho=1.1, rank=None, edges=False):
    R = post_reference(case, r=r, rho=rho, rank=rank)
    r = case["r"] if r is None else r
    rank = case.get("rank", 1) if rank is None else rank
    k, V, D = case["topics"], case["V"], len(case["offs"]) - 1
    got = hp.find_catchwords(k, r, assign=case["assign"], rho=rho)
    assert got["thresholds"].shape == R["thr"].shape
    bad = np.argwhere(_bits(got["thresholds"]) != _bits(R["thr"]))
    assert bad.size == 0, "%s: %d thresholds differ, first (word %d, topic %d): %r vs %r" % (
        name, len(bad), bad[0][0], bad[0][1], got["thresholds"][tuple(bad[0])], R["thr"][tuple(bad[0])])
    assert np.array_equal(got["catch_topic"], R["catch_topic"]), "%s: catch topics differ at words %s" % (
        name, np.flatnonzero(got["catch_topic"] != R["catch_topic"])[:10])
    assert got["num_catchwords"] == int((R["catch_topic"] >= 0).sum())
    tm = hp.construct_topic_model(k, rank, D)
    dts = R["dts"]
    assert tm["num_sums"] == len(dts["dts_val"])
    assert np.array_equal(tm["dts_off"], dts["dts_off"]) and np.array_equal(tm["dts_topic"], dts["dts_topic"])
    bad = np.flatnonzero(_bits(tm["dts_val"]) != _bits(dts["dts_val"]))
    assert bad.size == 0, "%s: %d document-topic sums differ in their bits, first %r vs %r" % (name, bad.size, tm["dts_val"][bad[0]], dts["dts_val"][bad[0]])
    assert np.array_equal(_bits(tm["model_threshold"]), _bits(R["mthr"])), "%s: rank thresholds %s vs %s" % (name, tm["model_threshold"], R["mthr"])
    assert np.array_equal(tm["top1"], dts["top1"]) and np.array_equal(tm["top2"], dts["top2"])
    res = sc.certify_model(tm["model"], R["model64"], R["m"], V)
    s = STATS.setdefault(name, {})
    s["model"] = max(s.get("model", 0.0), res["max_ratio"])
    s["model_bound_rel"] = max(s.get("model_bound_rel", 0.0), res["rel_max"])
    if edges:
        pairs = sc.edge_pairs(k, case.get("empty_topic"))
        E = hp.edge_topics(pairs)
        s["edge"] = max(s.get("edge", 0.0), sc.certify_edge(E, tm["model"], pairs)["max_ratio"])
        with pytest.raises(Exception):
            hp.edge_topics(np.array([[0, k]]))
    return R, tm


@pytest.mark.parametrize("k", sc.CATCH_K)
def test_catch_rule(hp, k):
    """P-catch: one document per cluster, r = 1, the designed threshold matrix, under rho = 1.1, 1.5 and 2.0."""
    case = sc.p_catch_case(k)
    _post_upload(hp, case)
    for rho in sc.CATCH_RHOS:
        _check_post(hp, case, "catch-%d" % k, rho=rho)


def test_threshold_arms(hp):
    """P-arms, with P-model and P-edge on it: an empty topic gives a NaN column; pairs with p == q and the last topic."""
    case = sc.p_arms_case()
    _post_upload(hp, case)
    R, tm = _check_post(hp, case, "arms", edges=True)
    assert np.isnan(tm["model"][:, 3]).all()


@pytest.mark.parametrize("r", sc.select_ranks())
def test_select(hp, r):
    """P-select: segments of 2, 255, 256, 257 and 1000 values (all equal; runs of equal values over the rank; a hundred values sharing
    their top 16 bits), the catchword rank and the per-topic rank both r: r == n - 1, n and n + 1 of every length are among them."""
    case = sc.p_select_case()
    _post_upload(hp, case)
    _check_post(hp, case, "select", r=r, rank=r)


@pytest.mark.parametrize("k", sc.DTS_K)
def test_doc_topic_sums_and_model(hp, k):
    """P-dts with P-model and P-edge on it (k > 64: the table loops take two and three trips)."""
    case = sc.p_dts_case(k)
    _post_upload(hp, case)
    R, tm = _check_post(hp, case, "dts-%d" % k, edges=True)
    assert np.isnan(tm["model"][:, case["empty_topic"]]).all()
    for rank in (1, 2):   # rank 1 and a rank above every topic's count on the same sums
        _check_post(hp, case, "dts-%d" % k, rank=rank)
    _check_post(hp, case, "dts-%d" % k, rank=10 ** 6)
