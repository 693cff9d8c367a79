"""isle_hip_kmeans_objective on one rank against tests/objective_certificate.py: crafted partitions and centres through the explicit
arguments in both spaces, the resident inputs of both loops against the same inputs passed explicitly, the trace of both loops against
the objective of the shorter runs, and the refusals by their messages.  Every comparison of two device results is bit for bit."""
import numpy as np
import pytest

import objective_certificate as oc
import shard_cases as sc

pytestmark = pytest.mark.gpu

RES_K = 65  # the resident and trace cases: more centres than a wave has lanes, round4(k) != k


@pytest.fixture(scope="module")
def hp():
    from isle_amd import HotPath
    h = HotPath(0)
    yield h
    h.close()


def same_bits(a, b, what):
    for f in ("sums", "sizes", "doc_dist"):
        if f in a or f in b:
            assert np.array_equal(np.asarray(a[f]).view(np.uint64), np.asarray(b[f]).view(np.uint64)), "%s: %s differs" % (what, f)
    assert np.float64(a["total"]).view(np.uint64) == np.float64(b["total"]).view(np.uint64), "%s: total differs" % what


def upload(hp, B):
    hp.upload_csc(B["V"], B["vals"], B["rows"], B["offs"])


@pytest.mark.parametrize("kind", ("crafted", "one"))
@pytest.mark.parametrize("k", oc.CASE_KS)
def test_word_space_explicit_inputs_lie_within_the_certificate_and_repeat_bit_for_bit(hp, k, kind):
    """documents of 0, 1, 63, 64, 65 and 200 entries, an empty cluster, a one-member cluster on its document's bits, twin centres, the
    outlier that sets the quantum; then the same call again, and again behind a Lloyd iteration that rebuilt the member lists"""
    B = oc.case_corpus()
    a, C = oc.case_partition(k, kind), oc.case_word_centers(k)
    truth, bound = oc.word_truth(B, a, C)
    upload(hp, B)
    got = hp.kmeans_objective(k, "word", assign=a, centers=C, fetch_docs=True)
    worst = oc.certify(got, truth, bound, a, k)
    print("objective certificate, word k=%d %s: worst error / bound %r" % (k, kind, worst))
    if k >= 5 and kind == "crafted":
        assert got["doc_dist"][4] == 0.0 and got["sums"][1] == 0.0 and got["sizes"][1] == 1
        assert got["sums"][k - 1] == 0.0 and got["sizes"][k - 1] == 0
    same_bits(got, hp.kmeans_objective(k, "word", assign=a, centers=C, fetch_docs=True), "second call")
    hp.run_lloyds(k, centers=C, max_reps=2)  # member lists of another partition, resident centres and partition of its own
    same_bits(got, hp.kmeans_objective(k, "word", assign=a, centers=C, fetch_docs=True), "behind run_lloyds")
    same_bits(got, hp.kmeans_objective(k, "word", assign=a, centers=C, fetch_docs=True), "behind run_lloyds, again")


@pytest.mark.parametrize("k", oc.CASE_KS)
def test_projected_space_explicit_inputs_lie_within_the_certificate_and_repeat_bit_for_bit(hp, k):
    B = oc.case_corpus()
    upload(hp, B)
    hp.set_U(oc.case_U(k))
    P = hp.get_projection(k)
    for kind in ("crafted", "one"):
        a, C = oc.case_partition(k, kind), oc.case_proj_centers(k, P)
        truth, bound = oc.proj_truth(P, a, C)
        got = hp.kmeans_objective(k, "projected", assign=a, centers=C, fetch_docs=True)
        worst = oc.certify(got, truth, bound, a, k)
        print("objective certificate, projected k=%d %s: worst error / bound %r" % (k, kind, worst))
        if k >= 5 and kind == "crafted":
            assert got["doc_dist"][4] == 0.0 and got["sums"][1] == 0.0 and got["sums"][k - 1] == 0.0
        same_bits(got, hp.kmeans_objective(k, "projected", assign=a, centers=C, fetch_docs=True), "second call")
    hp.run_lloyds_on_projected_space(k, C, max_reps=2)
    assert np.array_equal(P, hp.get_projection(k))
    same_bits(got, hp.kmeans_objective(k, "projected", assign=a, centers=C, fetch_docs=True), "behind run_lloyds_on_projected_space")


def test_resident_inputs_equal_the_explicit_ones_and_catchwords_reads_what_it_read(hp):
    """projected loop -> lift -> Lloyd on B on shard_cases.km_corpus: the resident call of each space is the explicit call on what the
    loop returned, both within the certificate; the catchword stage gives the same before and after the objective calls"""
    k = RES_K
    c = sc.km_ref(False, k)
    B = c.B
    hp.upload_counts(B["V"], np.maximum(1, np.rint(8 * B["vals"])), B["rows"], B["offs"])
    upload(hp, B)
    hp.set_U(c.U)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=3)
    res = hp.kmeans_objective(k, "projected", fetch_docs=True)
    same_bits(res, hp.kmeans_objective(k, "projected", assign=lp["assign"], centers=lp["C_lowd"], fetch_docs=True), "projected, resident against explicit")
    P = hp.get_projection(k)
    oc.certify(res, *oc.proj_truth(P, lp["assign"], lp["C_lowd"]), lp["assign"], k)
    hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
    ls = hp.run_lloyds(k, max_reps=3)
    before = hp.find_catchwords(k, 3)
    res = hp.kmeans_objective(k, "word", fetch_docs=True)
    same_bits(res, hp.kmeans_objective(k, "word", assign=ls["assign"], centers=ls["centers"], fetch_docs=True), "word, resident against explicit")
    oc.certify(res, *oc.word_truth(B, ls["assign"], ls["centers"]), ls["assign"], k)
    # other inputs through the scratch, both spaces, then the resident ones again
    other = ((ls["assign"].astype(np.int64) + 1) % k).astype(np.uint32)
    hp.kmeans_objective(k, "word", assign=other, centers=np.asfortranarray(ls["centers"][:, ::-1]))
    hp.kmeans_objective(k, "projected", assign=other, centers=lp["C_lowd"][::-1].copy())
    same_bits(res, hp.kmeans_objective(k, "word", fetch_docs=True), "word, resident, behind explicit calls")
    after = hp.find_catchwords(k, 3)
    assert before["num_catchwords"] == after["num_catchwords"] and np.array_equal(before["catch_topic"], after["catch_topic"])
    assert np.array_equal(before["thresholds"].view(np.uint32), after["thresholds"].view(np.uint32))


def km_start(hp, k):
    c = sc.km_ref(False, k)
    upload(hp, c.B)
    hp.set_U(c.U)
    return c, hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)["C_lowd"]


def test_the_trace_is_the_objective_of_the_shorter_runs_and_off_changes_nothing(hp):
    k, reps = RES_K, 3
    c, C0 = km_start(hp, k)
    hp.lloyds_trace(True)
    try:
        lp = hp.run_lloyds_on_projected_space(k, C0, max_reps=reps)
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k, max_reps=reps)
    finally:
        hp.lloyds_trace(False)
    assert len(lp["objective"]) == lp["iters"] and len(ls["objective"]) == ls["iters"] and lp["iters"] >= 2 and ls["iters"] >= 2
    for i in range(lp["iters"]):
        hp.run_lloyds_on_projected_space(k, C0, max_reps=i + 1)
        want = hp.kmeans_objective(k, "projected")["total"]
        assert np.float64(lp["objective"][i]).view(np.uint64) == np.float64(want).view(np.uint64), "projected trace[%d]" % i
    for i in range(ls["iters"]):
        hp.run_lloyds_on_projected_space(k, C0, max_reps=reps)  # the same calls in the same order as the traced run
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        hp.run_lloyds(k, max_reps=i + 1)
        want = hp.kmeans_objective(k, "word")["total"]
        assert np.float64(ls["objective"][i]).view(np.uint64) == np.float64(want).view(np.uint64), "word trace[%d]" % i
    # the trace off: no key, and the same partition and centres bit for bit
    lp0 = hp.run_lloyds_on_projected_space(k, C0, max_reps=reps)
    hp.left_multiply_by_U(lp0["C_lowd"], fetch=False)
    ls0 = hp.run_lloyds(k, max_reps=reps)
    assert "objective" not in lp0 and "objective" not in ls0
    assert np.array_equal(lp0["assign"], lp["assign"]) and np.array_equal(lp0["C_lowd"].view(np.uint32), lp["C_lowd"].view(np.uint32))
    assert np.array_equal(ls0["assign"], ls["assign"]) and np.array_equal(ls0["centers"].view(np.uint32), ls["centers"].view(np.uint32))


def test_refusals_by_message(hp):
    from isle_amd import IsleHipError
    import ctypes as C
    k = 5
    B = oc.case_corpus()
    a, Cw = oc.case_partition(k, "crafted"), oc.case_word_centers(k)
    upload(hp, B)  # a new matrix: nothing resident

    def refused(what, fn):
        with pytest.raises(IsleHipError, match=what):
            fn()

    rc = hp._lib.isle_hip_kmeans_objective(hp._h, 2, k, None, None, None, None, None, None)
    assert rc == -1 and b"unknown space 2" in hp._lib.isle_hip_last_error(hp._h)
    n = C.c_int()
    assert hp._lib.isle_hip_lloyds_trace_get(hp._h, 7, None, 0, C.byref(n)) == -1
    refused("no resident partition for the word space and k = 5", lambda: hp.kmeans_objective(k, "word", centers=Cw))
    refused("no resident centres for the word space and k = 5", lambda: hp.kmeans_objective(k, "word", assign=a))
    bad = a.copy()
    bad[17] = k
    refused(r"assign\[17\] = 5 out of range", lambda: hp.kmeans_objective(k, "word", assign=bad, centers=Cw))
    refused("projected space needs U of k = 5 columns, U has 0", lambda: hp.kmeans_objective(k, "projected", assign=a, centers=Cw[:k, :k]))
    hp.set_U(oc.case_U(k + 1))
    refused("projected space needs U of k = 5 columns, U has 6", lambda: hp.kmeans_objective(k, "projected", assign=a, centers=Cw[:k, :k]))
    hp.set_U(oc.case_U(k))
    refused("no resident partition for the projected space and k = 5", lambda: hp.kmeans_objective(k, "projected"))
    lp = hp.run_lloyds_on_projected_space(k, hp.get_projection(k)[:k].copy(), max_reps=2)
    hp.kmeans_objective(k, "projected")
    refused("projected space needs U of k = 4 columns, U has 5", lambda: hp.kmeans_objective(4, "projected"))
    refused("no resident partition for the word space and k = 5", lambda: hp.kmeans_objective(k, "word", centers=Cw))  # the last loop was the other space's
    hp.set_U(oc.case_U(k))  # a new U: P is released
    refused("projection P of the resident partition was released", lambda: hp.kmeans_objective(k, "projected"))
    hp.kmeans_objective(k, "projected", assign=lp["assign"], centers=lp["C_lowd"])  # explicit inputs form P again
    hp.run_lloyds(k, centers=Cw, max_reps=1)
    refused("no resident partition for the projected space and k = 5", lambda: hp.kmeans_objective(k, "projected"))
    hp.kmeans_objective(k, "word")
    with pytest.raises(ValueError):
        hp.kmeans_objective(k, "sideways")


def test_both_accumulation_forms_at_their_edge_give_the_same_bits(hp):
    """k = 1024 accumulates per workgroup in LDS, k = 1025 by global atomics (route_objective_acc): the same partition under the same
    first 1024 centres gives the same sums bit for bit, both within the certificate, in both spaces (the centres beyond: an empty cluster)"""
    B = oc.case_corpus()
    upload(hp, B)
    rng = np.random.default_rng(9)
    a = rng.integers(0, 1024, oc.CASE_D).astype(np.uint32)
    Cw = np.asfortranarray((0.3 * rng.random((oc.CASE_V, 1025))).astype(np.float32))
    got = {}
    for k in (1024, 1025):
        C = np.asfortranarray(Cw[:, :k])
        got[k] = hp.kmeans_objective(k, "word", assign=a, centers=C, fetch_docs=True)
        oc.certify(got[k], *oc.word_truth(B, a, C), a, k)
    assert np.array_equal(got[1024]["sums"].view(np.uint64), got[1025]["sums"][:1024].view(np.uint64)) and got[1025]["sums"][1024] == 0.0
    assert np.array_equal(got[1024]["doc_dist"].view(np.uint64), got[1025]["doc_dist"].view(np.uint64)) and got[1024]["total"] == got[1025]["total"]
