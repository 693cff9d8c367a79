"""tests/objective_certificate.py held to its own statement, without a GPU: a plain fp64 restatement of the objective passes in both
spaces for every crafted k, and the checker rejects each wrong answer it exists to catch."""
import numpy as np
import pytest

import objective_certificate as oc


def word_case(k, kind="crafted"):
    B = oc.case_corpus()
    a, C = oc.case_partition(k, kind), oc.case_word_centers(k)
    truth, bound = oc.word_truth(B, a, C)
    return B, a, C, truth, bound


@pytest.mark.parametrize("k", oc.CASE_KS)
@pytest.mark.parametrize("kind", ("crafted", "one"))
def test_the_fp64_restatement_passes_in_word_space(k, kind):
    B, a, C, truth, bound = word_case(k, kind)
    worst = oc.certify(oc.restate(truth, a, k), truth, bound, a, k)
    assert max(worst.values()) < 1.0
    if k >= 5 and kind == "crafted":
        assert truth[4] == 0 and np.bincount(a, minlength=k)[1] == 1 and np.bincount(a, minlength=k)[k - 1] == 0
        assert np.array_equal(C[:, 2], C[:, 3])


@pytest.mark.parametrize("k", oc.CASE_KS)
def test_the_fp64_restatement_passes_in_projected_space(k):
    B = oc.case_corpus()
    X = np.stack([oc.dense_doc(B, d) for d in range(B["D"])]).astype(np.float64)
    P = (X @ oc.case_U(k).astype(np.float64)).astype(np.float32)
    a, C = oc.case_partition(k, "crafted"), oc.case_proj_centers(k, P)
    truth, bound = oc.proj_truth(P, a, C)
    worst = oc.certify(oc.restate(truth, a, k), truth, bound, a, k)
    assert max(worst.values()) < 1.0
    if k >= 5:
        assert truth[4] == 0


def test_the_corpus_holds_the_edge_documents_and_the_outlier_sets_the_quantum():
    B = oc.case_corpus()
    assert tuple(np.diff(B["offs"])[:6]) == oc.CASE_LENGTHS and B["D"] == 333 and B["V"] == 257
    _, a, _, truth, bound = word_case(65)
    others = np.delete(truth, oc.OUTLIER_DOC)
    assert truth[oc.OUTLIER_DOC] > 64 * others.max()  # the others quantise at least 2^6 coarser than their own exponent asks


def rejected(got, truth, bound, a, k, what):
    with pytest.raises(AssertionError, match=what):
        oc.certify(got, truth, bound, a, k)


def test_a_document_moved_to_another_cluster_is_rejected():
    k = 65
    B, a, C, truth, bound = word_case(k)
    b = a.copy()
    b[10] = (a[10] + 1) % (k - 1)
    wrong, _ = oc.word_truth(B, b, C)
    rejected(oc.restate(wrong, b, k), truth, bound, a, k, "doc_dist\\[10\\]")
    got = oc.restate(wrong, b, k)
    got["doc_dist"] = None
    rejected(got, truth, bound, a, k, "cluster_sizes")


def test_the_centre_norm_left_out_is_rejected():
    k = 5
    B, a, C, truth, bound = word_case(k)
    cn = (C.astype(np.float64) ** 2).sum(axis=0)
    without = np.maximum(truth.astype(np.float64) - cn[a], 0)
    rejected(oc.restate(without.astype(oc.LD), a, k), truth, bound, a, k, "doc_dist")
    got = oc.restate(without.astype(oc.LD), a, k)
    got["doc_dist"] = None
    rejected(got, truth, bound, a, k, "cluster_sums")


def test_the_centres_of_the_previous_iteration_are_rejected():
    k = 65
    B, a, C, truth, bound = word_case(k)
    prev = np.asfortranarray(C * np.float32(1.0 + 2.0 ** -10))  # a centre update's worth of movement, far above any rounding
    wrong, _ = oc.word_truth(B, a, prev)
    got = oc.restate(wrong, a, k)
    got["doc_dist"] = None
    rejected(got, truth, bound, a, k, "cluster_sums")


def test_a_cluster_sum_off_by_four_bounds_is_rejected_and_by_a_quarter_passes():
    k = 65
    B, a, C, truth, bound = word_case(k)
    _, bnd_t, _ = oc.cluster_truth(truth, bound, a, k)
    for factor, ok in ((0.25, True), (4.0, False)):
        got = oc.restate(truth, a, k)
        got["sums"][2] += factor * bnd_t[2]
        tot = 0.0
        for t in range(k):
            tot += float(got["sums"][t])
        got["total"] = tot
        if ok:
            oc.certify(got, truth, bound, a, k)
        else:
            rejected(got, truth, bound, a, k, "cluster_sums\\[2\\]")


def test_a_sum_on_an_empty_cluster_is_rejected():
    k = 65
    B, a, C, truth, bound = word_case(k)
    got = oc.restate(truth, a, k)
    got["sums"][k - 1] = 2.0 ** -60
    rejected(got, truth, bound, a, k, "cluster %d is empty" % (k - 1))


def test_a_total_that_is_not_the_ascending_sum_is_rejected():
    k = 65
    B, a, C, truth, bound = word_case(k)
    got = oc.restate(truth, a, k)
    got["total"] = np.nextafter(got["total"], np.inf)
    rejected(got, truth, bound, a, k, "ascending order")
    with pytest.raises(AssertionError, match="total"):
        oc.certify_total(got["total"] * (1 + 1e-9), truth, bound, a, k)
