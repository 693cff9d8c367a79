"""The sharded path (N ranks on one GPU over the host-staged transport) certified against fp64 at shard edges: an unequal split, a
one-document shard, empty first / middle / last shards, the planner's own empty shards (tests/shard_cases.py).  Each layout's worker
runs once per module; the tests certify the arrays it stored, on the host.  A launch that fails fails that layout's tests and ends the
launches: nothing more is started on the GPU behind a fault, an abort or a time limit."""
from functools import partial

import numpy as np
import pytest

import kmeans_certificate as kc
import shard_cases as sc
from rank_launch import launch_each, ranks_of, write_report

pytestmark = pytest.mark.gpu

LAYOUTS = ("L2", "L3", "L4", "LP")
REPORT = []  # (case, quantity, error / bound)

_FAILED = []  # the first launch of this module that failed: nothing is started behind it, by either fixture


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """layout -> its launch: Gram apply, thresholding and k-means on the layout's shards."""
    tmp = str(tmp_path_factory.mktemp("shards"))
    return launch_each([(layout, layout, partial(sc.launch, layout, tmp)) for layout in LAYOUTS], _FAILED)


@pytest.fixture(scope="module")
def ks_launches(tmp_path_factory):
    """(case, tag) -> its launch: the sparse entry of the eigensolver on an even split of the documents."""
    tmp = str(tmp_path_factory.mktemp("shards_ks"))
    return launch_each([((name, tag), "%s-%s" % (name, tag), partial(sc.launch, name, tmp, env=env, tag="-" + tag)) for name, tag, env in sc.KS_RUNS], _FAILED)


@pytest.fixture(scope="module", autouse=True)
def report(launches, ks_launches):
    """At the end of the module: the launch times and the largest error / bound of every quantity, printed (shown with -s or on a
    failure) and written to the file ISLE_SHARD_REPORT names."""
    yield
    lines = ["shard certificate, launch %s: %.1f s" % ("-".join(name) if isinstance(name, tuple) else name, l["wall"])
             for name, l in list(launches.items()) + list(ks_launches.items()) if isinstance(l, dict)]
    lines += ["shard certificate, %s: %s %.3g" % r for r in REPORT]
    write_report(lines, "ISLE_SHARD_REPORT")


@pytest.mark.parametrize("kind", sc.GRAM_KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gram_apply(launches, hp, layout, kind):
    """Z = B (B^T X) all-reduced over the shards, b in {1, 10, 11, 25, 32}, V = 4079 (two bands, the second of one row): bit-identical on
    all ranks, one operator form on all ranks, bit-equal to fp64 on dyadic inputs and within (n_w + max n_d + 2 + N - 1) u M otherwise."""
    case = sc.gram_case(layout, kind)
    res = sc.certify_gram_case(case, ranks_of(launches, layout))
    if kind == "sqrt":
        REPORT.append(("%s Gram apply" % layout, "max |err| / (coeff u M)", res["max_ratio_over_coeff"]))
    if kind == "perrank" and layout == "L2":
        # shards that are each row-constant keep the banded form with per-rank scales; one rank holding the same matrix does not
        assert res["forms"] == [1, 1]
        hp.upload_csc(case["V"], case["vals"], case["rows"], case["offs"])
        hp.gram_apply(case["X"][1])
        assert hp.operator_form() == 0


@pytest.mark.parametrize("k", sc.KM_KS)
@pytest.mark.parametrize("layout", sc.KM_LAYOUTS)
def test_kmeanspp_injected_seeds_and_residual(launches, layout, k):
    """C_lowd = P[seeds], min_dist of every document, and the returned residual against the fp64 sum of the certified distances of
    documents 0 .. D - 2 (the last document is an outlier that holds a quarter of the total or more)."""
    res = sc.certify_kmpp_injected(sc.km_ref(True, k), ranks_of(launches, layout))
    REPORT.append(("%s k-means++ k=%d" % (layout, k), "|residual - fp64| / sum E", res["ratio"]))


@pytest.mark.parametrize("k", sc.KM_KS)
@pytest.mark.parametrize("layout", sc.KM_LAYOUTS)
def test_kmeanspp_free_running(launches, layout, k):
    """Seeds distinct, below D and equal on all ranks; C_lowd = P[seeds]; at k = 300 the schedule holds rounds of more than 16 dice
    (k_search instead of k_search_args)."""
    res = sc.certify_kmpp_free(sc.km_ref(True, k), ranks_of(launches, layout))
    assert res["wide_round"] == (k == 300)
    REPORT.append(("%s free k-means++ k=%d" % (layout, k), "C_lowd error / bound", res["gemm_ratio"]))


@pytest.mark.parametrize("k", sc.KM_KS)
@pytest.mark.parametrize("layout", sc.KM_LAYOUTS)
def test_lloyd_in_span_U(launches, layout, k):
    """Every document at every iteration (prefix method), from the k-means++ centres and from the degenerate start (twins, a zero centre,
    centres on documents, two clusters empty on every rank); the replicated centres bit-identical on all ranks."""
    ranks, c = ranks_of(launches, layout), sc.km_ref(False, k)
    C0 = sc.same_on_all_ranks(ranks, "c0_%d" % k)
    a = sc.certify_projected(c, ranks, "lp%d" % k, C0)
    b = sc.certify_projected(c, ranks, "dg%d" % k, sc.degenerate_start(c), near_ties=True)
    assert b["empty"] >= 2
    a1 = b["runs"][0]["assign"]
    assert not np.isin(a1, [5, 6, k - 2, k - 1]).any() and (a1 == 1).any()
    REPORT.append(("%s Lloyd in span(U) k=%d" % (layout, k), "gap / (E(c) + E(c*))", max(a["max_ratio"], b["max_ratio"])))
    REPORT.append(("%s Lloyd in span(U) k=%d" % (layout, k), "centre error / bound", max(a["cen_ratio"], b["cen_ratio"])))


@pytest.mark.parametrize("k", sc.KM_KS)
@pytest.mark.parametrize("layout", sc.KM_LAYOUTS)
def test_lloyd_on_B(launches, layout, k):
    """From the lifted centres of the last run in span(U).  The banded form (L2: integer centroid counts) is reproducible bit for bit; the
    gather form the ranks agree on when a shard is empty sums floats (kmeans_certificate.FLOAT_SUMS_ROW_CONSTANT_FROB)."""
    ranks, c = ranks_of(launches, layout), sc.km_ref(False, k)
    form = int(sc.same_on_all_ranks(ranks, "km_form").ravel()[0])
    if not sc.has_empty_shard(sc.bounds(layout, sc.KM_D)):
        assert form == 1
    last = sc.same_on_all_ranks(ranks, "lp%d_r%d_C" % (k, sc.KM_REPS))
    s = sc.certify_sparse(c, ranks, "ls%d" % k, last, reproducible=form == 1, frob_tol=1e-6 if form == 1 else kc.FLOAT_SUMS_ROW_CONSTANT_FROB)
    REPORT.append(("%s Lloyd on B k=%d" % (layout, k), "gap / (E(c) + E(c*))", s["max_ratio"]))
    REPORT.append(("%s Lloyd on B k=%d" % (layout, k), "centre error / bound", s["cen_ratio"]))


def test_first_assignment_from_the_tracked_rounds_on_two_ranks(launches):
    """k = 300 on L2: Lloyd in span(U) starts from the nearest seeds and tile minima the k-means++ rounds kept on each rank."""
    ranks, k = ranks_of(launches, "L2"), sc.KM_KS[-1]
    c = sc.km_ref(False, k)
    for o in launches["L2"]["outputs"]:
        assert o.count("first assignment taken from the k-means++ rounds") == sc.KM_REPS, o[-2000:]
        assert "[tile bounds, projected]" in o
    res = sc.certify_projected(c, ranks, "tk%d" % k, sc.same_on_all_ranks(ranks, "tk%d_c0" % k))
    REPORT.append(("L2 tracked rounds k=%d" % k, "gap / (E(c) + E(c*))", res["max_ratio"]))


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("layout", sc.TH_LAYOUTS)
def test_thresholding(launches, layout, sampled):
    """upload_counts + threshold on shards one of which (D > 0) loses every document to the rule: the shards' B side by side is the
    restated single-rank B bit for bit, with and without sampling, and doc_offset / D_global tile its columns."""
    A = sc.th_corpus()
    bnd = sc.bounds(layout, A["D"])
    kept = sc.certify_threshold(sc.th_reference(sampled), bnd, ranks_of(launches, layout), "ths" if sampled else "th")
    assert any(k == 0 and bnd[r + 1] > bnd[r] for r, k in enumerate(kept)), kept  # a shard with documents and no column of B


@pytest.mark.parametrize("name,tag", [(n, t) for n, t, _ in sc.KS_RUNS])
def test_krylov_schur_sparse_entry(ks_launches, name, tag):
    """The eigensolver on B B^T over the shards, with the orthogonalisation sharded by rows (zero-row, ragged and unaligned slices) and
    replicated: replicated results bit-identical on all ranks, residual enclosure of the leading nev eigenvalues of the fp64 B B^T, the
    solver's residual test, orthonormality and Rayleigh quotients within the bounds of ks_certificate."""
    res = sc.certify_ks(sc.ks_case(name), ranks_of(ks_launches, (name, tag)), "ks")
    for q in ("residual", "orth", "rayleigh"):
        REPORT.append(("Krylov-Schur %s (%s, %d restarts)" % (name, tag, res["restarts"]), "%s / bound" % q, res[q]))
