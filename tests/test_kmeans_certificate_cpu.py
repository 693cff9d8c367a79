"""The fp64 certificates of tests/kmeans_certificate.py must bite: the fp32 CPU oracle's Lloyd trajectories pass them, and every fault
planted into those trajectories (a document moved to a worse centre, a twin's documents given to the higher label, one centre entry off
by 1e-4, an empty cluster's centre left standing, one lift entry perturbed in a tail row or column) fails them.  The near-tie allowance
for starts on documents is shown to be needed by the oracle itself, and not to let a document beyond E through.  No GPU."""
import numpy as np
import pytest

from kmeans_certificate import (ISLE_SLACK_REL, certify_assignment, certify_centroids, certify_gemm, csc_points,
                                fp64_distances_argmin)

K = 10


@pytest.fixture(scope="module")
def case():
    from oracle.oracle import OracleCsc, lift
    from tools.synth import make_B
    B = make_B(2003, 4000, K, 1)
    D = min(B["D"], 3999)  # not a multiple of 64
    B = dict(V=B["V"], D=D, vals=B["vals"][:B["offs"][D]], rows=B["rows"][:B["offs"][D]], offs=B["offs"][:D + 1].copy())
    o = OracleCsc(B["V"], D, B["vals"], B["rows"], B["offs"])
    rng = np.random.default_rng(4)
    U = np.asfortranarray(np.linalg.qr(rng.standard_normal((B["V"], K)))[0].astype(np.float32))
    X = csc_points(B)
    P64 = np.asarray((X.T @ U.astype(np.float64)))
    Pabs = np.asarray(abs(X).T @ np.abs(U.astype(np.float64)))
    seeds = np.sort(rng.choice(D, K, replace=False)).astype(np.uint64)
    C0 = o.kmeanspp(U, K, inject=seeds)["C_lowd"]
    proj = [o.lloyds_projected(U, C0, max_reps=r) for r in (1, 2, 3)]
    cen0 = lift(U, proj[-1]["C_lowd"])
    sparse = [o.lloyds_sparse(cen0, max_reps=r) for r in (1, 2, 3)]
    return dict(B=B, o=o, U=U, X=X, P64=P64, Pabs=Pabs, C0=C0, proj=proj, cen0=cen0, sparse=sparse, lift=lift)


def test_oracle_trajectories_pass(case):
    """Iteration r of a run with max_reps = r was computed against the centres of the run with max_reps = r - 1 (the prefix method)."""
    P64, proj = case["P64"], case["proj"]
    starts = [case["C0"]] + [p["C_lowd"] for p in proj[:-1]]
    for r, (p, c_in) in enumerate(zip(proj, starts), 1):
        assert p["iters"] == r
        certify_assignment(P64, None, c_in, p["assign"])
        certify_centroids(P64, p["assign"], [q["assign"] for q in proj[:r - 1]], p["C_lowd"], X_abs=case["Pabs"])
    X, sparse = case["X"], case["sparse"]
    starts = [case["cen0"]] + [s["centers"] for s in sparse[:-1]]
    for r, (s, c_in) in enumerate(zip(sparse, starts), 1):
        certify_assignment(X, None, np.asarray(c_in).T, s["assign"])
        certify_centroids(X, s["assign"], [q["assign"] for q in sparse[:r - 1]], s["centers"].T)


def test_slack_is_the_header_value():
    assert ISLE_SLACK_REL == np.float32(1e-4)


def test_a_document_moved_to_a_worse_centre_is_caught(case):
    P64, p, C = case["P64"], case["proj"][1], case["proj"][0]["C_lowd"]
    dist, xn2, cn2 = fp64_distances_argmin(P64, C)
    order = np.argsort(dist, axis=1)
    rows = np.arange(dist.shape[0])
    best, second = order[:, 0], order[:, 1]
    gap = dist[rows, second] - dist[rows, best]
    E2 = ISLE_SLACK_REL * (2 * xn2 + cn2[best] + cn2[second])
    cand = np.flatnonzero((gap > 1.5 * E2) & (p["assign"] == best))
    d = int(cand[np.argmin(gap[cand] / E2[cand])])  # the hardest such document: the gap just above the slack
    bad = p["assign"].copy()
    bad[d] = second[d]
    with pytest.raises(AssertionError, match="gap"):
        certify_assignment(P64, None, C, bad)


def test_a_twin_labelled_with_the_higher_index_is_caught(case):
    P64 = case["P64"]
    C = case["proj"][1]["C_lowd"].copy()
    C[7] = C[3]  # bit-identical twins 3 < 7
    dist, _, _ = fp64_distances_argmin(P64, C)
    assign = np.argmin(dist, axis=1).astype(np.uint32)
    certify_assignment(P64, None, C, assign)
    d = int(np.flatnonzero(assign == 3)[0])
    assign[d] = 7  # the same fp64 distance: only the tie rule can see it
    with pytest.raises(AssertionError, match="bit-identical"):
        certify_assignment(P64, None, C, assign)


def test_one_centre_entry_off_by_1e_4_is_caught(case):
    X, s = case["X"], case["sparse"][0]
    C = s["centers"].T.copy()
    n = np.bincount(s["assign"], minlength=K)
    c = int(np.argmin(np.where(n > 0, n, 1 << 30)))  # the smallest cluster: n_c + 2 well below 1e4
    j = int(np.argmax(C[c]))
    C[c, j] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError, match="fp64 mean"):
        certify_centroids(X, s["assign"], [], C)


def test_an_empty_cluster_left_at_its_old_centre_is_caught(case):
    o, U, P64 = case["o"], case["U"], case["P64"]
    C0 = case["C0"].copy()
    C0[5] = 1e3 * np.abs(C0).max()  # far from every document: its cluster is empty from the first step on
    p = o.lloyds_projected(U, C0, max_reps=1)
    assert not (p["assign"] == 5).any()
    certify_centroids(P64, p["assign"], [], p["C_lowd"], X_abs=case["Pabs"])
    assert not p["C_lowd"][5].any()
    bad = p["C_lowd"].copy()
    bad[5] = C0[5]
    with pytest.raises(AssertionError, match="not exactly zero"):
        certify_centroids(P64, p["assign"], [], bad, X_abs=case["Pabs"])


@pytest.mark.parametrize("where", ["row", "col"])
def test_a_perturbed_lift_entry_is_caught(case, where):
    U, Cl = case["U"], case["proj"][-1]["C_lowd"]
    out = case["lift"](U, Cl)  # (V, K): U Cl^T
    certify_gemm(U, Cl.T, out)
    bad = out.copy()
    i, j = (bad.shape[0] - 1, 4) if where == "row" else (1234, bad.shape[1] - 1)
    bound = (K + 2) * 2.0 ** -24 * float(np.abs(U[i].astype(np.float64)) @ np.abs(Cl[j].astype(np.float64)))
    bad[i, j] = np.float32(bad[i, j] + 3 * bound)
    with pytest.raises(AssertionError, match="entry"):
        certify_gemm(U, Cl.T, bad)


def test_starts_on_documents_need_the_near_tie_allowance():
    """Centres placed on documents of a row-constant B: distances are short sums of a few distinct values and many documents sit at a
    near-exact tie, which fp32 breaks either way.  The fp32 oracle's first assignment is off the fp64 arg-min on more documents than
    max(3, 3e-4 D) allows, every gap within E; near_ties admits those, and a document moved beyond E is still caught."""
    from oracle.oracle import OracleCsc
    from tools.synth import make_B
    B = make_B(2003, 6100, 20, 3)
    D = 6001
    B = dict(V=B["V"], D=D, vals=B["vals"][:B["offs"][D]], rows=B["rows"][:B["offs"][D]], offs=B["offs"][:D + 1].copy())
    X = csc_points(B)
    o = OracleCsc(B["V"], D, B["vals"], B["rows"], B["offs"])
    seeds = np.sort(np.random.default_rng(1).choice(D, 7, replace=False))
    docs = np.asfortranarray(X[:, seeds].toarray().astype(np.float32))
    a = o.lloyds_sparse(docs, max_reps=1)["assign"]
    dist, xn2, cn2 = fp64_distances_argmin(X, docs.T)
    best = np.argmin(dist, axis=1)
    assert (a != best).sum() > 3
    with pytest.raises(AssertionError, match="off the fp64 arg-min"):
        certify_assignment(X, None, docs.T, a)
    certify_assignment(X, None, docs.T, a, near_ties=True)
    order = np.argsort(dist, axis=1)
    rows = np.arange(D)
    gap = dist[rows, order[:, 1]] - dist[rows, order[:, 0]]
    E2 = ISLE_SLACK_REL * (2 * xn2 + cn2[order[:, 0]] + cn2[order[:, 1]])
    d = int(np.flatnonzero((gap > 1.5 * E2) & (a == best))[0])
    bad = a.copy()
    bad[d] = order[d, 1]
    with pytest.raises(AssertionError, match="gap"):
        certify_assignment(X, None, docs.T, bad, near_ties=True)


def test_float_sums_of_a_row_constant_B_stay_above_1e_6():
    """The reference's own sequential fp32 centroid sums on a row-constant B (a centre entry is a sum of n_c copies of one value) miss the
    fp64 means by more than 1e-6 in Frobenius relative error, within the per-entry bound: the typical-level bound the GPU test holds the
    library's float sums of such a B to (test_gpu_kmeans_certified.FLOAT_SUMS_ROW_CONSTANT_FROB = 4e-6) is this level with a margin."""
    from oracle.oracle import OracleCsc
    from tools.synth import make_B
    B = make_B(2003, 6100, 20, 3)
    D = 6001
    B = dict(V=B["V"], D=D, vals=B["vals"][:B["offs"][D]], rows=B["rows"][:B["offs"][D]], offs=B["offs"][:D + 1].copy())
    X = csc_points(B)
    o = OracleCsc(B["V"], D, B["vals"], B["rows"], B["offs"])
    docs = np.asfortranarray(X[:, np.sort(np.random.default_rng(2).choice(D, 9, replace=False))].toarray().astype(np.float32))
    s = o.lloyds_sparse(docs, max_reps=1)
    with pytest.raises(AssertionError, match="Frobenius"):
        certify_centroids(X, s["assign"], [], s["centers"].T)
    res = certify_centroids(X, s["assign"], [], s["centers"].T, frob_tol=4e-6)
    assert 1e-6 < res["frob"] < 2e-6
