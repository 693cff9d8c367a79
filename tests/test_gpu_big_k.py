"""GPU parity at the topic counts the BASELINE configs use: k = 200 (configs[1]) and k = 1000 (configs[2..4]), with the
reference's ncv = 2k + 10 = 410 / 2010 (include/hyperparams.h:38-40, block-ks/restarted_block_ks.h:138-187).

These sizes select code that k <= 50 never reaches: the small EVD at n = 400 / 2000 in its persistent form (td_persist_k), the
projected assignment's chunked path (ldk > 256), the first word-space assignment through the projection (k <= 384) or through
the sparse product (k > 384), Yinyang bounds with 25 / 125 centre groups, k-means++ with 27 / 60 rounds.

Held to tests/golden/big_<case>.npz (tests/golden/make_golden_big.py): the reference's own Spectra solver run in the build
container, and fp64 NumPy mathematics (dense eigh, brute-force k-means by SURVEY App. B's statement).  Everything in the
fixture is invariant under a change of basis of span(U), so the HIP path is checked with ITS OWN eigenvectors; the tolerances
are the contract's (sigma 1e-4 relative) or a stated multiple of what the fp32 CPU restatement achieved against the same
fixture (recorded in it as oracle_*).  A second leg compares with the CPU oracle run here on the HIP path's U (same-input
parity: iteration counts equal, partitions >= 99.9 %).
"""
import os

import numpy as np
import pytest

from conftest import corpus, upload

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIGMA_TOL = 1e-4  # BASELINE.json north_star: top-k singular values within 1e-4 relative error


def load_case(name):
    f = np.load(os.path.join(GOLD, "big_%s.npz" % name))
    V, D, k, seed, sr = (int(x) for x in f["params"])
    B = corpus(V, D, k, seed, sample_rate=sr / 1000.0)
    sig = np.array([B["V"], B["D"], B["nnz"], int(B["rows"].astype(np.int64).sum())], np.int64)
    assert np.array_equal(sig, f["sig"]), "the generator no longer produces the corpus the fixture was made from"
    return f, B, k


@pytest.fixture(scope="module", params=["c2k200", "c3k1000", "c4k1000s"])
def solved(request, hp):
    """One eigensolve + the whole k-means chain per case, shared by the asserts below."""
    f, B, k = load_case(request.param)
    upload(hp, B)
    r = hp.compute_block_ks(k, allow_noconv=True)
    U = hp.get_U(k)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    md = hp.get_min_dist()
    lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
    hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
    ls = hp.run_lloyds(k)
    return dict(name=request.param, f=f, B=B, k=k, r=r, U=U, g=g, md=md, lp=lp, ls=ls)


def test_sigma_against_fp64_and_the_reference_solver(solved):
    f, k, r = solved["f"], solved["k"], solved["r"]
    assert r["rc"] == 0 and r["nconv"] == k
    sig = np.sqrt(r["evals"].astype(np.float64))
    truth = np.sqrt(f["truth_evalues"][:k])
    assert np.max(np.abs(sig - truth) / truth) <= SIGMA_TOL
    # the reference's Spectra solver (fp32, ncv = 2k + 1) is itself this far from the fp64 spectrum — 2e-5 at k = 200, 1.3e-4 at k = 1000
    ref = np.sqrt(f["spectra_evalues"].astype(np.float64))
    assert np.max(np.abs(sig - ref) / ref) <= SIGMA_TOL + float(f["spectra_sigma_err_vs_truth"])
    # same restart schedule as the restated reference algorithm (the start block differs: one restart of slack)
    assert abs(r["restarts"] - int(f["oracle_restarts_napplies"][0])) <= 1


def test_eigenvectors_span_the_true_subspace(solved):
    f, k, U = solved["f"], solved["k"], solved["U"].astype(np.float64)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 5e-5
    R = np.random.default_rng(12345).standard_normal((U.shape[0], 8))  # SKETCH_SEED / SKETCH_COLS of the generator
    err = np.linalg.norm(U @ (U.T @ R) - f["sketch"]) / np.linalg.norm(f["sketch"])
    # the boundary pair sigma_k / sigma_k+1 is 1e-3 .. 1e-4 apart: the fp32 CPU restatement reaches oracle_sketch_err
    assert err <= max(10.0 * float(f["oracle_sketch_err"]), 1e-3), (err, float(f["oracle_sketch_err"]))


def test_kmeanspp_min_distances(solved):
    f, md = solved["f"], solved["md"]
    idx = f["min_d2_idx"]
    scale = f["min_d2_val"].max()
    assert np.abs(md[idx] - f["min_d2_val"]).max() <= max(10.0 * float(f["oracle_min_d2_err"]), 1e-4) * scale
    assert abs(md.astype(np.float64).sum() - float(f["min_d2_sum"])) <= 1e-3 * float(f["min_d2_sum"])


def test_partitions_against_fp64_brute_force(solved):
    """Lloyd in span(U) and on B from the injected seeds against brute-force fp64 k-means with the true eigenvectors."""
    f, k, lp, ls = solved["f"], solved["k"], solved["lp"], solved["ls"]
    oa = f["oracle_agreement"]
    a_p = float((lp["assign"] == f["lp_assign"]).mean())
    a_w = float((ls["assign"] == f["ls_assign"]).mean())
    # fp32 rounding moves documents that sit between two centres; the CPU restatement agrees to oracle_agreement (>= 0.9998)
    assert a_p >= min(0.995, oa[0] - 0.003), (a_p, oa)
    assert a_w >= min(0.995, oa[1] - 0.003), (a_w, oa)
    if abs(oa[0] - 1.0) < 2e-3 and int(f["oracle_iters"][0]) == int(f["lp_iters"]):
        assert lp["iters"] == int(f["lp_iters"])
    if abs(oa[1] - 1.0) < 2e-3 and int(f["oracle_iters"][1]) == int(f["ls_iters"]):
        assert ls["iters"] == int(f["ls_iters"])
    assert np.bincount(ls["assign"], minlength=k).sum() == solved["B"]["D"]  # src/trainer.cpp:567-570
    cn = np.sqrt((ls["centers"].astype(np.float64) ** 2).sum(0))
    big = f["ls_cnorm"] > 1e-3 * f["ls_cnorm"].max()
    assert np.median(np.abs(cn[big] - f["ls_cnorm"][big]) / f["ls_cnorm"][big]) <= 1e-3


def test_same_input_parity_with_the_cpu_oracle(solved, hp):
    """The oracle run here on the HIP path's U and the same injected seeds: every stage compared on identical inputs."""
    from oracle.oracle import lift
    f, B, k, U = solved["f"], solved["B"], solved["k"], solved["U"]
    o = B["oracle"]
    ko = o.kmeanspp(U, k, inject=f["seeds"])
    assert ko["rounds"] == solved["g"]["rounds"]
    assert np.abs(solved["md"] - ko["min_dist"]).max() <= 1e-4 * ko["min_dist"].max()
    scale = np.abs(ko["C_lowd"]).max()
    assert np.abs(solved["g"]["C_lowd"] - ko["C_lowd"]).max() <= 1e-4 * scale
    lo = o.lloyds_projected(U, ko["C_lowd"])
    assert solved["lp"]["iters"] == lo["iters"]
    assert (solved["lp"]["assign"] == lo["assign"]).mean() >= 0.999
    # word space from the ORACLE's projected centres on both sides
    so = o.lloyds_sparse(lift(U, lo["C_lowd"]))
    upload(hp, B)
    hp.set_U(U)
    hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])  # materialises P for the k <= 384 first assignment
    hp.left_multiply_by_U(lo["C_lowd"], fetch=False)
    sg = hp.run_lloyds(k)
    assert sg["iters"] == so["iters"]
    assert (sg["assign"] == so["assign"]).mean() >= 0.999
    live = np.bincount(so["assign"], minlength=k) > 0
    num = np.linalg.norm((sg["centers"] - so["centers"])[:, live].astype(np.float64))
    assert num <= 1e-3 * np.linalg.norm(so["centers"][:, live].astype(np.float64))


def test_bound_modes_agree_at_k1000(hp, monkeypatch):
    """Exact accelerations: Yinyang (125 groups) / Hamerly / no bounds for Lloyd on B, tile bounds (32 tiles) / Hamerly / no bounds for
    Lloyd in span(U) — the same partition and iteration counts at k = 1000 in every mode."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    res = {}
    for mode in ("yinyang", "hamerly", "none"):  # projected loop: tile bounds (default at k > 224), Hamerly's single bound, none
        monkeypatch.setenv("ISLE_KMEANS_BOUNDS", mode)
        if mode == "hamerly":
            monkeypatch.setenv("ISLE_PROJ_BOUNDS", "hamerly")
        if mode == "none":
            monkeypatch.setenv("ISLE_NO_HAMERLY", "1")
        g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k, fetch_centers=False)
        res[mode] = (lp["assign"], lp["iters"], ls["assign"], ls["iters"])
    monkeypatch.delenv("ISLE_KMEANS_BOUNDS")
    monkeypatch.delenv("ISLE_NO_HAMERLY")
    monkeypatch.delenv("ISLE_PROJ_BOUNDS")
    for mode in ("hamerly", "none"):
        assert res[mode][1] == res["yinyang"][1] and res[mode][3] == res["yinyang"][3]
        assert np.array_equal(res[mode][0], res["yinyang"][0])
        assert np.array_equal(res[mode][2], res["yinyang"][2])


def test_grouped_projection_writes_give_the_same_projection(hp, monkeypatch):
    """Round 5: the panel passes of P = U^T B write their rows whole and in position order into slabs, sixteen panels at a time, and a second
    kernel assembles the document-major rows and their squared norms (k_gl_wide, gl_wide_assemble_k); ISLE_GL_WIDE_GROUPED=0 writes 40-byte
    pieces straight into P.  The accumulators are the same: the seeds' coordinates (rows of P) must be bit-equal, the k-means++ distances
    (which use the norms, summed in another order) equal to rounding, and the partitions of Lloyd in span(U) equal up to near-ties
    (src/sparseMatrix.cpp:1749-1791)."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, seed=2, allow_noconv=True)
    U = hp.get_U(k)
    res = {}
    for name, env in (("grouped", {}), ("direct", {"ISLE_GL_WIDE_GROUPED": "0"})):
        for a, b in env.items():
            monkeypatch.setenv(a, b)
        hp.set_U(U)  # invalidates the projection
        g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
        res[name] = (g, hp.get_min_dist(), hp.run_lloyds_on_projected_space(k, g["C_lowd"]))
        for a in env:
            monkeypatch.delenv(a)
    assert np.array_equal(res["grouped"][0]["C_lowd"].view(np.uint32), res["direct"][0]["C_lowd"].view(np.uint32))
    assert np.abs(res["grouped"][1] - res["direct"][1]).max() <= 1e-5 * res["direct"][1].max()
    assert res["grouped"][2]["iters"] == res["direct"][2]["iters"]
    assert (res["grouped"][2]["assign"] == res["direct"][2]["assign"]).mean() >= 0.9999


def test_lds_dma_assignment_product_gives_the_bits_of_the_register_staged_one(hp, monkeypatch):
    """Round 5: the two-term pass of the D x k x k assignment products reads the projection's pre-split copy (two bf16 terms per entry, laid out
    as the LDS image of every row block and slab) by LDS-DMA through a ring of stages (gemm_bf16x2_dma_k); ISLE_GEMM_DMA=0 splits on the fly
    and stages through registers (gemm_bf16x3_k).  The same products summed in the same order: partitions, iteration counts and centres of both
    Lloyd loops must be bit-equal (src/sparseMatrix.cpp:1794-1871, :1494-1572)."""
    f, B, k = load_case("c3k1000")
    res = {}
    for name, env in (("dma", {}), ("registers", {"ISLE_GEMM_DMA": "0"})):
        for a, b in env.items():
            monkeypatch.setenv(a, b)
        upload(hp, B)
        hp.compute_block_ks(k, seed=3, allow_noconv=True)
        monkeypatch.setenv("ISLE_KMPP_TRACK", "0")  # so that Lloyd in span(U) opens with a full product as well
        g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        monkeypatch.delenv("ISLE_KMPP_TRACK")
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k)
        res[name] = (lp, ls)
        for a in env:
            monkeypatch.delenv(a)
    for i in (0, 1):
        assert res["dma"][i]["iters"] == res["registers"][i]["iters"]
        assert np.array_equal(res["dma"][i]["assign"], res["registers"][i]["assign"])
    assert np.array_equal(res["dma"][0]["C_lowd"].view(np.uint32), res["registers"][0]["C_lowd"].view(np.uint32))
    assert np.array_equal(res["dma"][1]["centers"].view(np.uint32), res["registers"][1]["centers"].view(np.uint32))


def test_regrouped_yinyang_groups_give_the_same_partition(hp, monkeypatch):
    """Round 5: the Yinyang groups of the by-group iteration are formed from the centres in the order of their squared norms (slot tables,
    YyMap) instead of eight consecutive labels.  Bounds are bounds whichever centres share a group, labels and ties stay in the centres' own
    numbering: partition, iteration count and centres must equal the consecutive-label form's (ISLE_YY_REGROUP=0) bit for bit, and the
    no-bounds loop's partition (src/sparseMatrix.cpp:1587-1677)."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
    res = {}
    for name, env in (("regrouped", {}), ("consecutive", {"ISLE_YY_REGROUP": "0"}), ("two_launches", {"ISLE_YY_FUSED": "0"}),
                      ("none", {"ISLE_KMEANS_BOUNDS": "none"})):
        for a, b in env.items():
            monkeypatch.setenv(a, b)
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        res[name] = hp.run_lloyds(k)
        for a in env:
            monkeypatch.delenv(a)
    for name in ("consecutive", "two_launches"):
        assert res[name]["iters"] == res["regrouped"]["iters"]
        assert np.array_equal(res[name]["assign"], res["regrouped"]["assign"]), name
        assert np.array_equal(res[name]["centers"].view(np.uint32), res["regrouped"]["centers"].view(np.uint32)), name
    assert res["none"]["iters"] == res["regrouped"]["iters"]
    assert np.array_equal(res["none"]["assign"], res["regrouped"]["assign"])


def test_gather_form_runs_the_by_group_iteration_without_movers(hp, monkeypatch):
    """ISLE_GRAM_LDS=0 (or any matrix whose rows are not single-valued) has no LDS-banded stream for the movers' thin product: Lloyd on B
    at k >= 256 (by-group Yinyang iteration, fused filter) must run — round 4 failed there with "k_gl_thin needs the LDS-banded form" as
    soon as one centre's movement stood out — and give the partition of the LDS-banded form up to near-ties."""
    f, B, k = load_case("c3k1000")
    res = {}
    for form in ("1", "0"):
        monkeypatch.setenv("ISLE_GRAM_LDS", form)
        upload(hp, B)
        hp.compute_block_ks(k, allow_noconv=True)
        assert hp.operator_form() == int(form)
        g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k, fetch_centers=False)
        assert ls["iters"] >= 3  # several Yinyang iterations ran
        res[form] = (lp, ls)
    monkeypatch.delenv("ISLE_GRAM_LDS")
    upload(hp, B)  # leave the session's context in the default form
    assert (res["0"][0]["assign"] == res["1"][0]["assign"]).mean() >= 0.999
    assert (res["0"][1]["assign"] == res["1"][1]["assign"]).mean() >= 0.998


def test_fused_filter_and_tightening_give_the_bits_of_the_two_kernel_form(hp, monkeypatch):
    """The by-group Yinyang iteration lowers the group bounds and tightens the active documents in ONE launch (yy2_filter_tighten_k: the bounds
    stay in LDS between the two steps); ISLE_YY_FUSED=0 runs yy_filter_k and yy2_tighten_k as before.  Same arithmetic on the same values:
    partition, iteration count and centres must be bit-equal (Lloyd on B, src/sparseMatrix.cpp:1587-1677), also against the by-document form."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
    out = {}
    # (the fused launch visits the documents in their own order by default, the two-kernel form in the member lists'; ISLE_YY_ORDER forces either)
    for name, env in (("fused", {}), ("two", {"ISLE_YY_FUSED": "0"}), ("doc", {"ISLE_YY_MODE": "doc"}), ("fused_by_members", {"ISLE_YY_ORDER": "member"}),
                      ("two_in_document_order", {"ISLE_YY_FUSED": "0", "ISLE_YY_ORDER": "doc"})):
        for a, b in env.items():
            monkeypatch.setenv(a, b)
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        out[name] = hp.run_lloyds(k)
        for a in env:
            monkeypatch.delenv(a)
    for name in ("two", "doc", "fused_by_members", "two_in_document_order"):
        assert out[name]["iters"] == out["fused"]["iters"], name
        assert np.array_equal(out[name]["assign"], out["fused"]["assign"]), name
        assert np.array_equal(out[name]["centers"].view(np.uint32), out["fused"]["centers"].view(np.uint32)), name


def test_assignment_epilogues_inside_the_product_give_the_bits_of_the_two_kernel_route(hp, monkeypatch):
    """The two D x k x k assignment steps (full pass of Lloyd in span(U), first assignment of Lloyd on B through the projection:
    src/sparseMatrix.cpp:1794-1871, 1494-1572) form distances, tile / group bounds and the assignment INSIDE the matrix product's epilogue
    (gemm_bf16x3.h group epilogues + a pass over 16 candidates per document); ISLE_GEMM_EPILOGUE=0 writes the D x k product and runs
    proj_dots_tiles_k / dots_assign_cm_k over it.  Same dot products, same arithmetic: partitions, iteration counts, centres bit-equal."""
    from tools.synth import make_B
    V, D, k = 6000, 140_000, 1000  # 547 row blocks x 4 column tiles: the three-term bf16 product with 256 x 256 tiles is taken
    B = make_B(V, D, k, 77)
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, rng_seed=3)
    out = {}
    for name, env in (("fused", {"ISLE_KMPP_TRACK": "0"}), ("two", {"ISLE_KMPP_TRACK": "0", "ISLE_GEMM_EPILOGUE": "0"})):
        for a, b in env.items():
            monkeypatch.setenv(a, b)
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k)
        out[name] = (lp, ls)
        for a in env:
            monkeypatch.delenv(a)
    for i in (0, 1):
        assert out["fused"][i]["iters"] == out["two"][i]["iters"]
        assert np.array_equal(out["fused"][i]["assign"], out["two"][i]["assign"]), float((out["fused"][i]["assign"] == out["two"][i]["assign"]).mean())
    assert np.array_equal(out["fused"][0]["C_lowd"].view(np.uint32), out["two"][0]["C_lowd"].view(np.uint32))
    assert np.array_equal(out["fused"][1]["centers"].view(np.uint32), out["two"][1]["centers"].view(np.uint32))


def test_active_documents_ordered_by_their_tiles_give_the_same_bits(hp, monkeypatch):
    """Lloyd in span(U) with tile bounds orders the active documents of an iteration by the set of tiles they re-examine (pt_need_keys_k +
    radix sort), so that a workgroup's 128 documents ask for the same 2 - 3 tiles instead of 9 - 13 between them; ISLE_PT_SORT=0 keeps the
    member lists' order.  Every distance formed is exact and the order only changes which bounds happen to be tightened on the way:
    partition, iteration count and centres bit-equal (src/sparseMatrix.cpp:1794-1871)."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    out = {}
    for name, env in (("sorted", {}), ("members", {"ISLE_PT_SORT": "0"}), ("members, fresh sums", {"ISLE_PT_SORT": "0", "ISLE_PROJ_SUMS": "fresh"}),
                      ("sorted, fresh sums", {"ISLE_PROJ_SUMS": "fresh"})):
        for a, b in env.items():
            monkeypatch.setenv(a, b)
        out[name] = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        for a in env:
            monkeypatch.delenv(a)
    for a, b in (("sorted", "members"), ("sorted, fresh sums", "members, fresh sums")):
        assert out[a]["iters"] == out[b]["iters"]
        assert np.array_equal(out[a]["assign"], out[b]["assign"])
        assert np.array_equal(out[a]["C_lowd"].view(np.uint32), out[b]["C_lowd"].view(np.uint32))


@pytest.mark.parametrize("case", ["c2k200", "c3k1000"])
def test_centroid_sums_kept_up_to_date_agree_with_fresh_sums(hp, monkeypatch, case):
    """After its first iteration Lloyd in span(U) brings the centroid sums up to date with the rows of the documents that changed centre
    (proj_changed_k, proj_delta_sum_k: sorted by centre, document and sign, summed in that order — no atomics) instead of summing all
    member rows again (src/sparseMatrix.cpp:1957-1992 sums them all; ISLE_PROJ_SUMS=fresh does).  The two associate the additions
    differently: centres equal to rounding, the same iteration count, partitions equal up to ties at rounding level — and the default is
    bitwise reproducible run after run, like the fresh sums."""
    f, B, k = load_case(case)
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    a1 = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
    a2 = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
    monkeypatch.setenv("ISLE_PROJ_SUMS", "fresh")
    fr = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
    monkeypatch.delenv("ISLE_PROJ_SUMS")
    assert np.array_equal(a1["C_lowd"].view(np.uint32), a2["C_lowd"].view(np.uint32)) and np.array_equal(a1["assign"], a2["assign"])
    assert a1["iters"] == fr["iters"]
    assert (a1["assign"] == fr["assign"]).mean() >= 1 - 1e-4
    assert np.abs(a1["C_lowd"] - fr["C_lowd"]).max() <= 1e-5 * np.abs(fr["C_lowd"]).max()


def test_two_term_assignment_products_give_the_three_term_assignment(hp, monkeypatch):
    """The two D x k x k assignment products run with TWO bf16 terms per operand first (three partial products instead of six); every
    distance is then within 8.2e-5 (|row|^2 + max |centre|^2) of the three-term value, bounds are widened by that much, and the rows whose
    two smallest distances are closer than twice that are run again through the three-term product (dense.hip gemm_assign_two_pass).
    ISLE_GEMM_TERMS=3 runs the three-term product alone.  Partitions, iteration counts and centres bit-equal in both loops
    (src/sparseMatrix.cpp:1794-1871, 1494-1572) — also when centres coincide, so that every document near them is left open."""
    from tools.synth import make_B
    V, D, k = 6000, 140_000, 1000
    B = make_B(V, D, k, 78)
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, rng_seed=5)
    twins = g["C_lowd"].copy()
    twins[1::2] = twins[0::2]  # every centre twice: the arg-min of every document is an exact tie: every row is left open
    for start in (g["C_lowd"], twins):
        out = {}
        for name, env in (("two", {"ISLE_KMPP_TRACK": "0"}), ("three", {"ISLE_KMPP_TRACK": "0", "ISLE_GEMM_TERMS": "3"})):
            for a, b in env.items():
                monkeypatch.setenv(a, b)
            lp = hp.run_lloyds_on_projected_space(k, start, max_reps=3)
            hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
            ls = hp.run_lloyds(k, max_reps=3)
            out[name] = (lp, ls)
            for a in env:
                monkeypatch.delenv(a)
        for i in (0, 1):
            assert out["two"][i]["iters"] == out["three"][i]["iters"]
            assert np.array_equal(out["two"][i]["assign"], out["three"][i]["assign"]), float((out["two"][i]["assign"] == out["three"][i]["assign"]).mean())
        assert np.array_equal(out["two"][0]["C_lowd"].view(np.uint32), out["three"][0]["C_lowd"].view(np.uint32))
        assert np.array_equal(out["two"][1]["centers"].view(np.uint32), out["three"][1]["centers"].view(np.uint32))


def test_full_tile_pass_by_library_gemm_equals_the_fused_kernel(hp, monkeypatch):
    """At large k the full passes of the projected Lloyd (iteration 0, and later iterations with more than half the documents
    active) are one library GEMM over the coordinate-major projection plus proj_dots_tiles_k; the fused matrix-core kernel
    (ISLE_PROJ_FULL=fused) forms the same distances in another summation order.  Both routes must give the same partition, the
    same iteration count and centres equal to rounding, here and in the sparse loop's first assignment (ISLE_FIRST_ASSIGN)."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    out = {}
    for route in ("gemm", "fused"):
        monkeypatch.setenv("ISLE_PROJ_FULL", route)
        monkeypatch.setenv("ISLE_FIRST_ASSIGN", "projection" if route == "gemm" else "sparse")
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k, fetch_centers=False)
        out[route] = (lp, ls)
    (lg, sg), (lf, sf) = out["gemm"], out["fused"]
    assert lg["iters"] == lf["iters"] and sg["iters"] == sf["iters"]
    assert (lg["assign"] == lf["assign"]).mean() >= 0.9999
    assert (sg["assign"] == sf["assign"]).mean() >= 0.9995
    assert np.abs(lg["C_lowd"] - lf["C_lowd"]).max() <= 1e-3 * np.abs(lf["C_lowd"]).max()


def test_assignment_products_on_the_bf16_matrix_cores_equal_the_f32_ones(hp, monkeypatch):
    """The two D x k x k dot-product matrices of the assignment steps (full pass of Lloyd in span(U), first assignment of Lloyd on B) run
    on the bf16 matrix cores with both operands split into three bf16 terms (gemm_bf16x3.h: the six partial products down to 2^-16 of
    the leading one, each exact, summed in f32); ISLE_GEMM_BF16X3=0 puts them back on the f32 MFMA (gemm_f32.h).  Same partition
    (near-ties apart), same iteration counts, centres equal to rounding — and both equal to the CPU oracle's."""
    f, B, k = load_case("c3k1000")
    upload(hp, B)
    hp.compute_block_ks(k, allow_noconv=True)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=f["seeds"])
    monkeypatch.setenv("ISLE_PROJ_FULL", "gemm")          # the small fixture would take the fused kernel
    monkeypatch.setenv("ISLE_FIRST_ASSIGN", "projection")
    out = {}
    for mode in ("bf16x3", "f32"):
        if mode == "f32":
            monkeypatch.setenv("ISLE_GEMM_BF16X3", "0")
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        ls = hp.run_lloyds(k)
        out[mode] = (lp, ls)
    (la, sa), (lb, sb) = out["bf16x3"], out["f32"]
    assert la["iters"] == lb["iters"] and sa["iters"] == sb["iters"]
    assert (la["assign"] == lb["assign"]).mean() >= 0.9999 and (sa["assign"] == sb["assign"]).mean() >= 0.9999
    assert np.abs(la["C_lowd"] - lb["C_lowd"]).max() <= 1e-4 * np.abs(lb["C_lowd"]).max()
    assert np.abs(sa["centers"] - sb["centers"]).max() <= 1e-4 * np.abs(sb["centers"]).max()


def test_config5_edge_topics_at_k1000(hp):
    """BASELINE.json configs[4]: edge_topics = 1, max_edge_topics = 5000 at k = 1000 — catchwords, topic model and edge topics
    on the device from the fixture's partition, against the CPU restatement (src/trainer.cpp:577-654, :1116-1167)."""
    from test_gpu_post import _check_all, _setup
    from oracle import oracle as O
    f, B, k = load_case("c3k1000")
    V, D, _, seed, _ = (int(x) for x in f["params"])
    s = _setup(hp, V, D, k, seed, assign_fn=lambda oc, c: f["ls_assign"].astype(np.uint32))
    assert np.array_equal(s["B"]["rows"], B["rows"]) and np.array_equal(s["B"]["offs"], B["offs"])  # device thresholding = the fixture's B
    r, rank_thr = O.catchword_rank(D, k), O.model_rank_threshold(D, k)
    assert r >= 1 and rank_thr >= 1
    got, tm, ref = _check_all(hp, s, V, D, k, r, rank_thr)
    pairs, edge = O.post_edge_topics(ref["model"], ref["top1"], ref["top2"], 5000)
    assert pairs.shape[0] >= 50
    E = hp.edge_topics(pairs[:, :2])
    ok = np.isfinite(edge)
    assert np.array_equal(np.isfinite(E), ok)
    np.testing.assert_allclose(E[ok], edge[ok], rtol=5e-5, atol=1e-9)  # model columns already differ by the summation order (2e-5)


def test_inference_at_k1000(hp):
    """ISLEInfer with 1000 topics takes the wave-per-row kernel (inf_docs_k; k <= 256 takes inf_docs16_k)."""
    from oracle import oracle as O
    from tools.synth import Corpus
    V, D, k = 3000, 1500, 1000
    c = Corpus(V, D, 20, 9)
    cnt, rows, offs = c.A()
    rng = np.random.default_rng(4)
    M = rng.gamma(0.3, size=(V, k)).astype(np.float32)
    M /= M.sum(0, keepdims=True)
    got = hp.infer(M, offs, rows, cnt)
    ref = O.infer(M, offs, rows, cnt, avg_doc_sz=got["avg_doc_sz"])
    conv = ref["llh"][:, 0] != 0
    assert got["nconverged"] == ref["nconverged"] and conv.sum() >= D // 2
    wmax = ref["weights"][conv].max(1, keepdims=True)
    assert np.abs(got["weights"][conv] - ref["weights"][conv]).max() <= 2e-4 * wmax.max()
    np.testing.assert_allclose(got["llh"][conv], ref["llh"][conv], rtol=2e-4, atol=1e-4)


def ritz_like(n, seed):
    """Spectrum of a Ritz matrix of this corpus family: one dominant value, a cluster with ~1e-3 relative gaps, a decaying tail."""
    rng = np.random.default_rng(seed)
    lam = np.concatenate([[50.0], 5.0 * (1.0 - 1e-3 * np.arange(n // 2 - 1)), 2.0 / (1.0 + 0.01 * np.arange(n - n // 2))])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return ((Q * lam) @ Q.T).astype(np.float32)


@pytest.mark.parametrize("n,env", [(400, None), (400, "ISLE_TD_CHAIN"), (2000, None), (2048, None), (2100, None)])
def test_small_evd_at_the_sizes_the_restarts_meet(hp, monkeypatch, n, env):
    """arma::eig_sym of truncate() (block-ks/restarted_block_ks.h:150-161) at n = 400 (k = 200) and n = 2000 (k = 1000): persistent
    tridiagonalisation; n = 400 with ISLE_TD_CHAIN and n = 2048: the launch chain; n = 2100: beyond the tridiagonal solver (Jacobi)."""
    if env:
        monkeypatch.setenv(env, "1")
    S = ritz_like(n, n)
    e, v = hp.eig_sym(S)
    er = np.linalg.eigvalsh(S.astype(np.float64))[::-1]
    scale = np.abs(er).max()
    assert np.abs(e - er).max() <= 2e-6 * scale
    v = v.astype(np.float64)
    assert np.abs(v.T @ v - np.eye(n)).max() <= 2e-5
    assert np.abs(S.astype(np.float64) @ v - v * e).max() <= 3e-5 * scale


@pytest.mark.parametrize("n", [400, 2000])
def test_the_three_grid_barriers_of_the_persistent_tridiagonalisation_give_the_same_bits(hp, monkeypatch, n):
    """td_persist_k crosses one grid barrier per column (gridbar.h): sharded counters polled together (default), the hierarchical form
    (ISLE_TD_BAR=hier), one counter (ISLE_TD_BAR=flat).  A barrier orders the same loads and stores in every form, so eigenvalues and
    eigenvectors must agree bit for bit — a form that let a workgroup through early would read a stale column and differ."""
    S = ritz_like(n, n + 1)
    e0, v0 = hp.eig_sym(S)
    assert hp.eig_info()["solver"] == "tridiagonal"
    for form in ("hier", "flat"):
        monkeypatch.setenv("ISLE_TD_BAR", form)
        e, v = hp.eig_sym(S)
        assert hp.eig_info()["solver"] == "tridiagonal", form  # three Jacobi answers would agree bit for bit as well
        monkeypatch.delenv("ISLE_TD_BAR")
        assert np.array_equal(e.view(np.uint32), e0.view(np.uint32)), form
        assert np.array_equal(v.view(np.uint32), v0.view(np.uint32)), form


@pytest.mark.parametrize("n", [399, 400, 1212, 2010])
def test_back_transformation_by_blocks_of_four_reflectors_equals_the_sequential_one(hp, monkeypatch, n):
    """The eigenvectors' back-transformation Z <- H_0 ... H_{n-3} Z runs by blocks of four reflectors in compact WY form (td_wy_T_k + td_back_wy_k:
    S = V^T Z, Y = T S, Z -= V Y; the block's reflector columns staged by LDS-DMA one block ahead when n is even); ISLE_TD_BACK=seq applies the
    reflectors one by one (td_back_k).  Same eigenvalues bit for bit (the back-transformation does not touch them), eigenvectors equal to
    rounding, both orthonormal and both satisfying S v = lambda v.  n = 399: the element-wise path and a last block of one reflector;
    n = 2010 with all vectors: 503 workgroups, two rounds; n = 1212: rows per thread that do not fill the unrolled eight."""
    S = ritz_like(n, n + 7)
    e1, v1 = hp.eig_sym(S)
    i1 = hp.eig_info()
    monkeypatch.setenv("ISLE_TD_BACK", "seq")
    e0, v0 = hp.eig_sym(S)
    i0 = hp.eig_info()
    monkeypatch.delenv("ISLE_TD_BACK")
    # the two back-transformations are compared only if the tridiagonal solver answered with each (two Jacobi answers would agree as well)
    assert i1["solver"] == i0["solver"] == "tridiagonal" and i1["td_back"] == "wy" and i0["td_back"] in ("seq8", "seq4")
    assert np.array_equal(e1.view(np.uint32), e0.view(np.uint32))
    assert np.abs(v1.astype(np.float64) - v0).max() <= 2e-6
    S64 = S.astype(np.float64)
    for v in (v1, v0):
        V = v.astype(np.float64)
        assert np.abs(V.T @ V - np.eye(n)).max() <= 2e-6
        assert np.abs(S64 @ V - V * e1.astype(np.float64)).max() <= 2e-6 * np.abs(e1).max()
