"""The sharded certificate (tests/shard_cases.py) without a GPU: the layouts reach the edges they name, the inputs are what the cases
say, every certificate passes on the reference alone (fp64 products rounded to fp32; the CPU oracle's k-means, cut into the layout's
shards; the oracle's and the restated eigensolver) and fails on a wrong rule: a shard's Z left out of the sum, last_md = 0, a rank's
centroid sums counted twice, a shard's place among B's columns counting dropped documents, one slice's rows left unorthogonalised."""
import numpy as np
import pytest

import gram_certificate as gc
import kmeans_certificate as kc
import ks_certificate as ksc
import shard_cases as sc

LAYOUTS = ("L2", "L3", "L4", "LP")


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts and inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_tile_the_documents(layout):
    case = sc.gram_case(layout, "rowconst")
    for D, bnd in ((case["D"], case["bounds"]),) + (((sc.KM_D, sc.bounds(layout, sc.KM_D)),) if layout in sc.KM_LAYOUTS else ()):
        assert len(bnd) == sc.WORLD[layout] + 1 and bnd[0] == 0 and bnd[-1] == D and np.all(np.diff(bnd) >= 0)
        rk = sc.rank_of_doc(bnd, np.arange(D))
        assert np.array_equal(np.bincount(rk, minlength=sc.WORLD[layout]), np.diff(bnd))
        assert all(bnd[r] <= d < bnd[r + 1] for d, r in zip(range(D), rk))
    n = np.diff(case["bounds"])
    if layout == "L2":
        assert n[0] == n[1] + 1
    if layout == "L3":
        assert list(n) == [1, case["D"] - 1, 0]
    if layout == "L4":
        assert n[0] == 0 and n[2] == 0 and n[1] > 0 and n[3] > 0


def test_the_planner_itself_makes_empty_shards():
    assert list(sc.plan_shards_py([0, 1, 2, 1000, 1001, 1002], 4)) == [0, 3, 3, 3, 5]  # the header's example
    case = sc.gram_case("LP", "rowconst")
    offs = case["offs"]
    assert offs[3] - offs[2] > 0.75 * offs[-1]
    assert list(case["bounds"]) == [0, 3, 3, 3, case["D"]]
    try:
        from isle_amd import HotPath
        assert list(HotPath.plan_shards(offs, 4).astype(np.int64)) == list(case["bounds"])
        rng = np.random.default_rng(0)
        for parts in (1, 2, 3, 4, 7):
            o = np.concatenate([[0], np.cumsum(rng.integers(0, 50, 200))])
            assert list(HotPath.plan_shards(o, parts).astype(np.int64)) == list(sc.plan_shards_py(o, parts))
    except OSError:
        pass  # the library is not built: the restatement stands alone


@pytest.mark.parametrize("layout", LAYOUTS)
def test_patterns_hold_a_word_on_one_rank_only_and_a_word_on_none(layout):
    case = sc.gram_case(layout, "rowconst")
    occ = sc.words_of_ranks(case)
    assert (occ.sum(axis=1) == 1).any() and (occ.sum(axis=1) == 0).any() and (occ.sum(axis=1) >= 2).any()
    assert occ[gc.GL_RB:].any()  # the second band's one row is not empty
    assert case["V"] == gc.GL_RB + 1 and case["D"] % 2 == 1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_values_are_row_constant_where_the_case_says(layout):
    for kind in sc.GRAM_KINDS:
        case = sc.gram_case(layout, kind)
        per_rank = [sc.row_constant(*sc.shard(case, case["bounds"], r)[:2], case["V"]) for r in range(case["world"])]
        whole = sc.row_constant(case["vals"], case["rows"], case["V"])
        if kind in ("rowconst", "sqrt"):
            assert whole and all(per_rank)
        elif kind == "perrank":
            assert all(per_rank) and not whole
        else:
            assert [not p for p in per_rank] == [r == case["special"] for r in range(case["world"])]
        if kind != "sqrt":
            assert set(np.unique(case["vals"])) <= set(np.float32(gc.DYADIC_S))


# ---------------------------------------------------------------------------------------------------------------------------------
# Gram apply
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", sc.GRAM_KINDS)
def test_gram_certificate_on_the_reference_alone(layout, kind):
    case = sc.gram_case(layout, kind)
    res = sc.certify_gram_case(case, sc.gram_reference_ranks(case))
    assert res["max_ratio_over_coeff"] <= 0.5 / (1 + 2)  # one rounding of the fp64 product: half an ulp against a coefficient of 3 or more


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["rowconst", "sqrt"])
def test_a_shard_left_out_of_the_sum_is_caught(layout, kind):
    case = sc.gram_case(layout, kind)
    r = int(np.flatnonzero(np.diff(case["bounds"]) > 0)[0])  # the first rank that holds a document (on L3: the one-document shard)
    with pytest.raises(AssertionError, match="bit-equal|outside the fp32 bound"):
        sc.certify_gram_case(case, sc.gram_reference_ranks(case, leave_out=r))


def test_ranks_that_differ_in_one_bit_or_in_the_form_are_caught():
    case = sc.gram_case("L2", "rowconst")
    ranks = [dict(q) for q in sc.gram_reference_ranks(case)]
    ranks[1]["g_rowconst_form"] = np.array([0])
    with pytest.raises(AssertionError, match="forms differ"):
        sc.certify_gram_case(case, ranks)
    ranks = [dict(q) for q in sc.gram_reference_ranks(case)]
    Z = ranks[1]["g_rowconst_b11"].copy()
    Z[-1, -1] = np.nextafter(Z[-1, -1], np.float32(np.inf))
    ranks[1]["g_rowconst_b11"] = Z
    with pytest.raises(AssertionError, match="differs between rank 0 and rank 1"):
        sc.certify_gram_case(case, ranks)


def test_the_all_reduce_term_widens_the_bound_by_its_roundings_only():
    case = sc.gram_case("L4", "sqrt")
    Z64, M, B = gc.gram64(case["V"], case["vals"], case["rows"], case["offs"], case["X"][10])
    coeff = gc.bound_coeff(B)
    w = int(np.argmax(np.where(M[:, 0] > 0, 1.0 / np.maximum(coeff, 1), 0)))
    Z = Z64.astype(np.float32)
    Z[w, 0] = np.float32(Z64[w, 0] + (coeff[w] + 2) * gc.U_F32 * M[w, 0])
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        gc.certify_gram(Z, Z64, M, B)
    gc.certify_gram(Z, Z64, M, B, extra=3)
    empty = np.flatnonzero(coeff == 0)
    Z[empty[0], 0] = 1e-30  # an empty row stays exactly zero whatever the term
    with pytest.raises(AssertionError):
        gc.certify_gram(Z, Z64, M, B, extra=3)


# ---------------------------------------------------------------------------------------------------------------------------------
# k-means
# ---------------------------------------------------------------------------------------------------------------------------------
def split(ranks, bnd, key, a):
    for r, q in enumerate(ranks):
        q[key] = a[int(bnd[r]):int(bnd[r + 1])]


def replicate(ranks, key, a):
    for q in ranks:
        q[key] = a


def kmpp_reference_ranks(c, layout, last_md_zero=False):
    """k-means++ with injected seeds from fp64 alone: every product and distance rounded to fp32 once.  last_md_zero: the residual of a
    run whose last rank reports 0 as the last document's distance (the whole sum is returned)."""
    k, bnd = c.k, sc.bounds(layout, sc.KM_D)
    ranks = [dict() for _ in range(sc.WORLD[layout])]
    seeds = c.seeds.astype(np.int64)
    sched = sc.kmpp_schedule(k)
    folded = seeds[:k - min(sched[-1], k - 1 - sum(sched[:-1]))]
    Ps = c.P64[folded]
    d = np.maximum(c.pn2[:, None] + np.einsum("ij,ij->i", Ps, Ps)[None, :] - 2.0 * (c.P64 @ Ps.T), 0.0).min(axis=1)
    md = d.astype(np.float32)
    replicate(ranks, "pp%d_seeds" % k, c.seeds)
    replicate(ranks, "pp%d_C" % k, (c.B["X"][:, seeds].T.toarray() @ c.U.astype(np.float64)).astype(np.float32))
    total = md.astype(np.float64).sum()
    replicate(ranks, "pp%d_res" % k, np.array([np.float32(total if last_md_zero else total - float(md[-1]))], np.float64))
    replicate(ranks, "pp%d_rounds" % k, np.array([len(sched)]))
    split(ranks, bnd, "pp%d_md" % k, md)
    return ranks, d


@pytest.mark.parametrize("k", sc.KM_KS)
def test_kmeanspp_residual_on_the_reference_alone_and_with_last_md_zero(k):
    c = sc.km_ref(True, k)
    assert c.seeds.max() < sc.KM_D - 1 and len(np.unique(c.seeds)) == k
    for layout in sc.KM_LAYOUTS:
        ranks, d = kmpp_reference_ranks(c, layout)
        assert d[-1] >= 0.25 * d.sum(), (d[-1], d.sum())  # the outlier: a wrong last distance cannot hide inside the allowance
        res = sc.certify_kmpp_injected(c, ranks)
        assert res["ratio"] < 0.01
        with pytest.raises(AssertionError, match="residual"):
            sc.certify_kmpp_injected(c, kmpp_reference_ranks(c, layout, last_md_zero=True)[0])


def test_kmeanspp_schedule_reaches_a_round_of_more_than_16_dice_at_300_only():
    assert max(sc.kmpp_schedule(300)) > 16 and max(sc.kmpp_schedule(65)) <= 16 and max(sc.kmpp_schedule(9)) <= 16
    assert sum(sc.kmpp_schedule(300)[:-1]) < 299 <= sum(sc.kmpp_schedule(300))
    assert 300 > 224  # the tracked rounds and the tile bounds of Lloyd in span(U)


@pytest.fixture(scope="module")
def oracle_runs():
    """The CPU oracle's k-means on the whole row-constant corpus, once per k: k-means++ with the injected seeds, both Lloyd loops with
    max_reps = 1 .. KM_REPS, from the seeds and from the degenerate start."""
    from oracle.oracle import OracleCsc, lift
    B = sc.km_corpus(False)
    o = OracleCsc(B["V"], B["D"], B["vals"], B["rows"], B["offs"])
    out = {}
    for k in sc.KM_KS:
        c = sc.km_ref(False, k)
        g = o.kmeanspp(c.U, k, inject=c.seeds)
        run = dict(C0=g["C_lowd"])
        for tag, C0 in (("lp%d" % k, g["C_lowd"]), ("dg%d" % k, sc.degenerate_start(c))):
            run[tag] = [o.lloyds_projected(c.U, C0, max_reps=r) for r in range(1, sc.KM_REPS + 1)]
        run["lift"] = lift(c.U, run["lp%d" % k][-1]["C_lowd"])
        run["ls%d" % k] = [o.lloyds_sparse(run["lift"], max_reps=r) for r in range(1, sc.KM_REPS + 1)]
        out[k] = run
    return out


def lloyd_reference_ranks(run, k, layout):
    bnd = sc.bounds(layout, sc.KM_D)
    ranks = [dict() for _ in range(sc.WORLD[layout])]
    for tag in ("lp%d" % k, "dg%d" % k, "ls%d" % k):
        for r, res in enumerate(run[tag], 1):
            split(ranks, bnd, "%s_r%d_assign" % (tag, r), res["assign"])
            replicate(ranks, "%s_r%d_it" % (tag, r), np.array([res["iters"]]))
            if tag.startswith("ls"):
                replicate(ranks, "%s_r%d_cen" % (tag, r), res["centers"])
            else:
                replicate(ranks, "%s_r%d_C" % (tag, r), res["C_lowd"])
    replicate(ranks, "ls%d_lift" % k, run["lift"])
    return ranks


@pytest.mark.parametrize("k", sc.KM_KS)
def test_lloyd_certificates_on_the_oracle_cut_into_shards(oracle_runs, k):
    c, run = sc.km_ref(False, k), oracle_runs[k]
    for layout in sc.KM_LAYOUTS:
        ranks = lloyd_reference_ranks(run, k, layout)
        sc.certify_projected(c, ranks, "lp%d" % k, run["C0"])
        dg = sc.certify_projected(c, ranks, "dg%d" % k, sc.degenerate_start(c), near_ties=True)
        assert dg["empty"] >= 2  # the far-off centres: clusters empty on every rank
        a1 = dg["runs"][0]["assign"]
        assert not np.isin(a1, [5, 6, k - 2, k - 1]).any() and (a1 == 1).any()
        # the oracle's sequential float sums of a row-constant B: the level FLOAT_SUMS_ROW_CONSTANT_FROB is taken from
        sc.certify_sparse(c, ranks, "ls%d" % k, run["lp%d" % k][-1]["C_lowd"], reproducible=True, frob_tol=kc.FLOAT_SUMS_ROW_CONSTANT_FROB)
    # L3 holds every document but the first on one rank: every cluster without document 0 has all its members on one rank
    a = run["lp%d" % k][0]["assign"]
    assert len(np.unique(a[1:])) > 1


@pytest.mark.parametrize("layout", sc.KM_LAYOUTS)
def test_a_ranks_centroid_sums_counted_twice_are_caught(oracle_runs, layout):
    k = 9
    c, run = sc.km_ref(False, k), oracle_runs[k]
    bnd = sc.bounds(layout, sc.KM_D)
    ranks = [dict(q) for q in lloyd_reference_ranks(run, k, layout)]
    a = run["lp%d" % k][0]["assign"].astype(np.int64)
    r = int(np.flatnonzero(np.diff(bnd) > 0)[0])  # on L3: the one-document shard, the smallest double count there is
    S = np.zeros((k, k))
    np.add.at(S, a, c.P64)
    np.add.at(S, a[bnd[r]:bnd[r + 1]], c.P64[bnd[r]:bnd[r + 1]])
    n = np.bincount(a, minlength=k)
    bad = (S / np.maximum(n, 1)[:, None]).astype(np.float32)
    for q in ranks:
        q["lp%d_r1_C" % k] = bad
    with pytest.raises(AssertionError, match="fp64 mean"):
        sc.certify_projected(c, ranks, "lp%d" % k, run["C0"])


def test_assignments_put_side_by_side_in_the_wrong_order_are_caught(oracle_runs):
    k = 9
    c, run = sc.km_ref(False, k), oracle_runs[k]
    ranks = lloyd_reference_ranks(run, k, "L2")
    with pytest.raises(AssertionError):
        sc.certify_projected(c, ranks[::-1], "lp%d" % k, run["C0"])


# ---------------------------------------------------------------------------------------------------------------------------------
# thresholding
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sc.TH_LAYOUTS)
def test_a_shard_with_documents_loses_them_all_to_the_threshold(layout):
    A, full = sc.th_corpus(), sc.th_reference(False)
    bnd = sc.bounds(layout, A["D"])
    kept = full["kept"]
    assert full["avg"] < sc.TH_FLAT_WORDS / 2  # avg / 1000 rounds to 0
    gone = [r for r in range(sc.WORLD[layout]) if bnd[r + 1] > bnd[r] and not kept[bnd[r]:bnd[r + 1]].any()]
    assert gone == ([0] if layout == "L3" else [1])
    assert full["D"] == sc.TH_REGULAR and np.asarray(full["original_cols"]).min() == sc.TH_FLAT
    for sampled in (False, True):
        want, tag = sc.th_reference(sampled), "ths" if sampled else "th"
        got = sc.certify_threshold(want, bnd, sc.threshold_reference_ranks(want, bnd, tag), tag)
        assert sum(got) == want["D"] and got[gone[0]] == 0
        with pytest.raises(AssertionError, match="doc_offset"):
            sc.certify_threshold(want, bnd, sc.threshold_reference_ranks(want, bnd, tag, count_dropped=True), tag)
    assert 0 < sc.th_reference(True)["D"] < full["D"]


# ---------------------------------------------------------------------------------------------------------------------------------
# Krylov-Schur
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.KS_CASES))
def test_row_slices_are_the_tables(name):
    c = sc.KS_CASES[name]
    assert [sc.ks_row_slice_py(c["V"], sc.WORLD[name], r) for r in range(sc.WORLD[name])] == c["slices"]
    assert all(r0 % 4 == 0 for r0, r1 in c["slices"] if r1 > r0)  # 16-byte aligned starts


def test_row_slices_by_the_host_program():
    """A second witness: the host program ks_host_main prints ks_row_slice of the header itself."""
    import os
    import subprocess
    exe = os.path.join(sc.ROOT, "isle_amd", "host", "ks_host_main")
    assert os.path.exists(exe), "build() makes isle_amd/host/ks_host_main (isle_amd/csrc/Makefile)"
    import json
    for name, c in sc.KS_CASES.items():  # the program reads its commands from standard input
        out = subprocess.run([exe], input="slice %d %d\n" % (c["V"], sc.WORLD[name]), capture_output=True, text=True, timeout=30)
        assert out.returncode == 0, out.stderr
        got = json.loads(out.stdout.strip().split("\n")[0])["slices"]  # [nloc, r0, r1] per rank
        assert [(r0, r1) for _, r0, r1 in got] == c["slices"], (name, got)


def test_every_ks_case_reaches_the_kernel_forms_of_its_row():
    def forms(name):
        return {(nl, m >= 64, r["vtf"], r["vtf_rows"], r["vtf_aligned"], r["update"]) for nl, m, r in sc.ks_routes(sc.ks_case(name))}
    f = forms("slice-empty")  # zero-row slice, ragged slice, plain kernels only
    assert {x[0] for x in f} == {12, 9, 0} and {(x[2], x[5]) for x in f if x[0]} == {("valu", "valu")} and {(x[2], x[5]) for x in f if not x[0]} == {("none", "none")}
    f = forms("ld-odd")  # update_k strided at every m; vtf_mfma_k off its float4 path once m >= 64, its row chunk halved twice
    assert sc.KS_CASES["ld-odd"]["V"] & 3
    assert {x[5] for x in f} == {"valu"} and {x[2] for x in f if x[1]} == {"mfma"} and {x[2] for x in f if not x[1]} == {"valu"}
    assert {(x[3], x[4]) for x in f if x[2] == "mfma"} == {(256, False)} and {x[0] for x in f} == {260, 246}
    f = forms("ld-even")  # update_mfma_k strided from m = 32 on, 16-byte aligned at every r0; ragged last slice
    assert sc.KS_CASES["ld-even"]["V"] & 3 == 0
    assert "mfma" in {x[5] for x in f} and {x[0] for x in f} == {344, 340} and {x[4] for x in f if x[2] == "mfma"} == {True}
    for name in sc.KS_CASES:  # the replicated step takes ld = n
        c = sc.ks_case(name)
        assert ksc.route(c["V"], ksc.effective_blk(c["nev"], c["blk"]), 64)["update"] == ("mfma" if c["V"] % 4 == 0 else "valu")


def oracle_ks(c):
    from oracle.oracle import OracleCsc
    B = c["B"]
    o = OracleCsc(B["V"], B["D"], B["vals"], B["rows"], B["offs"])
    return o.block_ks(c["nev"], blk=c["blk"], ncv=c["ncv"], maxit=sc.KS_MAXIT, tol=sc.KS_TOL, seed=sc.KS_SEED)


def ks_ranks(c, r):
    return [dict(ks_counts=np.array([r.get("rc", 0), r["nconv"], r["restarts"], r["napplies"]], np.int64), ks_evals=np.asarray(r["evals"], np.float32),
                 ks_U=np.asarray(r["U"], np.float32))] * c["world"]


@pytest.mark.parametrize("name", sorted(sc.KS_CASES))
def test_ks_spectrum_gap_oracle_convergence_and_certificate_on_the_oracle(name):
    c = sc.ks_case(name)
    lam, b = c["lam"][:c["nev"] + 1], sc.ks_residual_bound(c)
    # separated: every gap among the leading nev + 1 eigenvalues is more than twice the two residual bounds beside it, so that intervals
    # within the bound are disjoint and hold one eigenvalue each
    assert np.all(lam[:-1] - lam[1:] > 2 * (b[:-1] + b[1:])), ((lam[:-1] - lam[1:]) / (b[:-1] + b[1:])).min()
    r = oracle_ks(c)
    assert r["rc"] == 0 and r["nconv"] == c["nev"] and r["restarts"] < sc.KS_MAXIT
    res = sc.certify_ks(c, ks_ranks(c, r), "ks")
    assert max(res["residual"], res["orth"], res["rayleigh"]) <= 1.0


@pytest.mark.parametrize("name", ["slice-empty", "ld-odd"])
def test_a_slice_left_unorthogonalised_is_caught(name):
    """The restated loop in float32 on the dense B B^T passes the certificate; with the rows of one rank's slice left out of every update
    of the panel it does not."""
    c = sc.ks_case(name)
    b = ksc.effective_blk(c["nev"], c["blk"])
    S = np.random.default_rng(5).uniform(size=(c["V"], b)).astype(np.float32)
    args = (c["A64"], S, c["nev"], c["blk"], c["ncv"], sc.KS_MAXIT, sc.KS_TOL, np.float32)
    good = ksc.reference_run(*args)
    assert good["nconv"] == c["nev"] and good["restarts"] < sc.KS_MAXIT
    sc.certify_ks(c, ks_ranks(c, good), "ks")
    r0, r1 = [s for s in c["slices"] if s[1] > s[0]][-1]  # the last slice that holds a row: the ragged one
    bad = ksc.reference_run(*args, wrong={"skip_slice": (r0, r1)})
    with pytest.raises(AssertionError):
        sc.certify_ks(c, ks_ranks(c, bad), "ks")
