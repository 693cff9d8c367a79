"""The inference certificate (tests/infer_certificate.py) tested without a GPU: the fp32 CPU restatement and two numpy fp32 emulations
of the step (sequential sums; a pairwise tree with four partial gradients, as in the kernels) pass it on the GPU test's cases, every
mutant of the emulation is rejected by the certificate that covers it, plan_lf classifies hand-built documents, and at most 5 % of the
documents of every GPU case are left out."""
import ctypes as C

import numpy as np
import pytest

import infer_certificate as ic
from infer_certificate import (BORDERLINE, SURE_FINITE, SURE_OVERFLOW, case_id, certify_llh, certify_prefix, certify_step, certify_top,
                               classify_guess, emulate_llh, emulate_step, emulate_top, eta64, gpu_cases, left_out, make_case, plan_lf)

F = np.float32


def _doc(case, n):
    d = [i for i, r in enumerate(case["kept"]) if len(r) == n][0]
    return d, case["M"][case["kept"][d]], case["a"][d]


def _trajectory(R, a, k, Lf, its, tree):
    ws = [np.full(k, F(1) / F(k), F)]
    for it in range(its):
        ws.append(emulate_step(R, a, ws[-1], it, Lf, tree=tree))
    return ws


# ---- what must pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", gpu_cases(), ids=case_id)
def test_at_most_five_percent_of_every_gpu_case_is_left_out(kw):
    case = make_case(**kw)
    out, some = left_out(case)
    assert some >= len(ic.KEPT_COUNTS) and out <= ic.MAX_LEFT_OUT * some, "%d of %d documents are not eligible" % (out, some)
    ns = {len(r) for r in case["kept"]}
    assert set(ic.KEPT_COUNTS) <= ns and len(case["kept"]) % 4 != 0
    assert any(len(r) == 0 and w > 0 for r, w in zip(case["kept"], case["words"]))  # every word absent from the model
    if kw.get("cap") in ("16", "512"):
        eff = min(int(kw["cap"]), ic.lds_cap_rows(kw["k"]))
        assert {eff - 1, eff, eff + 1} <= ns
    if kw.get("Lf", 10.0) < 1:
        assert sum(p is not None and p > 1.5 * float(F(kw["Lf"])) for p in case["plan"]) >= 5  # documents that double once or more


def test_the_cases_reach_every_instantiation_and_boundary():
    ks = {kw["k"] for kw in gpu_cases()}
    assert set(ic.K_VALUES) <= ks
    assert {ic.instantiation(k) for k in ic.K_PER_FORM} == {ic.instantiation(k) for k in range(1, 1025)} and len(ic.K_PER_FORM) == 5
    for lo in (64, 128, 256, 512):
        assert ic.instantiation(lo) != ic.instantiation(lo + 1) and {lo, lo + 1} <= ks
    assert ic.lds_cap_rows(1024) == 34 and ic.V_DEFAULT % 4 != 0


@pytest.mark.parametrize("kw", gpu_cases(), ids=case_id)
def test_the_fp32_cpu_restatement_passes_on_the_gpu_cases(kw):
    try:
        from oracle import oracle
        oracle.lib()
    except Exception as e:  # no compiler on this machine
        pytest.skip("the oracle library cannot be built here: %s" % e)
    case = make_case(**kw)
    k = case["k"]
    runs = [None]
    for j in range(1, case["J"] + 1):
        o = oracle.infer(case["M"], case["offs"], case["rows"], case["counts"], iters=j, Lf=case["Lf"])
        assert o["avg_doc_sz"] == case["avg"]
        o["top_topic"], o["top_weight"] = emulate_top(o["weights"], k)
        runs.append(o)
    res = certify_prefix(case, runs)
    assert res["certified"] > 0 and res["w_ratio"] <= 1 and res["llh_ratio"] <= 1


@pytest.mark.parametrize("tree", [False, True], ids=["sequential", "tree"])
@pytest.mark.parametrize("k,n", [(3, 5), (7, 13), (65, 33), (200, 17), (300, 257), (700, 32)])
def test_the_numpy_emulations_pass(k, n, tree):
    case = make_case(k=k)
    d, R, a = _doc(case, n)
    Lf = case["plan"][d]
    assert Lf is not None
    ws = _trajectory(R, a, k, Lf, 6, tree)
    worst = 0.0
    for it in range(6):
        worst = max(worst, certify_step(R, a, ws[it], ws[it + 1], it, Lf)["max_ratio"])
        certify_llh(R, a, ws[it + 1], case["words"][d], case["avg"], emulate_llh(R, a, ws[it + 1], case["words"][d], case["avg"], tree))
    assert 0 < worst <= 1


# ---- what must be rejected --------------------------------------------------------------------------------------------------------
STEP_MUTANTS = [
    ("last_row", 7, 13, 2), ("last_row", 300, 513, 2), ("row_4_mod_8", 7, 13, 2), ("a_not_normalised", 7, 13, 2), ("eta_it", 7, 13, 2),
    ("log_k_plus_1", 3, 13, 2), ("partial_not_added", 7, 13, 2), ("normaliser_share", 7, 13, 2), ("normaliser_share", 700, 33, 2),
    ("stale_weights", 7, 13, 2), ("padded_topic", 7, 13, 2), ("padded_topic", 1023, 17, 2), ("small_topic_scaled", 30, 13, 0),
]


@pytest.mark.parametrize("tree", [False, True], ids=["sequential", "tree"])
@pytest.mark.parametrize("mutant,k,n,it", STEP_MUTANTS)
def test_every_mutant_of_the_step_is_rejected(mutant, k, n, it, tree):
    # far smaller weights than the largest one: the first step under a doubled Lf (ic.LF_CASES), where the weights collapse
    case = make_case(**(ic.LF_CASES[0] if mutant == "small_topic_scaled" else dict(k=k)))
    assert case["k"] == k
    d, R, a = _doc(case, n)
    Lf = case["plan"][d]
    ws = _trajectory(R, a, k, Lf, it + 1, tree)
    certify_step(R, a, ws[it], ws[it + 1], it, Lf)
    bad = emulate_step(R, a, ws[it], it, Lf, tree=tree, mutant=mutant, w_stale=ws[it - 1])
    if mutant == "small_topic_scaled":  # the max-norm check of test_gpu_infer.py accepts this one
        assert np.max(np.abs(bad - ws[it + 1])) / ws[it + 1].max() <= 2e-4
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        certify_step(R, a, ws[it], bad, it, Lf)


def test_swapped_llh_scales_are_rejected():
    case = make_case(k=7)
    d, R, a = _doc(case, 13)
    w = _trajectory(R, a, 7, 10.0, 3, False)[-1]
    words, avg = case["words"][d], case["avg"]
    assert words != avg
    certify_llh(R, a, w, words, avg, emulate_llh(R, a, w, words, avg))
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        certify_llh(R, a, w, words, avg, emulate_llh(R, a, w, words, avg, mutant="llh_swapped"))
    with pytest.raises(AssertionError, match="outside the fp32 bound"):  # a row left out of the sum
        certify_llh(R, a, w, words, avg, emulate_llh(R[:-1], a[:-1], w, words, avg))


def test_a_term_with_z_near_one_is_covered_by_the_absolute_part():
    # one row equal to 1 in every topic: z = sum w ~ 1, log z ~ 0 and of either sign in fp32
    k = 8
    R = np.ones((1, k), F)
    a = np.array([1.0])
    for w in (np.full(k, 0.125, F), np.full(k, 0.125, F) * (1 + F(2.0 ** -22)), np.full(k, 0.125, F) * (1 - F(2.0 ** -22))):
        certify_llh(R, a, w, 1, 1.0, emulate_llh(R, a, w, 1, 1.0))
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        certify_llh(R, a, np.full(k, 0.125, F), 1, 1.0, np.array([1e-5, 1e-5], F))


@pytest.mark.parametrize("mutant", ["top_tie_high", "top_ge", "top_wrong_weight"])
def test_every_mutant_of_the_top_five_is_rejected(mutant):
    k = 8
    u = F(1) / F(k)
    W = np.array([[u, u, 0.3, 0.3, 0.05, 0.05, 0.025, 0.025],
                  [0.2, 0.15, 0.15, 0.14, 0.13, 0.13, 0.05, 0.05],
                  [u] * 8], F)
    certify_top(W, k, *emulate_top(W, k))
    assert (emulate_top(W, k)[0][2] == -1).all() and list(emulate_top(W, k)[0][0]) == [2, 3, -1, -1, -1]
    with pytest.raises(AssertionError, match="the weights give"):
        certify_top(W, k, *emulate_top(W, k, mutant=mutant))


def test_an_unconverged_document_must_be_uniform():
    k = 4
    W = np.array([[0.25, 0.25, 0.25, 0.25], [0.7, 0.1, 0.1, 0.1]], F)
    tt, tw = emulate_top(W, k)
    certify_top(W, k, tt, tw, llh=np.array([[0, 0], [-1, -2]], F))
    with pytest.raises(AssertionError, match="did not converge"):
        certify_top(W, k, tt, tw, llh=np.array([[0, 0], [0, 0]], F))


# ---- plan_lf ----------------------------------------------------------------------------------------------------------------------
def test_plan_lf_on_hand_built_documents():
    k = 4
    a = np.array([1.0])
    flat = np.full((1, k), 0.25, F)       # g = 1 for every topic: finite at any sensible Lf
    assert classify_guess(flat, a, k, 10.0, 15) == SURE_FINITE and plan_lf(flat, a, k, 10.0) == 10.0
    peak = np.array([[1, 0, 0, 0]], F)    # from uniform z = 1/4 and g_0 = 4: e_0 = 4 eta
    e1 = 4 * eta64(k, 0, 1.0)             # e_0 at Lf = 1
    assert classify_guess(peak, a, k, 0.01, 15) == SURE_OVERFLOW
    lf = float(F(0.01))
    assert [classify_guess(peak, a, k, lf * 2 ** g, 15) for g in range(4)] == [SURE_OVERFLOW] * 3 + [SURE_FINITE]
    assert plan_lf(peak, a, k, 0.01) == float(F(lf * 8))
    edge = float(F(e1 / (ic.LOG_FLT_MAX + np.log(4.0))))  # log w_0 + e_0 = log(FLT_MAX): neither sure
    assert classify_guess(peak, a, k, edge, 15) == BORDERLINE and plan_lf(peak, a, k, edge) is None
    assert plan_lf(peak, a, k, edge / 2) is None              # the guess after a sure overflow is borderline: left out
    assert classify_guess(peak, a, k, edge * 1.01, 15) == SURE_FINITE and classify_guess(peak, a, k, edge / 1.01, 15) == SURE_OVERFLOW
    assert plan_lf(peak, a, k, 1e-9) is None                  # ten guesses are not enough
    # z below the floor: not certifiable, left out
    assert classify_guess(np.array([[1e-35, 0, 0, 0]], F), a, k, 10.0, 15) == BORDERLINE


# ---- coverage guard ---------------------------------------------------------------------------------------------------------------
def test_infer_reads_no_switch_but_the_one_the_gpu_test_sweeps():
    import isle_amd
    lib = isle_amd.load_library()
    names = []
    for i in range(lib.isle_hip_switch_info(-1, None, None, None)):
        s = C.c_char_p()
        lib.isle_hip_switch_info(i, C.byref(s), None, None)
        names.append(s.value.decode())
    assert ic.infer_switches_read(names) == ic.INFER_SWITCHES
