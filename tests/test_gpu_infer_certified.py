"""Every step of isle_hip_infer certified topic by topic against fp64 (tests/infer_certificate.py), in every instantiation of the two
kernel templates, on every boundary of k_infer's dispatch and under every value of ISLE_INFER_CAP_ROWS.

The prefix method: the kernels have no floating-point atomics and add in fixed order, so a run with iters = j - 1 returns exactly the
weights that iteration j of a longer run starts from.  hp.infer runs with iters = 1 .. J; w_j is certified against the fp64 step from
the fp32 w_{j-1} (w_0 uniform), and the llh and the top five at every j.  The repeat-call test asserts that reproducibility directly.
The Lipschitz guess of every document is planned from the fp64 trajectory alone (plan_lf); at most 5 % of a case's documents may be
left out as borderline, which test_infer_certificate_cpu.py asserts for every case here before any GPU time is spent.

At the end of the module the largest error / bound per instantiation is printed (profiles/infer_certificate.md holds a measured run)."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import infer_certificate as ic
from infer_certificate import CAP_VALUES, K_PER_FORM, LF_CASES, K_VALUES, case_id, certify_prefix, instantiation, left_out, make_case

pytestmark = pytest.mark.gpu

STATS = {}  # instantiation -> dict(w_ratio, llh_ratio, certified, left_out)
_RAN = set()  # the k of every default-form case certified so far
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def certificate_summary():
    """At the end of the module: per instantiation the largest error / bound of the weights and of the llh, the documents certified and
    the documents left out, printed (shown with -s or -rA) and, with INFER_CERT_REPORT=<path>, written there as JSON."""
    yield STATS
    wall = time.time() - _T0
    for name, s in sorted(STATS.items()):
        print("infer certificate, %s: weights error / bound %.3g, llh error / bound %.3g, %d documents certified, %d left out"
              % (name, s["w_ratio"], s["llh_ratio"], s["certified"], s["left_out"]))
    print("infer certificate: %.1f s" % wall)
    path = os.environ.get("INFER_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(STATS, wall_seconds=wall), f, indent=1, sort_keys=True)
    for s in STATS.values():
        assert s["w_ratio"] <= 1.0 and s["llh_ratio"] <= 1.0 and s["certified"] > 0
    if set(K_VALUES) <= _RAN:  # the whole sweep ran: it reached all five instantiations
        assert set(STATS) == {instantiation(k) for k in K_PER_FORM} and len(STATS) == 5


def _run(hp, case, iters, want_weights=True):
    return hp.infer(case["M"], case["offs"], case["rows"], case["counts"], iters=iters, Lf=case["Lf"], want_weights=want_weights)


def _certify(hp, kw):
    case = make_case(**kw)
    out, some = left_out(case)
    assert out <= ic.MAX_LEFT_OUT * some, "%d of %d documents are not eligible" % (out, some)
    runs = [None] + [_run(hp, case, j) for j in range(1, case["J"] + 1)]
    assert all(r["avg_doc_sz"] == case["avg"] for r in runs[1:])
    res = certify_prefix(case, runs, stats=STATS)
    assert res["certified"] >= some - out > 0 and res["w_ratio"] <= 1 and res["llh_ratio"] <= 1
    return case, res


def _same_bits(a, b, with_weights=True):
    for name in ("llh", "top_topic", "top_weight") + (("weights",) if with_weights else ()):
        x, y = a[name], b[name]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    assert a["nconverged"] == b["nconverged"]


# ---- reproducibility first: everything below depends on it -------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_PER_FORM)
def test_two_identical_calls_return_identical_bits(hp, k):
    case = make_case(k=k)
    for iters in (1, 7, case["J"]):
        _same_bits(_run(hp, case, iters), _run(hp, case, iters))


@pytest.mark.parametrize("k", K_PER_FORM)
def test_the_null_weights_pointer_changes_no_other_output(hp, k):
    case = make_case(k=k)
    for iters in (1, case["J"]):
        g = _run(hp, case, iters, want_weights=False)
        assert g["weights"] is None
        _same_bits(_run(hp, case, iters), g, with_weights=False)


# ---- every instantiation and every boundary of the dispatch ------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_VALUES)
def test_every_step_is_certified_at_every_form_boundary(hp, k):
    case, res = _certify(hp, dict(k=k))
    _RAN.add(k)
    if k == 1:  # log k = 0: eta = 0, the weight stays 1 and no topic exceeds 1 / k
        g = _run(hp, case, case["J"])
        for d, ids in enumerate(case["kept"]):
            if len(ids):
                assert g["weights"][d, 0] == 1 and (g["top_topic"][d] == -1).all() and g["llh"][d, 0] != 0


def test_more_than_1024_topics_are_refused_before_any_launch(hp):
    from isle_amd.hot_path import IsleHipError
    M = np.full((8, 1025), 1.0 / 8, np.float32)
    offs = np.array([0, 2], np.int64)
    with pytest.raises(IsleHipError, match=r"not in \[1, 1024\]"):
        hp.infer(M, offs, np.array([0, 1], np.uint32), np.ones(2, np.float32))
    _certify(hp, dict(k=3))  # the context is intact


@pytest.mark.parametrize("k", K_PER_FORM)
def test_exact_zeros_inside_kept_rows(hp, k):
    case, _ = _certify(hp, dict(k=k, kind="zeros"))
    # topics whose gradient is exactly zero: their weights only shrink with the normaliser, all by the same factor
    g = _run(hp, case, case["J"])
    d = [i for i, r in enumerate(case["kept"]) if len(r) == 33][0]
    dead = np.flatnonzero(~case["M"][case["kept"][d]].any(0))
    assert len(dead) >= 1 and len(set(g["weights"][d, dead].tolist())) == 1


# ---- ISLE_INFER_CAP_ROWS: rows staged in LDS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAP_VALUES)
@pytest.mark.parametrize("k", K_PER_FORM)
def test_every_step_is_certified_with_rows_staged_in_lds(hp, monkeypatch, k, cap):
    monkeypatch.setenv("ISLE_INFER_CAP_ROWS", cap)
    case, _ = _certify(hp, dict(k=k, cap=cap))
    # staging changes where the rows are read from, not one bit of the arithmetic
    g = _run(hp, case, case["J"])
    _same_bits(g, _run(hp, case, case["J"], want_weights=False), with_weights=False)
    monkeypatch.delenv("ISLE_INFER_CAP_ROWS")
    _same_bits(g, _run(hp, case, case["J"]))


def test_infer_reads_no_other_switch(hp):
    names = []
    for i in range(hp._lib.isle_hip_switch_info(-1, None, None, None)):
        s = C.c_char_p()
        hp._lib.isle_hip_switch_info(i, C.byref(s), None, None)
        names.append(s.value.decode())
    assert ic.infer_switches_read(names) == ic.INFER_SWITCHES == {"ISLE_INFER_CAP_ROWS"}


# ---- a Lipschitz guess that has to double ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", LF_CASES, ids=case_id)
def test_documents_whose_lipschitz_guess_doubles(hp, kw):
    # certified with the doubled Lf that plan_lf derives from the fp64 trajectory (why J = 1 with the peaked model: see LF_CASES)
    case, _ = _certify(hp, kw)
    lf0 = float(np.float32(1e-3))
    assert sum(p is not None and p > 1.5 * lf0 for p in case["plan"]) >= 5

