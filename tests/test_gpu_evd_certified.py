"""The small symmetric eigensolver (k_eig_small: evd_tridiag.hip, the block Jacobi solver of dense.hip) through isle_hip_eig_sym and
isle_hip_eig_sym_leading, against scipy's float64 eigh of the matrix the upper triangle of the same float32 input defines
(tests/evd_certificate.py): eigenvalues value by value, eigenvectors entry by entry after fixing the sign (per cluster the projector, where
multiplicities are exact), orthonormality over all pairs, the residual componentwise, each inside the fp32 rounding of the fp64 answer plus
C n 2^-53 ||S||_2 with C from the LAPACK drivers alone.  Which solver answered, in which form and with which back-transformation is read
from isle_hip_eig_info and asserted per case: a tridiagonal path that failed its own check and let the Jacobi solver answer does not pass.
The cases sit on the dispatch edges of both solvers; test_evd_certificate_cpu.py asserts without a GPU that each reaches its edge, that no
case sits near a decision, and that seven wrong rules fail these bounds.

A grid-barrier time-out of the persistent form is timing on a shared device, not numerics: where the record says that THIS solve gave up
at a barrier, the certificate is asserted for the launch chain that answered, the bail-out is printed and reported, only the form
assertion is waived, and the cases after it get a fresh context (the old one stays on the chain for good).

At the end of the module the largest error / bound per case and quantity, the solver record and the wall time are printed;
EVD_CERT_REPORT=<path> writes them as JSON (profiles/evd_certificate.md holds a measured run)."""
import json
import os
import time

import numpy as np
import pytest

import evd_certificate as ec

pytestmark = pytest.mark.gpu

STATS = {}
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def certificate_summary():
    yield STATS
    wall = time.time() - _T0
    for name, s in sorted(STATS.items()):
        print("evd certificate, %s: error / bound %s | %s" % (name, ", ".join("%s %.3g" % (q, s[q]) for q in ec.QUANTITIES), s["record"]))
    print("evd certificate: %.1f s" % wall)
    path = os.environ.get("EVD_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(STATS, wall_seconds=wall), f, indent=1, sort_keys=True)


class _Own:
    """A context of this module's own: another test's bail-out cannot move its cases to the launch chain."""

    def __init__(self):
        self.h = None

    def get(self):
        if self.h is None:
            from isle_amd import HotPath
            self.h = HotPath(0)
        return self.h

    def renew(self):
        if self.h is not None:
            self.h.close()
        self.h = None


@pytest.fixture(scope="module")
def own():
    o = _Own()
    yield o
    o.renew()


def _solve(own, monkeypatch, c):
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    h = own.get()
    e, V = h.eig_sym(ec.matrix(c["key"]), nvec=c["nvec"])
    info = h.eig_info()
    for k in c["env"]:
        monkeypatch.delenv(k)
    if info["td_bailed"]:
        print("%s: the persistent form gave up at a grid barrier in this solve; the launch chain answered (form assertion waived)" % c["name"])
        own.renew()
    return e, V, info


def _check(c, e, V, info, key=None):
    """Every figure is printed and kept before anything is asserted."""
    name, n, nvec, want = key or c["name"], c["n"], c["nvec"], c["expect"]
    solver = info["solver"] or want["solver"]
    r = ec.ratios(c["key"], e, V, solver, nvec)
    STATS[name] = dict(r, record=info)
    print("%s: %s | error / bound %s, tail as documented: %s" % (name, info, ", ".join("%s %.3g" % (q, r[q]) for q in ec.QUANTITIES), r["tail"]))
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(V))
    assert info["n"] == n and info["nvec"] == (n if nvec is None else nvec)
    assert info["solver"] == want["solver"], "the %s solver answered, the case expects the %s solver" % (info["solver"], want["solver"])
    tried = ec.route(n, nvec, c["env"])["solver"] == "tridiagonal"
    assert info["td_tried"] == tried and info["td_rejected"] == c["rejected"]
    if tried:
        assert info["td_back"] == want["back"]
        if not info["td_bailed"]:
            assert info["td_form"] == want["form"]
        else:
            assert info["td_form"] == "chain"
        assert (info["td_defect"] > ec.ACCEPT) == c["rejected"]
    else:
        assert info["td_form"] is None and info["td_back"] is None and not info["td_bailed"] and info["td_defect"] == 0.0
    assert (info["jacobi_sweeps"] >= 1) == (want["solver"] == "jacobi" and n > 1)
    ec.certify(c["key"], e, V, solver, nvec, "device")
    return r


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_case_is_inside_the_certificate(own, monkeypatch, name):
    c = ec.CASES[name]
    e, V, info = _solve(own, monkeypatch, c)
    _check(c, e, V, info)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [33, 1025])
def test_the_three_grid_barriers_give_the_same_bits_with_the_tridiagonal_solver_answering(own, monkeypatch, n):
    """Sharded counters (default), ISLE_TD_BAR=hier, ISLE_TD_BAR=flat: a barrier orders the same loads and stores in every form.  Bit
    equality means something only if the persistent tridiagonalisation ran and its solver answered in every run: three Jacobi answers
    (or three launch chains) would agree as well."""
    runs = [_solve(own, monkeypatch, ec.CASES["bar-%s-%d" % (bar, n)]) for bar in ("default", "hier", "flat")]
    for bar, (e, V, info) in zip(("default", "hier", "flat"), runs):
        assert info["solver"] == "tridiagonal" and not info["td_rejected"], bar
    if any(info["td_bailed"] for _, _, info in runs):
        print("n = %d: a grid barrier timed out on the shared device in one of the runs; the launch chain answered there, no bits to compare" % n)
        return
    assert all(info["td_form"] == "persistent" for _, _, info in runs)
    for e, V, _ in runs[1:]:
        assert np.array_equal(_bits(e), _bits(runs[0][0])) and np.array_equal(_bits(V), _bits(runs[0][1]))


@pytest.mark.parametrize("n", [257, 1025])
def test_chain_and_persistent_form_answer_with_the_tridiagonal_solver_and_agree_to_rounding(own, monkeypatch, n):
    """The two tridiagonalisations round differently (td_persist_k sums a column's products in another order than td_update_symv_k),
    so they are not bit-equal; both are certified above, and here each is seen to be the form it claims, in one context."""
    ep, Vp, ip = _solve(own, monkeypatch, ec.CASES["persist-%d" % n])
    ech, Vc, ic = _solve(own, monkeypatch, ec.CASES["chain-%d" % n])
    assert ip["solver"] == ic["solver"] == "tridiagonal" and ic["td_form"] == "chain" and (ip["td_form"] == "persistent" or ip["td_bailed"])
    assert np.abs(ep.astype(np.float64) - ech).max() <= 2 * ec.U32 * np.abs(ep).max()


def test_the_lower_triangle_is_not_read(own, monkeypatch):
    """The answers for the matrix with unrelated values below the diagonal are the symmetric matrix's, bit for bit, in both solvers."""
    for a, b in (("upper-130", "persist-130"), ("upper-130-jacobi", None)):
        e1, V1, i1 = _solve(own, monkeypatch, ec.CASES[a])
        sym = dict(ec.CASES[a], key=("sep", 130)) if b is None else ec.CASES[b]
        e0, V0, i0 = _solve(own, monkeypatch, sym)
        assert i0["solver"] == i1["solver"] == ec.CASES[a]["expect"]["solver"]
        if i0["td_form"] == i1["td_form"]:
            assert np.array_equal(_bits(e1), _bits(e0)) and np.array_equal(_bits(V1), _bits(V0))


def test_leading_vectors_are_the_full_solves_leading_vectors(own, monkeypatch):
    """nvec < n computes the same T, the same eigenvalues and the same twisted factorisations as nvec = n: the returned columns are the
    full solve's leading columns bit for bit (the back-transformation works on each vector alone)."""
    e0, V0, i0 = _solve(own, monkeypatch, ec.CASES["persist-130"])
    for nv in (1, 63, 64, 65, 129):
        e, V, i = _solve(own, monkeypatch, ec.CASES["nvec-130-%d" % nv])
        assert i["solver"] == "tridiagonal" and i["nvec"] == nv and V.shape == (130, nv)
        if i["td_form"] == i0["td_form"]:
            assert np.array_equal(_bits(e[:nv]), _bits(e0[:nv])) and np.all(e[nv:] == 0.0)
            assert np.array_equal(_bits(V), _bits(V0[:, :nv]))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_entry_of_the_upper_triangle_is_refused_before_any_launch(own, bad):
    """ISLE_E_NUMERIC from the host's look at the upper triangle: no kernel runs on it (the record still shows the solve before)."""
    from isle_amd import IsleHipError
    h = own.get()
    S = ec.matrix(("sep", 33)).copy()
    h.eig_sym(ec.matrix(("sep", 20)))
    before = h.eig_info()
    for i, j in ((0, 0), (3, 17), (32, 32)):
        T = S.copy()
        T[min(i, j), max(i, j)] = bad
        for nvec in (None, 5):
            with pytest.raises(IsleHipError, match="error -4"):
                h.eig_sym(T, nvec=nvec)
    assert h.eig_info() == before and before["n"] == 20


def test_a_non_finite_entry_below_the_diagonal_is_ignored(own, monkeypatch):
    """The strict lower triangle is not part of the input: NaN there changes nothing (and reaches no kernel's arithmetic)."""
    c = ec.CASES["persist-33"]
    e0, V0, i0 = _solve(own, monkeypatch, c)
    S = ec.matrix(c["key"]).copy()
    S[17, 3] = np.nan
    S[32, 0] = np.inf
    h = own.get()
    e, V = h.eig_sym(S)
    i1 = h.eig_info()
    assert i1["solver"] == "tridiagonal" and np.all(np.isfinite(e)) and np.all(np.isfinite(V))
    if i1["td_form"] == i0["td_form"]:
        assert np.array_equal(_bits(e), _bits(e0)) and np.array_equal(_bits(V), _bits(V0))
    ec.certify(c["key"], e, V, "tridiagonal")
