"""The block Krylov-Schur solver (api_ks.cpp, dense.hip, evd_tridiag.hip) through isle_hip_block_ks_dense and its start_block argument,
against the float64 run of the plain restatement in tests/ks_certificate.py: same start block, same number of restarts.  Compared are
what does not depend on the basis: the Ritz values value by value, of the returned vectors the orthonormality, the Rayleigh quotients,
the residual norms and the distance from the float64 run's Krylov space, each inside C m 2^-24 ||A||_2 with C from the reference alone,
and the four counters exactly.  The cases sit on the dispatch edges of dense.hip (block width, n mod 4, n at the row-chunk edges, the
basis size at which the orthogonalisation changes kernels, ragged ncv); test_ks_certificate_cpu.py asserts without a GPU that each
reaches its edge, that no decision of the loop sits near its threshold, and that four wrong rules fail these bounds.

At the end of the module the largest error / bound per case is printed; KS_CERT_REPORT=<path> writes it there as JSON
(profiles/ks_certificate.md holds a measured run)."""
import json
import os
import time

import numpy as np
import pytest

import ks_certificate as kc

pytestmark = pytest.mark.gpu

STATS = {}
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def certificate_summary():
    yield STATS
    wall = time.time() - _T0
    for name, s in sorted(STATS.items()):
        print("ks certificate, %s: error / bound %s" % (name, ", ".join("%s %.3g" % (q, s[q]) for q in kc.QUANTITIES if q in s)))
    print("ks certificate: %.1f s" % wall)
    path = os.environ.get("KS_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(STATS, wall_seconds=wall), f, indent=1, sort_keys=True)


def _solve(hp, c):
    return hp.block_ks_dense(c["A"], c["nev"], blk=c["blk"], ncv=c["ncv"], maxit=c["maxit"], tol=c["tol"], start_block=c["S"], allow_noconv=True)


def _record(key, c, got, ref):
    """Every figure is printed and kept before anything is asserted."""
    r = kc.ratios(c, got, ref)
    STATS[key] = dict(r, m=ref["m"], **{k: got[k] for k in kc.COUNTERS})
    print("%s: m = %d, counters %s (fp64 run %s), error / bound %s" % (key, ref["m"], [got[k] for k in kc.COUNTERS], [ref[k] for k in kc.COUNTERS],
                                                                     ", ".join("%s %.3g" % (q, r[q]) for q in kc.QUANTITIES)))


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_case_is_inside_the_certificate(hp, name):
    c, ref = kc.build(name), kc.reference(name)
    got = _solve(hp, c)
    _record(name, c, got, ref)
    assert got["rc"] in (0, -3) and np.all(np.isfinite(got["evals"])) and np.all(np.isfinite(got["U"]))
    kc.certify(c, got, ref, "device")


FORMS = (("ISLE_UPDATE_MFMA", "0"), ("ISLE_KS_SYNC", "1"), ("ISLE_KS_ORTHO_PASSES", "3"))


@pytest.mark.parametrize("name", ["mod4-0", "basis-64", "rows-1025"])
def test_exact_forms_hold_the_same_bound(hp, monkeypatch, name):
    """update_k in place of update_mfma_k (mod4-0 and basis-64 take the matrix-core update by default, rows-1025 does not), the
    synchronous expand loop, three Gram-Schmidt passes: the same bound (the reference with three passes for the last; its counters are
    those of two), and the synchronous loop gives the default's bits."""
    c, ref = kc.build(name), kc.reference(name)
    base = _solve(hp, c)
    for var, val in FORMS:
        monkeypatch.setenv(var, val)
        got = _solve(hp, c)
        monkeypatch.delenv(var)
        r = kc.reference(name, passes=3) if var == "ISLE_KS_ORTHO_PASSES" else ref
        _record("%s %s=%s" % (name, var, val), c, got, r)
        kc.certify(c, got, r, "%s=%s" % (var, val))
        if var == "ISLE_KS_SYNC":
            assert np.array_equal(got["evals"].view(np.uint32), base["evals"].view(np.uint32))
            assert np.array_equal(got["U"].view(np.uint32), base["U"].view(np.uint32))
            assert all(got[k] == base[k] for k in kc.COUNTERS)
    again = _solve(hp, c)
    assert np.array_equal(again["U"].view(np.uint32), base["U"].view(np.uint32)), "the default form is deterministic"
