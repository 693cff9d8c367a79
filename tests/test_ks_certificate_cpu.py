"""tests/ks_certificate.py checked on its own, without a GPU: the constants it cites are the ones in the source, every case reaches the
dispatch edge it is named after, the float32 and float64 runs of the reference take the same decisions with margin, the float32 run sits
inside the bound with SPARE to spare, the recorded constants are the measured ones, and the certificate rejects four wrong rules by
TEETH or more.  Printed per case (-s or -rA): the edge, the float32-against-float64 figures, the factor of every wrong rule."""
import numpy as np
import pytest

import ks_certificate as kc

NAMES = sorted(kc.CASES)
TEETH = 10.0  # a wrong rule exceeds the bound by at least this factor on the case built for it


def _cdiv(a, b):
    return -(-a // b)


def _effective(run):
    """(m, b) of the orthogonalisation steps whose output reaches the returned pairs (those before the last truncation)."""
    return [(m, b) for step, m, b in run["ortho"] if step < run["steps_before_last_truncate"]]


@pytest.mark.parametrize("name", sorted(kc.SOURCE))
def test_cited_line_holds_the_constant(name):
    """vtf_rc, the update_mfma condition, PQ_ROWS, PQ_SUB, PQ_NSEG and the others: changed in the source -> the cases need another look."""
    assert kc.source_values(name) == kc.SOURCE[name][3]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge(name):
    c, run = kc.build(name), kc.reference(name)
    n, nev, blk, b = c["n"], c["nev"], c["blk"], run["b"]
    want, before = kc.ortho_sizes(nev, blk, c["ncv"], c["maxit"])
    assert [(m, w) for _, m, w in run["ortho"]] == want and run["steps_before_last_truncate"] == before
    eff = _effective(run)
    routes = [kc.route(n, w, m) for m, w in eff]
    assert c["ncv"] <= 135 and n <= 2049 and (n, nev) not in ((2000, 10), (2000, 20), (6000, 50))  # small, and not a workload's own size
    assert b == blk, "the block width is not overridden (ks_host.h ks_effective_blk)"
    edge = c["edge"]
    if edge == "blk":
        bt, rows, upd = {1: (4, 1024, True), 12: (12, 1024, True), 13: (16, 512, True), 16: (16, 512, True), 17: (32, 256, False), 32: (32, 256, False)}[blk]
        assert kc.bt_of(b) == bt and kc.vtf_rc(bt) == rows
        assert n % 4 == 0 and (blk == 1 or any(m >= 32 for m, _ in eff))
        assert all((r["update"] == "mfma") == (upd and m >= 32) for r, (m, _) in zip(routes, eff))
        assert any(r["vtf"] == "valu" and r["vtf_rows"] == rows for r in routes)
        if blk == 32:
            assert b == kc.PQ_W
        print("%s: BT %d, %d rows per chunk of V^T F, update on the matrix cores at m >= 32: %s" % (name, bt, rows, upd))
    elif edge == "mod4":
        assert name == "mod4-%d" % (n % 4) and b <= 16
        big = [r for r, (m, _) in zip(routes, eff) if m >= 32]
        assert big and all((r["update"] == "mfma") == (n % 4 == 0) for r in big)
        assert any(r["vtf"] == "mfma" for r in routes) and any(r["vtf"] == "valu" for r in routes)
        print("%s: n %% 4 = %d, update %s at m >= 32, V^T F on both routes" % (name, n % 4, big[0]["update"]))
    elif edge == "rows":
        R = {20: 256, 16: 512, 12: 1024, 10: 2048}[blk]
        assert abs(n - R) <= 1 and name == "rows-%d" % n
        if R < 2048:
            assert any(r["vtf"] == "valu" and r["vtf_rows"] == R for r in routes), "V^T F runs with chunks of the edge's size"
            assert _cdiv(n, R) == (2 if n > R else 1)
        else:
            slab = kc.PQ_ROWS * kc.PQ_SUB
            assert R == slab * kc.PQ_NSEG and _cdiv(n, slab) == (kc.PQ_NSEG + 1 if n > R else kc.PQ_NSEG)
        assert _cdiv(n, kc.PQ_ROWS) == R // kc.PQ_ROWS + (1 if n > R else 0)
        assert b > 16 or any(r["vtf"] == "mfma" and r["vtf_rows"] == 256 for r in routes)
        print("%s: %d rows against chunks of %d (V^T F), %d slabs of %d (panel QR)" % (name, n, R, _cdiv(n, kc.PQ_ROWS), kc.PQ_ROWS))
    elif edge == "basis":
        m0 = int(name.split("-")[1])
        assert (m0, b) in eff[len(kc.ortho_sizes(nev, blk, c["ncv"], 0)[0]):], "the size is reached after the restart, before the last truncation"
        assert b <= 16 and n % 4 == 0
        r = kc.route(n, b, m0)
        assert (r["update"] == "mfma") == (m0 >= 32) and (r["vtf"] == "mfma") == (m0 >= 64)
        assert _cdiv(m0, kc.VTF_CG) == {31: 1, 32: 1, 33: 2, 63: 2, 64: 2, 65: 3}[m0]
        print("%s: m = %d -> V^T F %s, update %s" % (name, m0, r["vtf"], r["update"]))
    else:
        assert edge == "ragged" and c["ncv"] % b and nev % b
        print("%s: ncv %d, nev %d, blk %d" % (name, c["ncv"], nev, b))


def test_the_routes_differ_across_each_edge():
    """Both sides of every dispatch condition are taken by some case."""
    seen = set()
    for name in NAMES:
        c, run = kc.build(name), kc.reference(name)
        for m, b in _effective(run):
            r = kc.route(c["n"], b, m)
            seen.add((r["vtf"], r["vtf_rows"], r["update"], kc.bt_of(b)))
    assert {s[3] for s in seen} == {4, 8, 12, 16, 32}
    assert {(s[0], s[1]) for s in seen} >= {("valu", 1024), ("valu", 512), ("valu", 256), ("mfma", 256)}
    assert {s[2] for s in seen} == {"mfma", "valu"}


@pytest.mark.parametrize("name", NAMES)
def test_float32_and_float64_take_the_same_decisions(name):
    c = kc.build(name)
    r64, r32 = kc.reference(name), kc.reference(name, np.float32)
    d64, d32 = kc.decisions(c, r64), kc.decisions(c, r32)
    for k in kc.COUNTERS:
        assert r64[k] == r32[k], k
    assert d64["js"] == d32["js"] and r64["ortho"] == r32["ortho"] and r64["m"] == r32["m"]
    assert r64["restarts"] == c["maxit"], "the run ends by its restart count, not by convergence"
    assert min(d64["pivot"], d32["pivot"]) >= kc.PIVOT_MARGIN
    assert min(d64["residual"], d32["residual"]) >= kc.DECISION_MARGIN
    print("%s: converged at the tests %s, estimates %.3g x from tol, smallest pivot %.3g" % (name, d64["js"], min(d64["residual"], d32["residual"]),
                                                                                          min(r64["pivots"] + r32["pivots"])))


def test_both_kinds_of_restart_occur():
    js = [tuple(kc.decisions(kc.build(n), kc.reference(n))["js"]) for n in NAMES]
    assert any(j[0] == 0 for j in js) and any(j[0] > 0 for j in js) and any(len(j) == 2 and j[0] == 0 and j[1] > 0 for j in js)
    assert {kc.CASES[n]["maxit"] for n in NAMES} == {1, 2}


@pytest.mark.parametrize("name", NAMES)
def test_float32_run_is_inside_the_bound_with_room(name):
    c = kc.build(name)
    r = kc.ratios(c, kc.reference(name, np.float32), kc.reference(name))
    print("%s: float32 / float64 in units of m u ||A||: %s" % (name, ", ".join("%s %.3g" % (q, kc.reference_figures([name])[name][q]) for q in kc.QUANTITIES)))
    assert max(r.values()) <= 1.0 / kc.SPARE, r


def test_recorded_constants_are_the_measured_ones():
    """C = MARGIN x the largest float32 figure over ALL cases: the record is neither below it nor more than twice above it."""
    fig = kc.reference_figures()
    for q in kc.QUANTITIES:
        worst = max(f[q] for f in fig.values())
        assert 0.5 * kc.R32[q] <= worst <= 1.0 * kc.R32[q] * 2.0, (q, worst, kc.R32[q])
        assert kc.C[q] == kc.MARGIN * kc.R32[q] and kc.MARGIN == 8.0


WRONG = [
    ("rows-257", dict(drop_rows=1), np.float64),   # one row of 257 missing from both projections of the first expand step
    ("rows-2049", dict(drop_rows=0), np.float64),  # the same at the largest n, in init
    ("mod4-1", dict(drop_rows=2), np.float64),
    ("blk-13", dict(zero_col=(2, 12)), np.float64),  # the thirteenth column: the first past a 12-wide tile
    ("blk-32", dict(zero_col=(2, 31)), np.float64),
    ("basis-65", dict(one_pass=True), np.float32),   # one Gram-Schmidt pass loses orthogonality in float32 only
    ("rows-2049", dict(one_pass=True), np.float32),
    ("ragged-37-8", dict(keep_short=True), np.float64),
    ("blk-12", dict(keep_short=True), np.float64),   # maxit = 1: the last returned vector is not a Ritz vector
]


@pytest.mark.parametrize("name,wrong,dtype", WRONG, ids=["%s-%s" % (w[0], next(iter(w[1]))) for w in WRONG])
def test_wrong_rule_fails_the_bound(name, wrong, dtype):
    c, ref = kc.build(name), kc.reference(name)
    got = kc.reference(name, dtype, wrong=wrong)
    r = kc.ratios(c, got, ref)
    print("%s under %s (%s): error / bound %s" % (name, wrong, np.dtype(dtype).name, ", ".join("%s %.3g" % (q, r[q]) for q in kc.QUANTITIES)))
    assert max(r.values()) >= TEETH
    with pytest.raises(AssertionError):
        kc.certify(c, got, ref)
    right = kc.ratios(c, kc.reference(name, dtype), ref)
    assert max(right.values()) <= 1.0 / kc.SPARE  # the same run without the rule passes


def test_one_spoilt_pass_is_repaired_by_the_other():
    """Why the wrong rules spoil both passes of a step (module docstring): with only the FIRST projection short of its rows the sum
    c1 + c2 and the panel are right again to rounding."""
    name = "rows-257"
    c, ref = kc.build(name), kc.reference(name)
    A, S = c["A64"], c["S"]
    n = c["n"]
    Q0, _ = np.linalg.qr(S.astype(np.float64))
    F = A @ Q0
    c1 = Q0[:n - 1].T @ F[:n - 1]
    F1 = F - Q0 @ c1
    c2 = Q0.T @ F1
    assert np.abs((c1 + c2) - Q0.T @ F).max() <= 1e-14 and np.abs(Q0.T @ (F1 - Q0 @ c2)).max() <= 1e-14
    assert np.abs(c1 - Q0.T @ F).max() >= 1e-4


def test_converged_run_agrees_with_eigvalsh():
    c = kc.build("blk-12")
    r = kc.reference_run(c["A64"], c["S"][:, :2], 4, 2, 40, 200, 1e-9, np.float64)
    assert r["restarts"] < 200 and r["nconv"] == 4 == r["nconv_ref_rule"]
    true = np.linalg.eigvalsh(c["A64"])[::-1][:4]
    assert np.abs(r["evals"] - true).max() <= 1e-12
    U = r["U"]
    assert np.abs(U.T @ U - np.eye(4)).max() <= 1e-13 and np.linalg.norm(c["A64"] @ U - U * r["evals"], axis=0).max() <= 1e-8
