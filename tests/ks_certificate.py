"""Plain restatement of the restarted block Krylov-Schur loop of isle_amd/csrc/api_ks.cpp / ks_host.h on a dense operator, the cases built for the
dispatch edges of dense.hip, and the bounds of the fp64 certificate (no GPU, no oracle library; numpy only).

reference_run: init (Ks::init, ks_h_start) from a given start block, expand (Ks::expand, ks_fold_step) in whole blocks to at least ncv rows,
truncate (Ks::truncate, ks_h_truncate) through the small symmetric EVD of the UPPER triangle of H (evd_tridiag.hip:839-840), the residual
test (ks_first_unconverged), maxit restarts (Ks::compute) and the counters of ks_solve (ks_final_counts).  One body, the dtype a parameter: float64 is the reference, float32 measures
what the same algorithm loses in the device's number format.  numpy.linalg.qr stands where the device has CholQR2 and numpy.linalg.eigh
where it has tridiagonalisation and bisection: the factors differ in sign and basis, so only quantities that do not depend on the basis
are compared (`measure`): the Ritz values, and of the returned vectors the orthonormality, the Rayleigh quotients, the residual norms and
the distance from the Krylov space of the fp64 run.  The counters must be equal.

Determinism.  Every case fixes the start block; the spectrum (`spectrum`) is simple and of full rank, ||A||_2 = 1.  The data-dependent
decisions of the loop are the rank of every panel (dense.hip:562-564: a pivot below 1e-6, or its square below 1e-13 w of the column's
own square), the number of converged pairs (ks_first_unconverged) and with it how many vectors truncation rotates (Ks::truncate: keep).  `decisions`
returns them with their margins: every pivot is at least PIVOT_MARGIN times the drop threshold, every residual estimate that the test
reads is DECISION_MARGIN away from tol on either side, in the fp32 and in the fp64 run; test_ks_certificate_cpu.py asserts it.

Bounds.  Each compared quantity q of a run with a basis of m vectors (the rows of H at the last truncation) is held to
    q <= C[q] * m * 2^-24 * ||A||_2,    C[q] = MARGIN * R32[q],    MARGIN = 8,
where R32[q] is the largest q / (m 2^-24 ||A||_2) of the float32 run of reference_run against its float64 run over ALL cases (recorded
below from numpy on the CPU; the CPU test recomputes every case and holds it to C[q] / SPARE).  The margin stands for the device's other
summation order and its CholQR2 in place of Householder; it is not tuned to what the device gives.

Wrong rules (`wrong=`), for the CPU test of the certificate's own teeth.  A restarted method with two Gram-Schmidt passes repairs a
defect of ONE pass: H takes c1 + c2, and whatever the first projection missed the second one finds, so a rule that spoils a single pass
of a single step is invisible by construction, on the device as here.  A kernel that is wrong is wrong in every launch of a shape, so the
rules spoil both passes of one step: "drop_rows" leaves the last n % 256 rows out of both projections of step `step`, "zero_col" zeroes
column `col` of both V^T F of that step; "one_pass" skips the second pass in every step; "keep_short" rotates one Ritz vector too few at
every truncation; "skip_slice" (r0, r1) leaves the rows [r0, r1) of the panel unorthogonalised in every pass of every step (the
row-sharded step with one rank's update missing).
"""
import os
import re

import numpy as np

U_F32 = 2.0 ** -24
MARGIN = 8.0            # device against the float32 reference run: other summation order, CholQR2
SPARE = 4.0             # the float32 run itself stays this far inside the bound on any BLAS (the recorded figures leave a factor 2 for that)
DECISION_MARGIN = 4.0   # residual estimate / tol or tol / estimate, at least
PIVOT_MARGIN = 100.0    # smallest panel pivot / 1e-6, at least
PIVOT_DROP = 1e-6       # dense.hip:564, ks_utils.h:66-69
QUANTITIES = ("ritz", "orth", "rayleigh", "residual", "containment")

# Largest float32-against-float64 figure of reference_run over all cases, in units of m 2^-24 ||A||_2 (numpy 2.2, OpenBLAS, CPU).
# reference_figures() recomputes them; profiles/ks_certificate.md holds the table per case.
R32 = dict(ritz=0.0165, orth=0.0425, rayleigh=0.0425, residual=0.155, containment=8.2)
C = {q: MARGIN * R32[q] for q in QUANTITIES}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------------------------
# The constants the cases were built from: name -> (file, line, pattern with one group per value, values).
# test_ks_certificate_cpu.py reads the cited line and fails when the text or the line moved: update the cases, then this table.
# ---------------------------------------------------------------------------------------------------------------------------------
DENSE, KS_HOST, ROUTE_HOST = "isle_amd/csrc/dense.hip", "isle_amd/csrc/ks_host.h", "isle_amd/csrc/route_host.h"
SOURCE = {
    "VTF_CG": (DENSE, 25, r"constexpr int VTF_CG = (\d+);", (32,)),
    "vtf_rc": (DENSE, 27, r"constexpr int vtf_rc\(int BT\) \{ return BT <= (\d+) \? (\d+) : \(BT <= (\d+) \? (\d+) : (\d+)\); \}", (12, 1024, 16, 512, 256)),
    "VM_RC": (DENSE, 78, r"constexpr int VM_RC = (\d+);", (1024,)),
    "bt_of": (DENSE, 181, r"static int bt_of\(int b\) \{ return b <= (\d+) \? 4 : b <= (\d+) \? 8 : b <= (\d+) \? 12 : b <= (\d+) \? 16 : 32; \}", (4, 8, 12, 16)),
    "vtf_mfma": (DENSE, 211, r"if \(b <= (\d+) && m >= (\d+)\) \{", (16, 64)),
    "update_mfma": (ROUTE_HOST, 148, r"return b <= (\d+) && m >= (\d+) && \(ld & (\d+)\) == 0 && ", (16, 32, 3)),  # route_update_mfma
    "PQ_ROWS": (DENSE, 401, r"constexpr int PQ_ROWS = (\d+);", (256,)),
    "PQ_W": (DENSE, 402, r"constexpr int PQ_W = (\d+);", (32,)),
    "PQ_SUB": (DENSE, 403, r"constexpr int PQ_SUB = (\d+);", (2,)),
    "PQ_NSEG": (DENSE, 449, r"constexpr int PQ_NSEG = (\d+);", (4,)),
    "blk_rule": (KS_HOST, 37, r"return \(blk < nev\) \? blk : 1;", ()),  # ks_effective_blk
    "ortho_passes": (KS_HOST, 52, r"int npass = (\d+);", (2,)),  # ks_ortho_passes
}


def source_values(name):
    """The values of SOURCE[name] as the cited line holds them now (AssertionError when the line no longer matches)."""
    path, line, pat, _ = SOURCE[name]
    with open(os.path.join(ROOT, path)) as f:
        text = f.read().split("\n")[line - 1]
    m = re.search(pat, text)
    assert m, "%s:%d no longer reads %r (it reads %r): revisit the cases of tests/ks_certificate.py, then SOURCE" % (path, line, pat, text.strip())
    return tuple(int(g) for g in m.groups())


VTF_CG = SOURCE["VTF_CG"][3][0]
PQ_ROWS, PQ_W, PQ_SUB, PQ_NSEG = (SOURCE[k][3][0] for k in ("PQ_ROWS", "PQ_W", "PQ_SUB", "PQ_NSEG"))
VM_RC = SOURCE["VM_RC"][3][0]


def bt_of(b):
    """dense.hip:181."""
    e = SOURCE["bt_of"][3]
    return 4 if b <= e[0] else 8 if b <= e[1] else 12 if b <= e[2] else 16 if b <= e[3] else 32


def vtf_rc(BT):
    """dense.hip:27."""
    a, ra, b, rb, rc = SOURCE["vtf_rc"][3]
    return ra if BT <= a else (rb if BT <= b else rc)


def route(n, b, m, num_cus=256, ld=None):
    """Which kernels one orthogonalisation pass of a b-wide panel against m basis vectors of n rows takes.  ld: the leading dimension of
    basis and panel — n in the dense entry and in the replicated step; the row count of the whole block when n is a rank's row slice
    (Ks::ortho: the slice starts at a multiple of four rows, ks_row_slice, so it is 16-byte aligned exactly when the block is).  Basis
    and panel are separate allocations, so the 16-byte test of dense.hip:366 (route_update_mfma) rests on ld alone.
    -> dict(vtf: "mfma" | "valu" | "none", vtf_rows: rows per chunk, vtf_aligned: vtf_mfma_k's float4 path (dense.hip:97),
    update: "mfma" | "valu" | "none"); "none": a slice of zero rows launches nothing (dense.hip:207, :363)."""
    ld = n if ld is None else ld
    if n == 0:
        return dict(vtf="none", vtf_rows=0, vtf_aligned=False, update="none")
    bmax, mmin = SOURCE["vtf_mfma"][3]
    ub, um, mask = SOURCE["update_mfma"][3]
    if b <= bmax and m >= mmin:
        rc = VM_RC  # dense.hip:217-218
        cd = lambda a, d: -(-a // d)
        while rc > 256 and cd(n, rc // 2) <= 128 and cd(n, rc) * cd(m, 128) < 2 * num_cus:
            rc //= 2
        vtf, rows = "mfma", rc
    else:
        vtf, rows = "valu", vtf_rc(bt_of(b))
    return dict(vtf=vtf, vtf_rows=rows, vtf_aligned=vtf == "mfma" and (ld & mask) == 0,
                update="mfma" if (b <= ub and m >= um and (ld & mask) == 0) else "valu")


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------
def effective_blk(nev, blk):
    """ks_host.h ks_effective_blk."""
    return blk if blk < nev else 1


def reference_run(A, S, nev, blk, ncv, maxit, tol, dtype, wrong=None, passes=2):
    """-> dict(evals, U, restarts, napplies, nconv, nconv_ref_rule, m (rows of H at the last truncation), space (the basis columns that
    truncation rotated: the returned vectors lie in their span), ortho [(step, m, b, counted)], pivots [smallest |R_ii| of every panel],
    tests [(residual estimates, first unconverged)], steps_before_last_truncate)."""
    dt = np.dtype(dtype)
    wrong = wrong or {}
    A = np.asarray(A, dt)
    n = A.shape[0]
    b = effective_blk(nev, blk)
    assert nev >= 1 and 1 <= blk <= 32 and maxit >= 1 and ncv >= nev + 2 * b and ncv + b <= n  # ks_host.h ks_check_counts, ks_check_range
    tol = dt.type(tol)
    V = np.zeros((n, ncv + 2 * b), dt, order="F")      # ks_solve: the basis
    H = np.zeros((ncv + 2 * b, ncv + b), dt, order="F")
    tr = dict(ortho=[], pivots=[], tests=[], estimates=[])
    st = dict(napplies=0, step=0, hr=0, hc=0, nconv=0, last_j=0, truncations=0, space=None, m=0, steps_at_truncate=0)

    def qr(F):
        Q, R = np.linalg.qr(F)
        assert Q.dtype == dt and R.dtype == dt
        tr["pivots"].append(float(np.abs(np.diag(R)).min()))
        return Q, R

    def ortho(F, m):
        """`passes` times c = V^T F, F -= V c (Ks::ortho); H takes the sum of the c (ks_fold_step)."""
        step = st["step"]
        st["step"] += 1
        tr["ortho"].append((step, m, F.shape[1]))
        Vm = V[:, :m]
        coef = np.zeros((m, F.shape[1]), dt)
        npass = 1 if wrong.get("one_pass") else passes
        for p in range(npass):
            if wrong.get("drop_rows") == step and n % 256:
                c = Vm[:n - n % 256].T @ F[:n - n % 256]
            else:
                c = Vm.T @ F
            if "zero_col" in wrong and wrong["zero_col"][0] == step:
                c[:, wrong["zero_col"][1]] = 0
            Fn = F - Vm @ c
            if "skip_slice" in wrong:  # the rows of one rank's slice are left as they were, in every pass of every step
                r0, r1 = wrong["skip_slice"]
                Fn[r0:r1] = F[r0:r1]
            F = Fn
            coef = coef + c
        assert F.dtype == dt and coef.dtype == dt
        return F, coef

    def apply(X):
        st["napplies"] += 1
        return A @ X

    def init():  # Ks::init, ks_h_start
        Q0, _ = qr(np.asarray(S, dt))
        V[:, :b] = Q0
        F, coef = ortho(apply(V[:, :b]), b)
        Q1, R = qr(F)
        H[:b, :b] = coef
        H[b:2 * b, :b] = R
        V[:, b:2 * b] = Q1
        st["hr"], st["hc"] = 2 * b, b

    def expand():  # Ks::expand, ks_fold_step
        while st["hr"] < ncv:
            m, hc = st["hr"], st["hc"]
            F, coef = ortho(apply(V[:, hc:hc + b]), m)
            Q, R = qr(F)
            H[:m, hc:hc + b] = coef
            H[m:m + b, hc:hc + b] = R
            V[:, m:m + b] = Q
            st["hr"], st["hc"] = m + b, hc + b

    def truncate():  # Ks::truncate, ks_h_truncate
        hr, hc, nconv = st["hr"], st["hc"], st["nconv"]
        nn, keep = hc - nconv, nev - nconv
        st["m"], st["space"], st["steps_at_truncate"] = hr, V[:, :hc].copy(), st["step"]
        w, Z = np.linalg.eigh(H[nconv:hc, nconv:hc], UPLO="U")
        assert w.dtype == dt and Z.dtype == dt
        eH, vH = w[::-1], Z[:, ::-1][:, :keep]
        rot = keep - 1 if wrong.get("keep_short") else keep
        Vn = V[:, nconv:hc] @ vH[:, :rot]
        tail = V[:, hr - b:hr].copy()
        top = H[:nconv, nconv:hc] @ vH
        newrows = H[hr - b:hr, hc - b:hc] @ vH[nn - b:, :]
        Hn = np.zeros_like(H)
        Hn[:nev, :nconv] = H[:nev, :nconv]
        Hn[nev:nev + b, :nconv] = H[nev:nev + b, :nconv]
        for j in range(nconv, nev):
            Hn[j, j] = eH[j - nconv]
            Hn[nev:nev + b, j] = newrows[:, j - nconv]
            Hn[:nconv, j] = top[:, j - nconv]
        H[:] = Hn
        V[:, nconv:nconv + rot] = Vn
        V[:, nev:nev + b] = tail
        V[:, nev + b:] = 0
        st["hr"], st["hc"] = nev + b, nev
        st["truncations"] += 1

    def first_unconverged(divide):  # ks_first_unconverged -> (first j at or above tol, the estimates it read, the estimates of all columns)
        hr, hc = st["hr"], st["hc"]
        est = []
        for j in range(hc):
            s = dt.type(0)
            for i in range(hr - b, hr):
                s = dt.type(s + H[i, j] * H[i, j])
            nrm = np.sqrt(s)
            if divide:
                nrm = nrm / H[j, j]
            est.append(float(nrm))
        j = next((j for j in range(hc) if dt.type(est[j]) >= tol), hc)
        return j, est[:j + 1], est

    init()
    restarts = 0
    expand()
    while restarts < maxit:  # Ks::compute
        truncate()
        j, est, every = first_unconverged(True)
        tr["tests"].append((est, j))
        tr["estimates"].append(every)
        st["last_j"] = j
        if j == st["hc"]:
            st["nconv"] = st["hc"]
            break
        st["nconv"] = j
        restarts += 1
        expand()
    nc = nc_ref = st["nconv"]
    if restarts == maxit:  # ks_final_counts
        nc_ref = first_unconverged(False)[0]
        nc = min(st["last_j"], nev)
    out = dict(evals=np.diag(H)[:nev].copy(), U=V[:, :nev].copy(), restarts=restarts, napplies=st["napplies"], nconv=min(nc, nev),
               nconv_ref_rule=min(nc_ref, nev), m=st["m"], space=st["space"], steps_before_last_truncate=st["steps_at_truncate"], b=b)
    out.update(tr)
    return out


def ortho_sizes(nev, blk, ncv, maxit):
    """(m, b) of every orthogonalisation step when nothing converges early and no panel loses rank, and how many of them come before
    the last truncation (what runs after it moves only the counters)."""
    b = effective_blk(nev, blk)
    out, hr = [(b, b)], 2 * b
    before = 0
    for r in range(maxit + 1):
        while hr < ncv:
            out.append((hr, b))
            hr += b
        if r < maxit:
            before = len(out)
        hr = nev + b
    return out, before


COUNTERS = ("restarts", "napplies", "nconv", "nconv_ref_rule")


def measure(A64, evals, U, ref):
    """The basis-independent figures of a run (evals, U) against the fp64 run `ref`, in fp64 -> dict over QUANTITIES (absolute)."""
    ev = np.asarray(evals, np.float64)
    U = np.asarray(U, np.float64)
    rU = np.asarray(ref["U"], np.float64)
    rev = np.asarray(ref["evals"], np.float64)
    k = U.shape[1]
    AU = A64 @ U
    res = np.linalg.norm(AU - U * ev, axis=0)
    rres = np.linalg.norm(A64 @ rU - rU * rev, axis=0)
    Vs = np.asarray(ref["space"], np.float64)
    return dict(ritz=float(np.abs(ev - rev).max()), orth=float(np.abs(U.T @ U - np.eye(k)).max()),
                rayleigh=float(np.abs(np.sum(U * AU, axis=0) - ev).max()), residual=float(np.abs(res - rres).max()),
                containment=float(np.linalg.norm(U - Vs @ (Vs.T @ U), axis=0).max()))


def unit(case, ref):
    """m 2^-24 ||A||_2 of a case."""
    return ref["m"] * U_F32 * case["norm2"]


def ratios(case, got, ref):
    """q / (C[q] m 2^-24 ||A||_2) for every quantity: the certificate holds when all are <= 1."""
    ms = measure(case["A64"], got["evals"], got["U"], ref)
    return {q: ms[q] / (C[q] * unit(case, ref)) for q in QUANTITIES}


def certify(case, got, ref, what=""):
    """Counters equal, every quantity inside its bound.  -> the ratios."""
    for k in COUNTERS:
        assert got[k] == ref[k], "%s %s: %s is %d, the fp64 run has %d" % (case["name"], what, k, got[k], ref[k])
    r = ratios(case, got, ref)
    bad = {q: v for q, v in r.items() if not v <= 1.0}
    assert not bad, "%s %s: outside the bound C m u ||A|| (m = %d), error / bound: %s" % (
        case["name"], what, ref["m"], ", ".join("%s %.3g" % kv for kv in sorted(bad.items())))
    return r


def decisions(case, run):
    """-> dict(pivot: smallest panel pivot / 1e-6, residual: smallest distance factor of a residual estimate that was read from tol,
    js: the first unconverged index of every test)."""
    tol = float(np.float32(case["tol"]))
    far = min(max(e / tol, tol / e) if e > 0 else np.inf for est, _ in run["tests"] for e in est)
    return dict(pivot=min(run["pivots"]) / PIVOT_DROP, residual=far, js=[j for _, j in run["tests"]])


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
# tol per case: between the residual estimates of the four leading pairs and those of the bulk at every test of the run, DECISION_MARGIN
# or more from both (1e-5 / 3e-5: nothing has converged at the first test, js = [0, ...]; 1e-4 / 3e-4: the four leading pairs are locked)
TOL = {"blk-12": 1e-5, "blk-13": 3e-5, "blk-17": 3e-4, "blk-32": 1e-5, "rows-255": 1e-5, "rows-256": 1e-5, "rows-257": 1e-5, "rows-511": 1e-5,
       "rows-512": 1e-5, "rows-513": 1e-5, "basis-31": 1e-5, "basis-32": 1e-5, "basis-33": 1e-5}


def _case(name, edge, n, nev, blk, ncv, maxit):
    tol = TOL.get(name, 1e-4)
    return dict(name=name, edge=edge, n=n, nev=nev, blk=blk, ncv=ncv, maxit=maxit, tol=tol)


def _cases():
    out = []
    # blk: bt_of (dense.hip:181) 4 | 12 | 16 | 32, vtf_rc (:27) 1024 | 512 | 256, update_mfma b <= 16 (route_host.h route_update_mfma), PQ_W (:402)
    for blk, nev, ncv, maxit in ((1, 6, 24, 2), (12, 24, 60, 1), (13, 24, 60, 2), (16, 24, 64, 1), (17, 24, 68, 2), (32, 40, 104, 2)):
        out.append(_case("blk-%d" % blk, "blk", 400, nev, blk, ncv, maxit))
    # n % 4: the (ld & 3) == 0 test of route_update_mfma (and the aligned test of vtf_mfma_k, :97), b = 12 <= 16 and m up to 72 >= 64
    for n in (300, 301, 302, 303):
        out.append(_case("mod4-%d" % (n % 4), "mod4", n, 24, 12, 80, 2 if n % 2 else 1))
    # n at row-chunk edges: vtf_rc (:27) through blk = 20 (256 rows), 16 (512), 12 (1024); VM_RC (:78), PQ_ROWS (:401), and the
    # PQ_NSEG (:449) runs of PQ_ROWS * PQ_SUB (:403) rows at 2047 / 2049; ncv = 75 with blk = 10 is ragged as well
    for n, blk in ((255, 20), (256, 20), (257, 20), (511, 16), (512, 16), (513, 16), (1023, 12), (1024, 12), (1025, 12), (2047, 10), (2049, 10)):
        ncv = {20: 90, 16: 80, 12: 76, 10: 75}[blk]
        out.append(_case("rows-%d" % n, "rows", n, 30, blk, ncv, 1 + (n + blk) % 2))
    # basis size m when the orthogonalisation runs: m = nev + blk, nev + 2 blk, ... after the restart (VTF_CG :25, m >= 32 :366, m >= 64 :211)
    for m, nev, blk, ncv in ((31, 19, 12, 50), (32, 20, 12, 50), (33, 21, 12, 50), (63, 39, 12, 76), (64, 40, 12, 76), (65, 41, 12, 76)):
        out.append(_case("basis-%d" % m, "basis", 388, nev, blk, ncv, 2))
    # ragged ncv (and nev) with a narrow block
    out.append(_case("ragged-37-8", "ragged", 362, 37, 8, 61, 2))
    return out


CASES = {c["name"]: c for c in _cases()}
_BUILT = {}


LEADING = (1.0, 0.9, 0.8, 0.7)


def spectrum(n):
    """Four separated values, which converge within a restart, above a slowly decaying bulk, which does not: the residual estimates of
    the two groups lie decades apart, and tol goes between them.  Simple, positive, ||A||_2 = 1."""
    g = len(LEADING)
    return np.concatenate([LEADING, 0.2 - 0.1 * np.arange(n - g, dtype=np.float64) / (n - g)])


def build(name):
    """The case with A (float32, Fortran order), A64 (the same values widened), S (float32 start block), norm2 (||A64||_2).  Cached."""
    if name not in _BUILT:
        c = dict(CASES[name])
        n = c["n"]
        seed = int.from_bytes(name.encode(), "little") % (2 ** 31)
        rng = np.random.default_rng(seed)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * spectrum(n)) @ Q.T
        A = 0.5 * (A + A.T)
        c["A"] = np.asfortranarray(A.astype(np.float32))
        c["A64"] = c["A"].astype(np.float64)
        c["S"] = np.asfortranarray(rng.uniform(size=(n, effective_blk(c["nev"], c["blk"]))).astype(np.float32))
        c["norm2"] = float(np.abs(np.linalg.eigvalsh(c["A64"])[[0, -1]]).max())
        _BUILT[name] = c
    return _BUILT[name]


_RUNS = {}


def reference(name, dtype=np.float64, wrong=None, passes=2):
    """reference_run on a case, cached per (case, dtype, rule)."""
    key = (name, np.dtype(dtype).name, repr(sorted((wrong or {}).items())), passes)
    if key not in _RUNS:
        c = build(name)
        _RUNS[key] = reference_run(c["A64"], c["S"], c["nev"], c["blk"], c["ncv"], c["maxit"], c["tol"], dtype, wrong=wrong, passes=passes)
    return _RUNS[key]


def reference_figures(names=None):
    """name -> {quantity: float32 run against float64 run, in units of m 2^-24 ||A||_2} (what R32 records the largest of)."""
    out = {}
    for name in (names or sorted(CASES)):
        c, r64, r32 = build(name), reference(name), reference(name, np.float32)
        ms = measure(c["A64"], r32["evals"], r32["U"], r64)
        out[name] = {q: ms[q] / unit(c, r64) for q in QUANTITIES}
    return out
