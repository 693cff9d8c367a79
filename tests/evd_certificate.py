"""The fp64 certificate of the small symmetric eigensolver (k_eig_small: evd_tridiag.hip, the block Jacobi solver of dense.hip), its cases at
the dispatch edges of both, and a plain restatement of the rules that choose a kernel form (no GPU; numpy and scipy only).

Reference.  scipy.linalg.eigh(driver="evd") in float64 of the matrix that the UPPER triangle of the same float32 S defines (LAPACK 'U':
td_sym_k, the host loop of k_jacobi_eig), descending, cached per matrix (`reference`).  Nothing from the code under test enters a bound.

Bounds.  Both solvers work in fp64 and round to fp32 once, at the end, so the honest bound is the fp32 rounding of the fp64 answer plus
what a backward-stable fp64 solver may differ by.  With u32 = 2^-24, unit = n 2^-53 ||S||_2, gap_j the reference's distance from
lambda_j to its nearest other eigenvalue, and s = C unit:
    eigenvalues       |e_i - lambda_i|        <= u32 |lambda_i| + s
    eigenvectors      |v_ij - u_ij|           <= b_ij = u32 |u_ij| + s / gap_j                      (sign fixed by <v_j, u_j>)
    orthonormality    |(V^T V - I)_jk|        <= sum_i (|u_ij| b_ik + |u_ik| b_ij + b_ij b_ik)      (all pairs)
    residual          |S v_j - e_j v_j|_i     <= u32 ((|S| |u_j|)_i + |lambda_j| |u_ij|) + s
What the Jacobi solver answers is held to the same eigenvalue, eigenvector and residual bounds with
    s = (C n 2^-53 + JACOBI_TOL) (||S||_2 + mu),
mu the Gershgorin shift of k_jacobi_eig recomputed from the input and JACOBI_TOL = 1e-12 the solver's own rotation threshold (dense.hip
`tol`: an off-diagonal of the Gram matrix of S + mu I that stays below tol sqrt(g_pp g_qq) turns a vector by at most
tol (||S|| + mu) / gap).  Its vectors are the columns of a product of rotations, whatever the gaps, so orthonormality gets the gap-free
    |(V^T V - I)_jk| <= 2 u32 min(1, sum_i m_ij m_ik) + u32^2 + 2 (C n 2^-53 + JACOBI_TOL).
Exact multiplicities (`clusters`: reference eigenvalues closer than CLUSTER ||S||_2; the cases have gaps >= SEPARATED ||S||_2 or exact
multiplicities and nothing between) have no single reference vector.  There the envelope m_ij = sqrt(P_ii) stands for |u_ij| (P the
reference's projector on the cluster's space: |w_ij| <= sqrt(P_ii) for every orthonormal basis W of it), gap_j is the cluster's distance
from the rest of the spectrum, orthonormality is gap-free as above, and instead of single vectors the projector is compared: with
r_i = u32 sqrt(P_ii) + sqrt(m) s / gap (m the multiplicity; the rows of V_c - W),
    |(V_c V_c^T - P)_ik| <= r_i sqrt(P_kk) + r_k sqrt(P_ii) + r_i r_k.

C is measured, not chosen: the worst disagreement in these units (eigenvalues / unit, vector entries gap / unit) between the three fp64
LAPACK drivers evd, evr and evx over all matrices of the case list (`driver_figures`), C = MARGIN max(1, that) rounded up to a power
of two, MARGIN = 8 for a backward-stable fp64 solver of another construction.  DRIVER_WORST records the figures;
test_evd_certificate_cpu.py recomputes them, and profiles/evd_certificate.md holds the table.

A separated case that the tridiagonal solver answers has C unit / gap_j <= 2^-27 for every j (`separation`): its bound is the fp32
rounding, not the slack.  (The Jacobi solver's slack carries mu and 1e-12 and exceeds that at n = 2049; it is printed, not required.)

Wrong rules (`wrong_answer`), for the CPU test of the certificate's own teeth: an fp32 solver (LAPACK's ssyevd), one reflector left out of the
back-transformation, one WY block's T taken as diagonal (both on `householder`, a plain restatement of the tridiagonalisation and of the
compact WY back-transformation of evd_tridiag.hip), the lower triangle in place of the upper, two adjacent eigenvalues exchanged, a
vector pair five apart with inner product 5e-7 (inside the solver's own acceptance of 1e-6 and out of reach of its four-neighbour
check), the tail of an nvec < n result shifted by one column.
"""
import os
import re

import numpy as np
import scipy.linalg

U32 = 2.0 ** -24
U64 = 2.0 ** -53
MARGIN = 8.0
JACOBI_TOL = 1e-12      # dense.hip `tol`
SEPARATED = 1e-4        # gaps of a separated case / ||S||_2, at least
CLUSTER = 1e-6          # reference eigenvalues closer than this x ||S||_2 are one eigenvalue (the cases have none between the two)
ROUNDING_ONLY = 2.0 ** -27  # C unit / gap of a separated case, at most
NUM_CUS = 256           # MI355X
QUANTITIES = ("eval", "vec", "proj", "orth", "resid")

# Worst disagreement between scipy.linalg.eigh's drivers evd, evr and evx in float64 over all matrices of the case list, in units of
# n 2^-53 ||S||_2 (eigenvalues) and n 2^-53 ||S||_2 / gap_j (vector entries); scipy 1.15, OpenBLAS, CPU.  driver_figures() recomputes them.
DRIVER_WORST = dict(eval=1.57, vec=0.47)  # both at n = 15; 0.6 and 0.16 at most from n = 31 on
C = float(2.0 ** np.ceil(np.log2(MARGIN * max(1.0, max(DRIVER_WORST.values())))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------------------------
# The constants the cases were built from: name -> (file, line, pattern with one group per value, values).
# test_evd_certificate_cpu.py reads the cited line and fails when the text or the line moved: update the cases, then this table.
# ---------------------------------------------------------------------------------------------------------------------------------
TD, DENSE, ROUTE_HOST = "isle_amd/csrc/evd_tridiag.hip", "isle_amd/csrc/dense.hip", "isle_amd/csrc/route_host.h"
SOURCE = {
    "TD_ROWS": (TD, 29, r"constexpr int TD_ROWS = (\d+);", (256,)),
    "TD_NMAX_BACK": (TD, 30, r"constexpr int TD_NMAX_BACK = (\d+);", (2048,)),
    "TD_P_GSMALL": (TD, 239, r"constexpr int TD_P_GSMALL = (\d+);", (32,)),
    "TD_P_T": (TD, 240, r"constexpr int TD_P_T = (\d+);", (1024,)),
    "TD_P_LDS": (TD, 242, r"constexpr size_t TD_P_LDS = (\d+) \* 1024 - (\d+);", (160, 512)),
    "TD_B_T": (TD, 607, r"constexpr int TD_B_T = (\d+);", (1024,)),
    "TD_WY": (TD, 648, r"constexpr int TD_WY = (\d+);", (4,)),
    "nrow": (TD, 706, r"const int nrow = \(n \+ (\d+)\) & ~(\d+);", (127, 127)),
    "td_range": (TD, 855, r"if \(n < (\d+) \|\| n > TD_NMAX_BACK \|\| n > TD_ROWS \* (\d+)\) return 1;", (3, 16)),
    "CB": (TD, 863, r"int CB = (\d+);", (16,)),
    "CB_rule": (TD, 864, r"while \(CB < (\d+) && \(n \+ CB - 1\) / CB > (\d+)\) CB \*= (\d+);", (64, 32, 2)),
    "small": (TD, 891, r"const bool small = n <= TD_ROWS \* (\d+);", (4,)),
    "wy_blocks": (TD, 989, r"const int nblk = \(n - 2 \+ TD_WY - 1\) / TD_WY;", ()),
    "wy_dma": (TD, 994, r"if \(n & 1\) hipLaunchKernelGGL\(\(td_back_wy_k<4, true, false>\)", ()),
    "accept": (TD, 1026, r"if \(!\(dev <= (1e-6)f\)\) \{", (1e-6,)),
    "jacobi_pad": (DENSE, 1389, r"const int np = \(n \+ (\d+)\) & ~(\d+);", (63, 63)),
    "jacobi_tol": (DENSE, 1422, r"const double tol = (1e-12);", (1e-12,)),
    "route_evd_tridiag": (ROUTE_HOST, 162, r"inline bool route_evd_tridiag\(int n, const RouteEnv& e\) \{ return n >= (\d+) && !e.evd_jacobi; \}", (16,)),
    "route_td_workgroups": (ROUTE_HOST, 377, r"const int ncl_max = \(int\)\(lds_bytes / sizeof\(double\) / \(size_t\)n\) - (\d+);", (2,)),
    "route_td_persist": (ROUTE_HOST, 385, r"return pG <= num_cus && n <= nmax_back && !e.td_chain && !failed;", ()),
    "route_td_back": (ROUTE_HOST, 410, r"return \(nvec \+ (\d+)\) / (\d+) > num_cus / (\d+) && !kc \? TD_BACK_SEQ8 : TD_BACK_SEQ4;", (7, 8, 2)),
}


def source_values(name):
    """The values of SOURCE[name] as the cited line holds them now (AssertionError when the line no longer matches)."""
    path, line, pat, vals = SOURCE[name]
    with open(os.path.join(ROOT, path)) as f:
        text = f.read().split("\n")[line - 1]
    m = re.search(pat, text)
    assert m, "%s:%d no longer reads %r (it reads %r): revisit the cases of tests/evd_certificate.py, then SOURCE" % (path, line, pat, text.strip())
    return tuple(type(v)(g) for g, v in zip(m.groups(), vals))


def _src(name, i=0):
    return SOURCE[name][3][i]


TD_ROWS, TD_NMAX_BACK, TD_P_GSMALL, TD_P_T, TD_B_T, TD_WY = (_src(k) for k in ("TD_ROWS", "TD_NMAX_BACK", "TD_P_GSMALL", "TD_P_T", "TD_B_T", "TD_WY"))
TD_P_LDS = _src("TD_P_LDS", 0) * 1024 - _src("TD_P_LDS", 1)
ACCEPT = _src("accept")


def _cdiv(a, b):
    return -(-a // b)


def route(n, nvec=None, env=None, num_cus=NUM_CUS, failed=False):
    """What k_eig_small does with an n x n matrix under the switches `env` on a device of num_cus CUs, before any data-dependent decision:
    dict(solver "tridiagonal" | "jacobi", form "persistent" | "chain" | None, back "wy" | "seq8" | "seq4" | None, and the sizes the
    kernels derive: pG workgroups and ncl columns per workgroup of td_persist_k, entries per thread of its column phases, CB and
    `small` of the launch chain, row blocks of td_update_symv_k's first launch, WY blocks and the reflectors of the last one, rows
    per thread of td_back_wy_k, dma (LDS-DMA image: even n) and its 1-KiB pieces per reflector, np of the Jacobi solver)."""
    env = env or {}
    nvec = n if nvec is None else max(1, min(nvec, n))
    lo, mult = SOURCE["td_range"][3]
    r = dict(n=n, nvec=nvec, form=None, back=None, np=(n + _src("jacobi_pad")) & ~_src("jacobi_pad", 1))
    tri = n >= _src("route_evd_tridiag") and not env.get("ISLE_EVD_JACOBI")       # route_evd_tridiag
    tri = tri and not (n < lo or n > TD_NMAX_BACK or n > TD_ROWS * mult)             # k_tridiag_eig's own range
    r["solver"] = "tridiagonal" if tri else "jacobi"
    if not tri:
        return r
    ncl_max = TD_P_LDS // 8 // n - _src("route_td_workgroups")                       # route_td_workgroups
    pG = max(TD_P_GSMALL, _cdiv(n, ncl_max)) if ncl_max >= 1 else 1 << 30
    persist = pG <= num_cus and n <= TD_NMAX_BACK and not env.get("ISLE_TD_CHAIN") and not failed  # route_td_persist
    r.update(form="persistent" if persist else "chain", pG=pG, ncl=_cdiv(n, pG), idle_workgroups=max(0, pG - n), per_thread=_cdiv(n, TD_P_T))
    cb, (cmax, per, mul) = _src("CB"), SOURCE["CB_rule"][3]
    while cb < cmax and _cdiv(n, cb) > per:
        cb *= mul
    r.update(CB=cb, small=n <= TD_ROWS * _src("small"), row_blocks=_cdiv(n - 1, TD_ROWS))
    a, b, c = SOURCE["route_td_back"][3]
    if str(env.get("ISLE_TD_BACK", ""))[:1] == "s":                                  # route_td_back (one rank: kc = 0)
        r["back"] = "seq8" if (nvec + a) // b > num_cus // c else "seq4"
    else:
        r["back"] = "wy"
    nref = n - 2
    r.update(wy_blocks=_cdiv(nref, TD_WY), wy_last=nref - TD_WY * (_cdiv(nref, TD_WY) - 1), dma=n % 2 == 0,
             pieces=((n + _src("nrow")) & ~_src("nrow", 1)) // 128, rows_per_thread=_cdiv(n, TD_B_T // 4),
             back_workgroups=_cdiv(nvec, 8 if r["back"] == "seq8" else 4))
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------------------------------------------
def spectrum(kind, n):
    """"lin": lambda_i = 1 + i / n (positive definite, gaps 1 / n); "ind": linspace(1, -1, n) (indefinite, gaps 2 / (n - 1))."""
    return 1.0 + np.arange(n) / float(n) if kind == "lin" else np.linspace(1.0, -1.0, n)


def kind_of(n):
    """Even n below 1024 take the definite spectrum, odd n and the large n (whose gaps it would leave too small, see `separation`) the indefinite one."""
    return "lin" if n % 2 == 0 and n < 1024 else "ind"


_MATS = {}


def _rotated(lam, seed):
    n = len(lam)
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def matrix(key):
    """float32 n x n, Fortran order.  key: ("sep", n) random orthogonal Q with spectrum(kind_of(n), n); ("identity", n); ("zero", n);
    ("mm", n) blockdiag(M, M) with M = ("sep", n / 2): every eigenvalue exactly twice behind a non-trivial tridiagonalisation;
    ("upper", n) = ("sep", n) with its strict lower triangle overwritten by unrelated finite values."""
    if key not in _MATS:
        what, n = key
        if what == "sep":
            S = _rotated(spectrum(kind_of(n), n), 1000 + n).astype(np.float32)
        elif what == "identity":
            S = np.eye(n, dtype=np.float32)
        elif what == "zero":
            S = np.zeros((n, n), np.float32)
        elif what == "mm":
            M = matrix(("sep", n // 2))
            S = np.zeros((n, n), np.float32)
            S[:n // 2, :n // 2] = M
            S[n // 2:, n // 2:] = M
        else:
            assert what == "upper"
            S = np.triu(matrix(("sep", n))) + np.tril(np.random.default_rng(7).uniform(-3.0, 3.0, (n, n)).astype(np.float32), -1)
        _MATS[key] = np.asfortranarray(S, dtype=np.float32)
    return _MATS[key]


def upper(S):
    """float64: the symmetric matrix whose upper triangle is S's."""
    A = np.triu(np.asarray(S, np.float64))
    return A + np.triu(A, 1).T


def gershgorin_shift(A):
    """mu of k_jacobi_eig (dense.hip): the smallest shift >= 0 that Gershgorin's discs show makes A + mu I positive semi-definite."""
    off = np.abs(A).sum(axis=0) - np.abs(np.diag(A))
    return float(max(0.0, (off - np.diag(A)).max())) if A.size else 0.0


_REFS = {}


def reference(key):
    """-> dict(A (float64, from the upper triangle), lam (descending), U, norm2, mu, gap (per eigenvalue: to the nearest eigenvalue outside
    its cluster), clusters [(first, last + 1)], env (n x n: |u_ij|, or sqrt(P_ii) for the members of a cluster)).  Cached."""
    if key not in _REFS:
        A = upper(matrix(key))
        n = A.shape[0]
        w, U = scipy.linalg.eigh(A, driver="evd")
        lam, U = w[::-1].copy(), np.ascontiguousarray(U[:, ::-1])
        norm2 = float(np.abs(lam).max())
        cl, first = [], 0
        for i in range(1, n + 1):
            if i == n or lam[i - 1] - lam[i] > CLUSTER * norm2:
                cl.append((first, i))
                first = i
        gap, env = np.empty(n), np.abs(U)
        for a, b in cl:
            g = min(lam[a - 1] - lam[a] if a > 0 else np.inf, lam[b - 1] - lam[b] if b < n else np.inf)
            gap[a:b] = g
            if b - a > 1:
                env[:, a:b] = np.sqrt(np.sum(U[:, a:b] ** 2, axis=1))[:, None]
        _REFS[key] = dict(A=A, lam=lam, U=U, norm2=norm2, mu=gershgorin_shift(A), gap=gap, clusters=cl, env=env, n=n)
    return _REFS[key]


def slack(ref, solver):
    """s of the module docstring: what a backward-stable fp64 solver of this kind may differ by, on the scale of the eigenvalues."""
    n = ref["n"]
    if solver == "jacobi":
        return (C * n * U64 + JACOBI_TOL) * (ref["norm2"] + ref["mu"])
    return C * n * U64 * ref["norm2"]


def separation(ref, solver="tridiagonal"):
    """-> (smallest gap / ||S||_2, largest slack / gap): a separated case has the first >= SEPARATED; the second <= 2^-27 makes the bound the fp32 rounding."""
    g = ref["gap"].min()
    return float(g / ref["norm2"]) if ref["norm2"] > 0 else np.inf, float(slack(ref, solver) / g)


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)  # an exact answer is inside a bound of zero
    return float(q.max())


def ratios(key, evals, vecs, solver, nvec=None):
    """error / bound of every quantity for the answer (evals: n values descending, vecs: n x nvec) of the solver `solver` ("tridiagonal" |
    "jacobi": which slack applies) against reference(key) -> dict over QUANTITIES plus "tail" (True when evals[nvec:] is as documented:
    zeros from the tridiagonal solver, the remaining eigenvalues inside their bound from the Jacobi solver)."""
    ref = reference(key)
    n, lam, U, A = ref["n"], ref["lam"], ref["U"], ref["A"]
    e = np.asarray(evals, np.float64)
    V = np.asarray(vecs, np.float64)
    k = n if nvec is None else nvec
    assert e.shape == (n,) and V.shape == (n, k)
    s = slack(ref, solver)
    clustered = any(b - a > 1 for a, b in ref["clusters"])
    assert all(b <= k or a >= k for a, b in ref["clusters"]), "nvec cuts through a cluster"
    eb = U32 * np.abs(lam) + s
    out = dict(eval=_ratio(np.abs(e[:k] - lam[:k]), eb[:k]))
    out["tail"] = bool(np.all(e[k:] == 0.0)) if solver == "tridiagonal" else bool(_ratio(np.abs(e[k:] - lam[k:]), eb[k:]) <= 1.0)
    M = ref["env"][:, :k]
    with np.errstate(divide="ignore", invalid="ignore"):
        sg = np.where(np.isinf(ref["gap"][:k]), 0.0, s / ref["gap"][:k])
    B = U32 * M + sg[None, :]
    vec, proj = 0.0, 0.0
    for a, b in ref["clusters"]:
        if a >= k:
            break
        if b - a == 1:
            u, v = U[:, a], V[:, a]
            sign = 1.0 if float(v @ u) >= 0.0 else -1.0
            vec = max(vec, _ratio(np.abs(sign * v - u), B[:, a]))
        else:
            p = M[:, a]  # sqrt(P_ii)
            r = U32 * p + np.sqrt(b - a) * sg[a]
            bound = r[:, None] * p[None, :] + p[:, None] * r[None, :] + r[:, None] * r[None, :]
            proj = max(proj, _ratio(np.abs(V[:, a:b] @ V[:, a:b].T - U[:, a:b] @ U[:, a:b].T), bound))
    out.update(vec=vec, proj=proj)
    G = np.abs(V.T @ V - np.eye(k))
    if solver == "jacobi" or clustered:
        ob = 2.0 * U32 * np.minimum(1.0, M.T @ M) + U32 ** 2 + 2.0 * (C * n * U64 + (JACOBI_TOL if solver == "jacobi" else 0.0))
    else:
        MB = M.T @ B
        ob = MB + MB.T + B.T @ B
    out["orth"] = _ratio(G, ob)
    rb = U32 * (np.abs(A) @ M + np.abs(lam[:k])[None, :] * M) + s
    out["resid"] = _ratio(np.abs(A @ V - V * e[:k][None, :]), rb)
    return out


def worst(r):
    return max(r[q] for q in QUANTITIES)


def certify(key, evals, vecs, solver, nvec=None, what=""):
    """Every quantity inside its bound, the tail of evals as documented.  -> the ratios."""
    r = ratios(key, evals, vecs, solver, nvec)
    bad = {q: r[q] for q in QUANTITIES if not r[q] <= 1.0}
    assert not bad, "%s %s: outside the fp64 certificate, error / bound: %s" % (key, what, ", ".join("%s %.3g" % kv for kv in sorted(bad.items())))
    assert r["tail"], "%s %s: evals[nvec:] is not what the %s solver documents" % (key, what, solver)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# C: the three fp64 LAPACK drivers against each other
# ---------------------------------------------------------------------------------------------------------------------------------
def driver_figures(key):
    """-> dict(eval, vec): the worst disagreement between the drivers evd, evr and evx on a separated matrix, in units of n 2^-53 ||S||_2
    and n 2^-53 ||S||_2 / gap_j."""
    ref = reference(key)
    assert all(b - a == 1 for a, b in ref["clusters"])
    A, n = ref["A"], ref["n"]
    unit = n * U64 * ref["norm2"]
    res = [(ref["lam"], ref["U"])]
    for d in ("evr", "evx"):
        w, Z = scipy.linalg.eigh(A, driver=d)
        res.append((w[::-1], Z[:, ::-1]))
    fe = fv = 0.0
    for i in range(3):
        for j in range(i + 1, 3):
            (wa, Ua), (wb, Ub) = res[i], res[j]
            sg = np.where(np.sum(Ua * Ub, axis=0) >= 0.0, 1.0, -1.0)
            fe = max(fe, float(np.abs(wa - wb).max() / unit))
            fv = max(fv, float((np.abs(Ua - Ub * sg) * ref["gap"][None, :]).max() / unit))
    return dict(eval=fe, vec=fv)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _case(name, group, key, nvec=None, env=None, solver="tridiagonal", form=None, back="wy", edge=None, rejected=False):
    n = key[1]
    if solver == "jacobi" and not rejected:
        form = back = None
    return dict(name=name, group=group, key=key, n=n, nvec=nvec, env=dict(env or {}), edge=edge, rejected=rejected,
                expect=dict(solver=solver, form=form, back=back))


def _cases():
    out = []
    # persistent form: both sides of every edge of td_persist_k, td_back_wy_k, td_wy_T_k (n even: the LDS-DMA image)
    edges = {16: "the first size routed to the tridiagonal solver; workgroups of td_persist_k that own no column",
             17: "(n - 2) % 4 = 3, odd n: no LDS-DMA", 18: "(n - 2) % 4 = 0", 19: "(n - 2) % 4 = 1, odd n", 20: "(n - 2) % 4 = 2",
             31: "n < TD_P_GSMALL: a workgroup without a column", 33: "n > TD_P_GSMALL: a second column in workgroup 0",
             128: "one 1-KiB piece per reflector of the LDS-DMA image", 129: "two pieces' worth of rows, odd n: read from memory", 130: "two pieces",
             257: "one row block of td_update_symv_k; the second row per thread of td_back_wy_k", 258: "two row blocks",
             512: "CB = 16", 513: "CB = 32", 1024: "one entry per thread of td_persist_k; small; CB = 32", 1025: "a second entry per thread; not small; CB = 64",
             2041: "the largest n the persistent form holds on 256 CUs"}
    for n in sorted(edges):
        out.append(_case("persist-%d" % n, "persistent", ("sep", n), form="persistent", edge=edges[n]))
    for n in (16, 257, 258, 512, 513, 1024, 1025):
        out.append(_case("chain-%d" % n, "chain", ("sep", n), env={"ISLE_TD_CHAIN": "1"}, form="chain", edge="ISLE_TD_CHAIN=1"))
    for n in (2042, 2048):
        out.append(_case("chain-%d" % n, "chain", ("sep", n), form="chain", edge="beyond the LDS of 256 workgroups: the launch chain by route"))
    for n in (33, 1025):
        for bar in ("default", "hier", "flat"):
            out.append(_case("bar-%s-%d" % (bar, n), "barrier", ("sep", n), env={} if bar == "default" else {"ISLE_TD_BAR": bar}, form="persistent",
                             edge="grid barrier %s" % bar))
    out.append(_case("seq-1024", "seq", ("sep", 1024), env={"ISLE_TD_BACK": "seq"}, form="persistent", back="seq4", edge="128 workgroups of eight: four per workgroup"))
    out.append(_case("seq-1025", "seq", ("sep", 1025), env={"ISLE_TD_BACK": "seq"}, form="persistent", back="seq8", edge="129 workgroups of eight"))
    out.append(_case("seq-1025-nvec5", "seq", ("sep", 1025), nvec=5, env={"ISLE_TD_BACK": "seq"}, form="persistent", back="seq4", edge="a ragged workgroup of four"))
    for n in (130, 1025):
        for nv in (1, 63, 64, 65, n - 1):
            out.append(_case("nvec-%d-%d" % (n, nv), "nvec", ("sep", n), nvec=nv, form="persistent", edge="nvec < n"))
    for n in (63, 64, 65):
        out.append(_case("jacobi-%d" % n, "jacobi", ("sep", n), env={"ISLE_EVD_JACOBI": "1"}, solver="jacobi", edge="ISLE_EVD_JACOBI=1 at the 64-padding"))
    for n in (2, 15, 2049):
        out.append(_case("jacobi-%d" % n, "jacobi", ("sep", n), solver="jacobi", edge="outside the tridiagonal solver's range: Jacobi by route"))
    for what in ("identity", "zero", "mm"):
        out.append(_case("reject-%s" % what, "reject", (what, 64), solver="jacobi", form="persistent", rejected=True, edge="exact multiplicities: the tridiagonal solver must reject itself"))
    out.append(_case("upper-130", "upper", ("upper", 130), form="persistent", edge="the strict lower triangle holds unrelated values"))
    out.append(_case("upper-130-jacobi", "upper", ("upper", 130), env={"ISLE_EVD_JACOBI": "1"}, solver="jacobi", edge="the same in the Jacobi solver"))
    return out


CASES = {c["name"]: c for c in _cases()}
SEPARATED_KEYS = sorted({c["key"] for c in CASES.values() if c["key"][0] in ("sep", "upper")}, key=lambda k: (k[1], k[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# wrong rules
# ---------------------------------------------------------------------------------------------------------------------------------
def householder(A):
    """The tridiagonalisation of evd_tridiag.hip in plain fp64: reflector j (v = [1, x], tau) zeroes column j below its subdiagonal
    (the formulas of td_step_dev).  -> (d, e, [(v_j over the rows j + 1 .., tau_j)] for j = 0 .. n - 3)."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    d, e, refl = np.zeros(n), np.zeros(n - 1), []
    for j in range(n - 1):
        d[j] = A[j, j]
        x = A[j + 1:, j].copy()
        alpha, nrm2 = x[0], float(x[1:] @ x[1:])
        beta, tau, v = alpha, 0.0, np.zeros_like(x)
        v[0] = 1.0
        if nrm2 > 0.0:
            beta = -np.copysign(np.sqrt(alpha * alpha + nrm2), alpha)
            tau = (beta - alpha) / beta
            v[1:] = x[1:] / (alpha - beta)
        e[j] = beta
        if j < n - 2:
            refl.append((v, tau))
            B = A[j + 1:, j + 1:]
            p = tau * (B @ v)
            w = p - 0.5 * tau * (p @ v) * v
            B -= np.outer(v, w) + np.outer(w, v)
    d[n - 1] = A[n - 1, n - 1]
    return d, e, refl


def back_transform(refl, Z, n, skip=None, diagonal_T=None):
    """Z <- H_0 ... H_{n-3} Z by blocks of TD_WY reflectors in compact WY form (td_wy_T_k, td_back_wy_k).  skip: a reflector left out;
    diagonal_T: a block whose T is taken as diag(tau)."""
    Z = np.array(Z, np.float64)
    nref = len(refl)
    for b in range(_cdiv(nref, TD_WY) - 1, -1, -1):
        js = [j for j in range(TD_WY * b, min(nref, TD_WY * (b + 1))) if j != skip]
        Vb = np.zeros((n, len(js)))
        taus = []
        for c, j in enumerate(js):
            Vb[j + 1:, c] = refl[j][0]
            taus.append(refl[j][1])
        T = np.zeros((len(js), len(js)))
        for i in range(len(js)):
            T[i, i] = taus[i]
            if i and diagonal_T != b:
                T[:i, i] = -taus[i] * (T[:i, :i] @ (Vb[:, :i].T @ Vb[:, i]))
        Z -= Vb @ (T @ (Vb.T @ Z))
    return Z


def restated_answer(key, skip=None, diagonal_T=None):
    """The tridiagonal solver's answer from the plain restatement, rounded to float32 once (eigenpairs of T by LAPACK in fp64)."""
    ref = reference(key)
    d, e, refl = householder(ref["A"])
    w, Z = scipy.linalg.eigh_tridiagonal(d, e)
    V = back_transform(refl, Z[:, ::-1], ref["n"], skip=skip, diagonal_T=diagonal_T)
    return w[::-1].astype(np.float32), V.astype(np.float32)


def rounded_reference(key, nvec=None):
    """The reference itself rounded to float32: the best answer there is."""
    ref = reference(key)
    k = ref["n"] if nvec is None else nvec
    e = ref["lam"].astype(np.float32)
    if nvec is not None:
        e[k:] = 0.0
    return e, ref["U"][:, :k].astype(np.float32)


def wrong_answer(rule, key, nvec=None):
    """-> (evals, vecs) of a solver that is wrong by `rule` (module docstring)."""
    ref = reference(key)
    n = ref["n"]
    if rule == "fp32_solver":
        # LAPACK's ssyevd through scipy: float32 throughout (numpy.linalg.eigh widens a float32 matrix to double inside and is no fp32 solver)
        w, Z = scipy.linalg.eigh(matrix(key), driver="evd", lower=False)
        assert w.dtype == np.float32 and Z.dtype == np.float32
        return w[::-1].copy(), Z[:, ::-1].copy()
    if rule == "reflector_left_out":
        return restated_answer(key, skip=n - 3)  # the last one: two rows
    if rule == "diagonal_T":
        return restated_answer(key, diagonal_T=_cdiv(n - 2, TD_WY) // 2)
    if rule == "lower_triangle":
        S = matrix(key).astype(np.float64)
        w, Z = scipy.linalg.eigh(np.tril(S) + np.tril(S, -1).T, driver="evd")
        return w[::-1].astype(np.float32), Z[:, ::-1].astype(np.float32)
    e, V = rounded_reference(key, nvec)
    if rule == "exchanged_eigenvalues":
        e[[n // 2, n // 2 + 1]] = e[[n // 2 + 1, n // 2]]
    elif rule == "pair_five_apart":
        V = V.astype(np.float64)
        j = n // 3
        V[:, j + 5] += 5e-7 * V[:, j]
        V = V.astype(np.float32)
    else:
        assert rule == "tail_shifted" and nvec is not None
        U = ref["U"]
        V[:, nvec // 2:] = U[:, nvec // 2 + 1:nvec + 1].astype(np.float32)
    return e, V
