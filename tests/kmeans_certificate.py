"""fp64 certificates of the k-means steps (no GPU; numpy + scipy.sparse).

Every document of an assignment and every entry of a centroid step is held against a plain fp64 evaluation of the same step:

- certify_assignment: the label of every document is the fp64 arg-min up to the slack E(x) = ISLE_SLACK_REL (|b|^2 + |C_x|^2) that
  every fp32 squared distance of the library is allowed (isle_amd/csrc/hamerly.h), at most max(3, 3e-4 D) documents are off the
  fp64 arg-min at all, and bit-identical centres obey the reference's tie rule (cblas_isamin: the first index of the minimum).
- certify_centroids: every non-empty centre is the fp64 mean of its members to within the rounding of a sum of n_c terms plus the
  drift of sums kept up to date by the m_c documents that moved; an empty cluster's centre is exactly zero (the reference clears the
  centres with memset and rescales only the non-empty ones).
- certify_gemm: every entry of an fp32 product is the fp64 product to within (K + 2) 2^-24 (|A| |B|)_ij.

Points: a dense (D, dim) array of fp64 rows (the projection B^T U, U the fp32 values the device holds) or a scipy.sparse (V, D)
matrix whose columns are the documents (Lloyd on B).  Centres: (k, dim) rows.  Each checker raises AssertionError with the worst
offender and returns a dict of what it measured.
"""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.sparse as sp

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_F32 = 2.0 ** -24


def _header_slack():
    text = open(os.path.join(_ROOT, "isle_amd", "csrc", "hamerly.h")).read()
    m = re.search(r"#define\s+ISLE_SLACK_REL\s+([0-9.]+(?:[eE][-+]?[0-9]+)?)[fF]?", text)
    assert m, "ISLE_SLACK_REL not found in hamerly.h"
    return float(np.float32(float(m.group(1))))


ISLE_SLACK_REL = _header_slack()
_THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
_BLOCK_ELEMS = 1 << 22  # documents x centres per block of fp64 distances


def csc_points(B):
    """The documents of a CSC dict (V, D, vals, rows, offs) as a scipy.sparse (V, D) fp64 matrix."""
    return sp.csc_matrix((np.asarray(B["vals"], np.float64), np.asarray(B["rows"], np.int64), np.asarray(B["offs"], np.int64)),
                         shape=(int(B["V"]), len(B["offs"]) - 1))


def _rows(X):
    """documents as rows: dense fp64 (D, dim) or CSR (D, V)."""
    if sp.issparse(X):
        return X.T.tocsr().astype(np.float64)
    return np.asarray(X, np.float64)


def _sq_norms(Xr):
    if sp.issparse(Xr):
        return np.asarray(Xr.multiply(Xr).sum(axis=1)).ravel()
    return np.einsum("ij,ij->i", Xr, Xr)


def _blocked(fn, D, k):
    """fn(d0, d1) over blocks of documents, on the host's threads (the products release the GIL)."""
    step = max(256, _BLOCK_ELEMS // max(k, 1))
    spans = [(d0, min(D, d0 + step)) for d0 in range(0, D, step)]
    with ThreadPoolExecutor(_THREADS) as ex:
        return list(ex.map(lambda s: fn(*s), spans))


def fp64_distances_argmin(X, C, xn2=None):
    """-> (dist (D, k) fp64 squared distances, xn2, cn2)."""
    Xr = _rows(X)
    C64 = np.asarray(C, np.float32).astype(np.float64)
    CT = np.ascontiguousarray(C64.T)
    cn2 = np.einsum("ij,ij->i", C64, C64)
    xn2 = _sq_norms(Xr) if xn2 is None else np.asarray(xn2, np.float64)
    D, k = Xr.shape[0], C64.shape[0]

    def blk(d0, d1):
        G = Xr[d0:d1] @ CT
        return np.maximum((xn2[d0:d1, None] + cn2[None, :]) - 2.0 * np.asarray(G), 0.0)

    dist = np.concatenate(_blocked(blk, D, k), axis=0) if D else np.zeros((0, k))
    return dist, xn2, cn2


def certify_assignment(X64, xn2, C, assign, what="", near_ties=False):
    """assign (D,) against the fp32 centres C (k, dim) it was computed with.  The gap of the chosen centre c over the fp64 arg-min c*
    must be within E(c) + E(c*); the number of documents off the arg-min within max(3, 3e-4 D); no document may carry the label of a
    centre whose bits equal those of a lower-numbered one.  near_ties: a start built to hold many near-ties (centres placed on documents,
    twins and copies) also allows every document whose fp64 runner-up is within E of its best.  -> dict(max_ratio (largest gap / (E(c) + E(c*))), off, D)."""
    C = np.asarray(C, np.float32)
    assign = np.asarray(assign).astype(np.int64)
    dist, xn2, cn2 = fp64_distances_argmin(X64, C, xn2)
    D, k = dist.shape
    assert assign.shape == (D,), (assign.shape, D)
    assert D == 0 or (assign.min() >= 0 and assign.max() < k), "labels out of range %s" % what
    best = np.argmin(dist, axis=1)  # first index of the minimum
    rows = np.arange(D)
    gap = dist[rows, assign] - dist[rows, best]
    E = ISLE_SLACK_REL * (xn2 + cn2[assign]) + ISLE_SLACK_REL * (xn2 + cn2[best])
    ratio = np.where(gap > 0, gap / np.maximum(E, 1e-300), 0.0)
    worst = int(np.argmax(ratio)) if D else 0
    assert D == 0 or ratio[worst] <= 1.0, ("%s document %d labelled %d, fp64 arg-min %d: d = %.9g vs %.9g, gap %.3g > E(c) + E(c*) = %.3g"
                                           % (what, worst, assign[worst], best[worst], dist[worst, assign[worst]], dist[worst, best[worst]],
                                              gap[worst], E[worst]))
    off = int((assign != best).sum())
    allowed = max(3, int(3e-4 * D))
    if near_ties and k > 1:
        two = np.argpartition(dist, 1, axis=1)[:, :2]
        d2 = np.take_along_axis(dist, two, axis=1)
        c2 = two[rows, np.argmax(d2, axis=1)]
        allowed += int((d2.max(1) - d2.min(1) <= ISLE_SLACK_REL * (2 * xn2 + cn2[best] + cn2[c2])).sum())
    assert off <= allowed, "%s %d of %d documents off the fp64 arg-min (allowed %d)" % (what, off, D, allowed)
    # exact tie rule: the first of bit-identical centres takes the documents
    _, first = np.unique(C.view(np.uint32).reshape(k, -1), axis=0, return_index=True)
    _, inv = np.unique(C.view(np.uint32).reshape(k, -1), axis=0, return_inverse=True)
    lowest = first[inv.ravel()]
    bad = np.flatnonzero(lowest[assign] != assign)
    assert bad.size == 0, ("%s %d documents labelled with a centre bit-identical to a lower-numbered one, e.g. document %d labelled %d (twin %d)"
                           % (what, bad.size, bad[0], assign[bad[0]], lowest[assign[bad[0]]]))
    return dict(max_ratio=float(ratio[worst]) if D else 0.0, off=off, D=D)


def moves_since_first(assigns, k):
    """m_c: the documents that entered or left cluster c, summed over the steps of a trajectory of assignments."""
    m = np.zeros(k, np.int64)
    for a, b in zip(assigns[:-1], assigns[1:]):
        a = np.asarray(a, np.int64)
        b = np.asarray(b, np.int64)
        mv = a != b
        m += np.bincount(a[mv], minlength=k) + np.bincount(b[mv], minlength=k)
    return m


def certify_centroids(X64, assign, assign_prev, C_out, X_abs=None, X_err=None, frob_tol=1e-6, what=""):
    """C_out (k, dim) fp32, the centroid step of the assignment assign.  assign_prev: the assignments of the earlier iterations, from the
    first on (a list, possibly empty; or one array), from which m_c is counted.  Non-empty centre c, every entry j:
    |C_out - mean64| <= (n_c + m_c + 2) 2^-24 sum_{d in c} |x_dj| / n_c; over all non-empty centres the Frobenius relative error <= frob_tol;
    empty centres exactly zero.  X_abs (same shape as X64): magnitudes to sum instead of |x| — for the projection, |B|^T |U|, the scale of
    the rounding of its sums.  X_err (D, dim): an absolute error the points themselves may carry on the device, added as sum_{d in c} X_err / n_c —
    for the projection, (nnz_d + 1) 2^-24 (|B|^T |U|)_d, the rounding of the device's fp32 projection of each document.  -> dict(max_ratio, frob, empty)."""
    Xr = _rows(X64)
    Ar = Xr if X_abs is None else _rows(X_abs)
    C_out = np.asarray(C_out, np.float32)
    k = C_out.shape[0]
    assign = np.asarray(assign, np.int64)
    D = assign.shape[0]
    if assign_prev is None:
        prev = []
    elif isinstance(assign_prev, np.ndarray) and assign_prev.ndim == 1:
        prev = [assign_prev]
    else:
        prev = list(assign_prev)
    m = moves_since_first(prev + [assign], k)
    n = np.bincount(assign, minlength=k)
    onehot = sp.csr_matrix((np.ones(D), (assign, np.arange(D))), shape=(k, D))
    S = onehot @ Xr
    A = onehot @ (abs(Ar) if sp.issparse(Ar) else np.abs(Ar))
    S = S.toarray() if sp.issparse(S) else np.asarray(S)
    A = A.toarray() if sp.issparse(A) else np.asarray(A)
    live = n > 0
    mean = np.zeros_like(S)
    mean[live] = S[live] / n[live, None]
    gamma = (n + m + 2) * U_F32
    bound = np.zeros_like(A)
    bound[live] = gamma[live, None] * A[live] / n[live, None]
    if X_err is not None:
        bound[live] += np.asarray(onehot @ np.asarray(X_err, np.float64))[live] / n[live, None]
    err = np.abs(C_out.astype(np.float64) - mean)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    ratio[~live] = 0.0
    c, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[c, j] <= 1.0, ("%s centre %d (n_c %d, m_c %d) entry %d: %.9g against the fp64 mean %.9g, bound %.3g"
                                % (what, c, n[c], m[c], j, C_out[c, j], mean[c, j], bound[c, j]))
    nz = np.flatnonzero(~live)
    dirty = [int(e) for e in nz if np.any(C_out[e].view(np.uint32) != 0)]
    assert not dirty, "%s empty cluster %d has a centre that is not exactly zero (max |x| %.3g)" % (what, dirty[0], np.abs(C_out[dirty[0]]).max())
    den = np.linalg.norm(mean[live])
    frob = float(np.linalg.norm(C_out[live].astype(np.float64) - mean[live]) / den) if den > 0 else 0.0
    assert frob <= frob_tol, "%s Frobenius relative error of the centres %.3g > %.3g" % (what, frob, frob_tol)
    return dict(max_ratio=float(ratio[c, j]), frob=frob, empty=int(nz.size))


def certify_gemm(A, B, C_gpu, what=""):
    """C_gpu (M, N) fp32 = A (M, K) B (K, N) from fp32 operands: |C - C64| <= (K + 2) 2^-24 (|A| |B|)_ij entry by entry."""
    A64 = np.asarray(A, np.float32).astype(np.float64)
    B64 = np.asarray(B, np.float32).astype(np.float64)
    K = A64.shape[1]
    C64 = A64 @ B64
    bound = (K + 2) * U_F32 * (np.abs(A64) @ np.abs(B64))
    err = np.abs(np.asarray(C_gpu, np.float64) - C64)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else (0, 0)
    assert ratio.size == 0 or ratio[i, j] <= 1.0, ("%s entry (%d, %d) of %s: %.9g against %.9g, bound %.3g"
                                                   % (what, i, j, C64.shape, C_gpu[i, j], C64[i, j], bound[i, j]))
    return dict(max_ratio=float(ratio[i, j]) if ratio.size else 0.0)


# Float centroid sums of a row-constant B (the gather form of the operator on such a B: forced by ISLE_GRAM_LDS=0, or agreed by the ranks
# when a shard is empty): a centre entry is a sum of n_c copies of one value, whose fp32 roundings do not cancel.  The reference's own
# sequential fp32 sums reach a Frobenius relative error of 1.0 - 1.6e-6 there (tests/test_kmeans_certificate_cpu.py: the oracle on the same
# corpus); the library's float sums 1.1 - 1.3e-6.  The per-entry bound holds unchanged; the typical-level bound is the reference's level
# with a margin.
FLOAT_SUMS_ROW_CONSTANT_FROB = 4e-6


def certify_kmeanspp(c, g, md):
    """k-means++ with injected seeds.  c: the fp64 side of the case (k, B["X"], U, P64, pn2, seeds); g: seeds and C_lowd as returned; md:
    get_min_dist() of all documents.  C_lowd = P[seeds] within the product bound; md per document within E = ISLE_SLACK_REL (|p_d|^2 +
    max_s |p_s|^2) of the fp64 minimum over the seeds folded in (the last batch of the rounds never is: src/sparseMatrix.cpp:2163-2207).
    -> (d, E): the fp64 minima and their allowances, or None where nothing is folded in."""
    k, B = c.k, c.B
    assert np.array_equal(g["seeds"], c.seeds)
    Bs = B["X"][:, c.seeds.astype(np.int64)].T.toarray()
    certify_gemm(Bs, c.U, g["C_lowd"], what="k-means++ seeds k=%d:" % k)
    s, last = 1, 0
    while s < k:
        nd = 0
        while nd < 1 + np.sqrt(max(s - 5, 0)):
            nd += 1
        last = min(nd, k - s)
        s += last
    folded = c.seeds[:k - last].astype(np.int64)
    if folded.size == 0 or k == 1:
        return None
    Ps = c.P64[folded]
    d = np.maximum(c.pn2[:, None] + np.einsum("ij,ij->i", Ps, Ps)[None, :] - 2.0 * (c.P64 @ Ps.T), 0.0).min(axis=1)
    E = ISLE_SLACK_REL * (c.pn2 + c.pn2[folded].max())
    bad = np.flatnonzero(np.abs(np.asarray(md, np.float64) - d) > E)
    assert bad.size == 0, ("k=%d: min_dist of document %d is %.9g, fp64 %.9g, E %.3g" % (k, bad[0], md[bad[0]], d[bad[0]], E[bad[0]]))
    return d, E
