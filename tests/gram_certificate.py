"""fp64 certificates of the Gram apply Z = B (B^T X) (no GPU; numpy + scipy.sparse).

Every entry of a Gram apply is held against the fp64 product of the same fp32 inputs, in one of two ways:

- certify_gram: |Z - Z64|[w, j] <= (n_w + max_{d ∋ w} n_d + 2) u M[w, j], u = 2^-24, M = |B| (|B|^T |X|), n_w the entries of word
  (row) w, n_d the entries of document (column) d.  The bound holds for any order and any tree of the sums.  Derivation: every form
  computes Y_d = sum_{w' ∈ d} B[w', d] X[w', j] with one rounding per product (the banded form: gl_pack_scale_k rounds s_w' X[w', j])
  and n_d - 1 roundings of the additions (FMA: fewer), so |Y^_d - Y_d| <= g(n_d) (|B|^T |X|)_d with g(k) = k u / (1 - k u) (Higham,
  Accuracy and Stability, 3.1 / 3.5).  Then Z_w = sum_{d ∋ w} B[w, d] Y^_d: one rounding per product (the banded form: sums the n_w
  terms Y^_d first and multiplies by s_w once in gl_reduce_cm_k — still n_w roundings in all), n_w - 1 for the additions, so
  |Z^_w - Z_w| <= g(n_w) |B| |Y^| + |B| |Y^ - Y| <= ((1 + g(n_w))(1 + g(n_d)) - 1) M <= g(n_w + n_d) M.  Finally
  g(k) <= (k + 2) u whenever k^2 u + 2 k u <= 2, i.e. k <= 5790: certify_gram asserts that, and uses n_d = the longest document
  of the word.  An entry with M = 0 (an empty row of B, a zero column of X, a word whose documents see only zeros) must be exactly 0.
- certify_exact: with dyadic inputs every product and every partial sum is a multiple of `quantum` below 2^23 quanta, so fp32
  arithmetic is exact in any order, and Z must equal Z64 bit for bit: a lost, duplicated or misplaced id, a padding slot that reads a
  non-zero row, a wrong scaling shows at any size.  Precondition, asserted: Z64 is a multiple of quantum and M.max() / quantum < 2^22.
  Why that suffices with B in {1/2, 1, 2} and integer X (quantum 1/4): a partial sum of Y_d is a multiple of 1/2 and at most
  (|B|^T |X|)_d <= M[w, j] / s_w <= 2 M[w, j] for any word w of d; a partial sum of Z_w is a multiple of 1/4 (the banded form sums the
  Y_d before the final s_w: multiples of 1/2 up to M / s_w <= 2 M); in quanta of their own both stay below 4 M / (1/4) / 2 < 2^23.

The builders make the dyadic and non-dyadic inputs of the GPU sweep (test_gpu_gram_certified.py) and of the CPU tests
(test_gram_certificate_cpu.py); GRAM_SWEEP is every switch value the GPU test runs, GRAM_EXCLUDED the switches it leaves out and why.
"""
import os

import numpy as np
import scipy.sparse as sp

import route_reads

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_F32 = 2.0 ** -24
GL_RB = 4078  # rows per band of the LDS-banded form (gram_lds.hip GL_RB_V)
GL_VP = 81920  # words per vocabulary part of the build's LDS histograms (gram_lds.hip)
DYADIC_S = (0.5, 1.0, 2.0)
QUANTUM = 0.25  # min |B|^2 x the integer step of X
_BOUND_K_MAX = 5790  # largest n_w + n_d with g(k) <= (k + 2) u

# Every switch of the Gram apply, with the values the GPU sweep runs besides the default.
GRAM_SWEEP = {
    "ISLE_GRAM_LDS": ["0"],                      # gram_lds.hip k_gl_detect: the gather form on row-constant input
    "ISLE_GL_G1": ["4", "5", "6", "7", "8"],     # pass-1 items per lane (8 only by the switch)
    "ISLE_GL_G2": ["4", "5", "6", "7", "8"],     # pass-2 items per lane
    "ISLE_GL_PLACE": ["0"],                      # ids packed in ascending order instead of gl_place_k
    "ISLE_GL_FILL_BUCKETS": ["0"],               # pass-2 stream by the direct scatter
    "ISLE_GL_ROUNDS": ["0"],                     # strided workgroups instead of whole rounds
    "ISLE_GL_COLUMNS": ["0"],                    # pass 2 chunked per word block instead of band columns
    "ISLE_GL_TEST_CUS": ["3", "7"],              # test hook: pass 1 laid out for a device of that many CUs
    "ISLE_CHUNK_COLS": ["64", "997"],            # gather form: columns per chunk (read when a context is created)
}
# Switches that the Gram apply's sources read but that do not take part in the Gram apply.
GRAM_EXCLUDED = {
    "ISLE_GL_PANEL": "columns per pass of the k-wide and thin products; the Gram apply always takes panels of 10 (api.cpp gram_apply_dev)",
    "ISLE_GL_WIDE_GROUPED": "layout of the projection's output (k-wide product), not read by the Gram apply",
    "ISLE_WIDE_GATHER": "selects the form of the k-wide products only",
    "ISLE_WIDE_LDS": "selects the form of the k-wide products only",
    "ISLE_GL_VERBOSE": "prints the build's geometry; no effect on the operator",
    "ISLE_GL_ABLATE_SKIP": "timing experiment whose results are wrong by design",
    "ISLE_CENTERS_FRESH": "centroid counts of Lloyd on B (spmm.hip), not the Gram apply",
}
# The sources of the Gram apply; api.cpp hands the gather form its chunk size (isle_ctx::band_rows) at context creation.
GRAM_SOURCES = ("gram_lds.hip", "spmm.hip")


def gram_switches_read(table_names):
    """Names of the switches the Gram apply reads: every switch GRAM_SOURCES read (route_reads.py), plus every one api.cpp stores in band_rows."""
    src = os.path.join(_ROOT, "isle_amd", "csrc")
    text = "".join(open(os.path.join(src, f)).read() for f in GRAM_SOURCES)
    text += "".join(line for line in open(os.path.join(src, "api.cpp")) if "band_rows" in line)
    return route_reads.switches_read(text, table_names)


def uncovered_gram_switches(table_names, sweep=GRAM_SWEEP, excluded=GRAM_EXCLUDED):
    """Switches the Gram apply reads that are neither swept nor excluded, and swept / excluded names the table does not know."""
    known = set(table_names)
    missing = gram_switches_read(table_names) - set(sweep) - set(excluded)
    stale = (set(sweep) | set(excluded)) - known
    return sorted(missing), sorted(stale)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 product and the certificates
# ---------------------------------------------------------------------------------------------------------------------------------
def csc64(V, vals, rows, offs):
    offs = np.asarray(offs, np.int64)
    return sp.csc_matrix((np.asarray(vals, np.float32).astype(np.float64), np.asarray(rows, np.int64), offs), shape=(int(V), len(offs) - 1))


def gram64(V, vals, rows, offs, X):
    """-> (Z64, M, B): the fp64 product B (B^T X) of the fp32 inputs, M = |B| (|B|^T |X|), B the fp64 scipy matrix."""
    B = csc64(V, vals, rows, offs)
    X64 = np.asarray(X, np.float32).astype(np.float64)
    Z64 = np.asarray(B @ (B.T @ X64))
    A = abs(B)
    M = np.asarray(A @ (A.T @ np.abs(X64)))
    return Z64, M, B


def bound_coeff(B):
    """(n_w + max_{d ∋ w} n_d + 2) per word (0 for an empty row: such a row must be exactly zero anyway)."""
    B = sp.csc_matrix(B)
    nd = np.diff(B.indptr).astype(np.float64)
    R = sp.csr_matrix((nd[B.tocoo().col], (B.tocoo().row, B.tocoo().col)), shape=B.shape)
    nw = np.diff(R.indptr)
    mx = np.zeros(B.shape[0])
    nz = nw > 0
    if R.nnz:
        mx[nz] = np.maximum.reduceat(R.data, R.indptr[:-1][nz])
    return np.where(nz, nw + mx + 2.0, 0.0)


def _worst(ratio, k=5):
    flat = np.argsort(ratio, axis=None)[::-1][:k]
    return [np.unravel_index(i, ratio.shape) for i in flat]


def certify_gram(Z, Z64, M, B, extra=0):
    """Every entry within (n_w + max n_d + 2 + extra) u M of the fp64 product.  extra: roundings beyond those of one rank's sums — N - 1
    for a Z all-reduced over N ranks (each entry is a sum of N partial results, joined by at most N - 1 additions in any order).
    -> {'max_ratio': max |err| / (u M), 'coeff_max': ...}."""
    Z = np.asarray(Z)
    assert Z.shape == Z64.shape, (Z.shape, Z64.shape)
    assert Z.dtype == np.float32, Z.dtype
    coeff = bound_coeff(B)
    coeff = np.where(coeff > 0, coeff + extra, 0.0)
    assert coeff.max(initial=0.0) - 2 <= _BOUND_K_MAX, "bound needs n_w + n_d <= %d (got %d)" % (_BOUND_K_MAX, coeff.max() - 2)
    err = np.abs(Z.astype(np.float64) - Z64)
    uM = U_F32 * M
    ratio = np.where(uM > 0, err / np.where(uM > 0, uM, 1.0), np.where(err > 0, np.inf, 0.0))
    bad = ratio > coeff[:, None]
    if bad.any():
        rep = ["Z[%d, %d] = %r vs fp64 %r: |err| / (u M) = %.4g > bound %g" % (w, j, float(Z[w, j]), float(Z64[w, j]), ratio[w, j], coeff[w])
               for (w, j) in _worst(np.where(bad, ratio, -1.0))]
        raise AssertionError("%d entries outside the fp32 bound:\n  %s" % (int(bad.sum()), "\n  ".join(rep)))
    return {"max_ratio": float(ratio.max(initial=0.0)), "coeff_max": float(coeff.max(initial=0.0)),
            "max_ratio_over_coeff": float((ratio / np.where(coeff > 0, coeff, 1.0)[:, None]).max(initial=0.0))}


def certify_exact(Z, Z64, M, quantum=QUANTUM):
    """Bit-equal to the fp64 product, under the precondition that makes fp32 exact in any order."""
    Z = np.asarray(Z)
    assert Z.dtype == np.float32, Z.dtype
    assert float(M.max(initial=0.0)) / quantum < 2.0 ** 22, "precondition: M.max() / quantum = %g >= 2^22" % (M.max() / quantum)
    assert np.all(np.mod(Z64, quantum) == 0), "precondition: the fp64 product is not a multiple of the quantum"
    bad = Z.astype(np.float64) != Z64
    if bad.any():
        err = np.abs(Z.astype(np.float64) - Z64)
        rep = ["Z[%d, %d] = %r vs fp64 %r (M %g)" % (w, j, float(Z[w, j]), float(Z64[w, j]), M[w, j]) for (w, j) in _worst(np.where(bad, err, -1.0))]
        raise AssertionError("%d entries not bit-equal to the fp64 product:\n  %s" % (int(bad.sum()), "\n  ".join(rep)))


def certify_structure(Z, B, X):
    """Rows of B without entries and all-zero columns of X give exactly zero rows / columns of Z."""
    Z = np.asarray(Z)
    empty = np.diff(sp.csr_matrix(B).indptr) == 0
    assert not np.any(Z[empty]), "an empty row of B has a non-zero Z row (rows %s)" % np.flatnonzero(empty & np.any(Z != 0, axis=1))[:5]
    zc = ~np.any(np.asarray(X) != 0, axis=0)
    assert not np.any(Z[:, zc]), "a zero column of X has a non-zero Z column (columns %s)" % np.flatnonzero(zc & np.any(Z != 0, axis=0))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def pattern_from_lists(V, cols):
    """CSC pattern (rows u32, offs i64) from per-document lists of word ids."""
    cols = [np.unique(np.asarray(c, np.int64)) for c in cols]
    offs = np.zeros(len(cols) + 1, np.int64)
    offs[1:] = np.cumsum([len(c) for c in cols])
    rows = np.concatenate(cols).astype(np.uint32) if cols else np.zeros(0, np.uint32)
    assert rows.size == 0 or int(rows.max()) < V
    return rows, offs


def pattern_random(V, D, lo, hi, seed, must=()):
    """D documents of lo..hi distinct words drawn uniformly (vectorised: duplicates dropped), plus the words `must` placed in
    documents 0, 1, ... so that those rows are not empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, D)
    W = rng.integers(0, V, (D, hi))
    W[np.arange(hi)[None, :] >= lens[:, None]] = V  # sentinel: no entry
    for i, w in enumerate(must):
        W[i % D, 0] = w
    W.sort(axis=1)
    keep = W < V
    keep[:, 1:] &= W[:, 1:] != W[:, :-1]
    offs = np.zeros(D + 1, np.int64)
    offs[1:] = np.cumsum(keep.sum(axis=1))
    return W[keep].astype(np.uint32), offs


def pattern_ragged(V, D, seed):
    """test_gpu_parity._ragged with words that occur nowhere: documents of 0, 1, 7, 64, 65 and 700 words, document 17 holds every
    word except every 97th, which occurs nowhere."""
    rng = np.random.default_rng(seed)
    live = np.flatnonzero(np.arange(V) % 97 != 96)
    cols = []
    for d in range(D):
        n = [0, 1, 7, 64, 65, 700][d % 6]
        cols.append(live if d == 17 else np.sort(rng.choice(live, size=min(n, live.size), replace=False)))
    return pattern_from_lists(V, cols)


def pattern_place(seed):
    """One word band and one document band (V = D = 4078): words 0..4 occur in 32, 33, 64, 65 and 256 documents, word 5 in all 4078;
    documents 100..103 hold 32, 33, 64 and 65 words (word 5 included).  The slices straddle gl_place_k's 8 super-rounds
    (GL_PLACE_MAXN) and the register sorts' limits (gl_sort2_k / gl_sort2_big_k)."""
    rng = np.random.default_rng(seed)
    V = D = GL_RB
    cols = [[5] for _ in range(D)]
    for w, n in enumerate([32, 33, 64, 65, 256]):
        for d in rng.choice(np.arange(200, D), size=n, replace=False):
            cols[d].append(w)
    for d, n in zip(range(100, 104), [32, 33, 64, 65]):
        cols[d] += list(rng.choice(np.arange(10, V), size=n - 1, replace=False))
    for d in range(104, 200):  # some background so that other words are not empty
        cols[d] += list(rng.choice(np.arange(10, V), size=20, replace=False))
    return pattern_from_lists(V, cols)


def dyadic_row_values(V, rows, seed):
    """row-constant B: s_w from {1/2, 1, 2}."""
    s = np.asarray(DYADIC_S, np.float32)[np.random.default_rng(seed).integers(0, 3, V)]
    return s[np.asarray(rows, np.int64)], s


def dyadic_entry_values(rows, seed):
    """B with per-entry values from {1/2, 1, 2} (rows with two or more entries are not constant, in general)."""
    return np.asarray(DYADIC_S, np.float32)[np.random.default_rng(seed).integers(0, 3, len(rows))]


def sqrt_row_values(V, rows, seed):
    """non-dyadic row-constant B like tools/synth.make_B: s_w = sqrt(idf-like weights)."""
    s = np.sqrt(np.random.default_rng(seed).uniform(0.5, 12.0, V)).astype(np.float32)
    return s[np.asarray(rows, np.int64)], s


def sqrt_entry_values(rows, seed):
    return np.sqrt(np.random.default_rng(seed).uniform(0.5, 12.0, len(rows))).astype(np.float32)


def dyadic_X(V, b, seed, B=None, r=7, zero_cols=()):
    """Small integers in [-r, r], r shrunk (7, 3, 1) until M = |B| (|B|^T |X|) <= r M1 stays under 2^22 quanta."""
    if B is not None:
        A = abs(sp.csc_matrix(B))
        m1 = float(np.max(A @ (A.T @ np.ones(B.shape[0])), initial=0.0))
        for r in [q for q in (7, 3, 1) if q <= r]:
            if r * m1 / QUANTUM < 2.0 ** 22:
                break
        assert r * m1 / QUANTUM < 2.0 ** 22, "no integer X keeps this B exact (M1 = %g)" % m1
    X = np.random.default_rng(seed).integers(-r, r + 1, (V, b)).astype(np.float32)
    X[:, list(zero_cols)] = 0
    return X


def normal_X(V, b, seed, zero_cols=()):
    X = np.random.default_rng(seed).standard_normal((V, b)).astype(np.float32)
    X[:, list(zero_cols)] = 0
    return X
