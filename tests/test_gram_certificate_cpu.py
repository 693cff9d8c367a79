"""The Gram certificate (tests/gram_certificate.py) on the fp32 CPU oracle: the oracle passes it, planted faults of the kinds the banded
form could make fail it, the norm-wise check of the older tests misses a fault it catches, and every switch of the Gram apply is swept
by the GPU test or excluded with a reason."""
import ctypes as C

import numpy as np
import pytest

from gram_certificate import (GL_RB, GRAM_EXCLUDED, GRAM_SWEEP, certify_exact, certify_gram, certify_structure, csc64, dyadic_X,
                              dyadic_entry_values, dyadic_row_values, gram64, normal_X, pattern_place, pattern_random, pattern_ragged,
                              sqrt_row_values, uncovered_gram_switches)
from conftest import relerr


def _oracle_Z(V, vals, rows, offs, X):
    from oracle.oracle import OracleCsc
    return OracleCsc(V, len(offs) - 1, vals, rows, offs).gram_apply(X)


# the geometries of the GPU sweep that a CPU handles in a moment
CPU_GEOMETRIES = {
    "ragged": lambda: (4500, *pattern_ragged(4500, 300, 11)),
    "V4079": lambda: (4079, *pattern_random(4079, 3000, 1, 12, 1, must=(4077, 4078))),
    "V8157": lambda: (8157, *pattern_random(8157, 3000, 1, 12, 2, must=(4077, 4078, 8156))),
    "D65": lambda: (3000, *pattern_random(3000, 65, 1, 200, 3)),
    "D4079": lambda: (3000, *pattern_random(3000, 4079, 1, 20, 4)),
    "D61171": lambda: (3000, *pattern_random(3000, 61171, 1, 6, 5)),
    "V81921": lambda: (81921, *pattern_random(81921, 3000, 20, 60, 6, must=(81919, 81920))),
    "place": lambda: (GL_RB, *pattern_place(7)),
}


@pytest.fixture(scope="module", params=sorted(CPU_GEOMETRIES))
def geom(request):
    return request.param, CPU_GEOMETRIES[request.param]()


def test_the_fp32_oracle_is_exact_on_dyadic_inputs_and_within_the_bound_on_others(geom):
    name, (V, rows, offs) = geom
    vals, _ = dyadic_row_values(V, rows, 1)
    B = csc64(V, vals, rows, offs)
    X = dyadic_X(V, 12, 2, B=B, zero_cols=(3,))
    Z64, M, B = gram64(V, vals, rows, offs, X)
    Z = _oracle_Z(V, vals, rows, offs, X)
    certify_exact(Z, Z64, M)
    certify_structure(Z, B, X)
    vals2, _ = sqrt_row_values(V, rows, 3)
    X2 = normal_X(V, 12, 4, zero_cols=(5,))
    Z64, M, B = gram64(V, vals2, rows, offs, X2)
    Z = _oracle_Z(V, vals2, rows, offs, X2)
    r = certify_gram(Z, Z64, M, B)
    certify_structure(Z, B, X2)
    assert 0 < r["max_ratio"] <= r["coeff_max"]


def test_per_entry_values_are_exact_too():
    V, rows, offs = 3000, *pattern_random(3000, 4000, 1, 30, 8)
    vals = dyadic_entry_values(rows, 9)
    B = csc64(V, vals, rows, offs)
    X = dyadic_X(V, 7, 10, B=B)
    Z64, M, _ = gram64(V, vals, rows, offs, X)
    certify_exact(_oracle_Z(V, vals, rows, offs, X), Z64, M)


def test_the_exact_check_refuses_inputs_that_are_not_exact_in_fp32():
    V, rows, offs = 3000, *pattern_random(3000, 500, 1, 30, 8)
    vals, _ = sqrt_row_values(V, rows, 1)
    X = normal_X(V, 3, 2)
    Z64, M, _ = gram64(V, vals, rows, offs, X)
    with pytest.raises(AssertionError, match="precondition"):
        certify_exact(_oracle_Z(V, vals, rows, offs, X), Z64, M)
    vals, _ = dyadic_row_values(V, rows, 1)
    Z64, M, _ = gram64(V, vals, rows, offs, np.full((V, 1), 2.0 ** 21, np.float32))
    with pytest.raises(AssertionError, match="precondition"):
        certify_exact(Z64.astype(np.float32), Z64, M)


# ---- planted faults: each models a way the banded form could go wrong (gram_lds.hip) ------------------------------------------------
@pytest.fixture(scope="module")
def case():
    """Two word bands (V = 8157), one document band and a half, b = 20 (two panels of 10), dyadic and non-dyadic values."""
    V = 8157
    rows, offs = pattern_random(V, 6000, 2, 40, 21, must=(4077, 4078, 8156))
    vals, s = dyadic_row_values(V, rows, 22)
    B = csc64(V, vals, rows, offs)
    X = dyadic_X(V, 20, 23, B=B)
    Z64, M, B = gram64(V, vals, rows, offs, X)
    Z = _oracle_Z(V, vals, rows, offs, X)
    certify_exact(Z, Z64, M)
    vals2, s2 = sqrt_row_values(V, rows, 24)
    X2 = normal_X(V, 20, 25)
    Z64b, Mb, B2 = gram64(V, vals2, rows, offs, X2)
    Zb = _oracle_Z(V, vals2, rows, offs, X2)
    certify_gram(Zb, Z64b, Mb, B2)
    return dict(V=V, rows=rows, offs=offs, dy=(B, s, X, Z, Z64, M), nd=(B2, s2, X2, Zb, Z64b, Mb))


def _heavy_entry(B, X, Z64, M, avoid_s1=False, s=None):
    """(w, d): an entry of B whose term B[w, d] Y_d is large against M[w] (a fault there is far above any rounding)."""
    Bc = B.tocoo()
    Y = np.asarray(B.T @ X.astype(np.float64))
    term = np.abs(Bc.data * Y[Bc.col, 0]) / np.maximum(M[Bc.row, 0], 1e-300)
    if avoid_s1:
        term = np.where(s[Bc.row] != 1.0, term, -1.0)
    i = int(np.argmax(term))
    return int(Bc.row[i]), int(Bc.col[i]), Y


def _term(B, w, d, Y):
    return B[w, d] * Y[d]


def _faults(c, which):
    """-> list of (name, fn(Z) -> faulty Z) on the case's data set `which` ('dy' or 'nd')."""
    B, s, X, Z, Z64, M = c[which]
    V = c["V"]
    w, d, Y = _heavy_entry(B, X, Z64, M)
    ws, _, _ = _heavy_entry(B, X, Z64, M, avoid_s1=True, s=s)
    Bcsr = B.tocsr()
    f = {}

    def put(name, fn):
        f[name] = fn

    # 1 / 2: an id dropped from / duplicated in word w's pass-2 stream
    put("dropped", lambda Zf: _add_row(Zf, w, -_term(B, w, d, Y)))
    put("duplicated", lambda Zf: _add_row(Zf, w, _term(B, w, d, Y)))
    # 3: the id moved to its neighbour inside the band (a document of the same band that word w does not hold)
    row_docs = set(Bcsr.indices[Bcsr.indptr[w]:Bcsr.indptr[w + 1]].tolist())
    dn = next(x for x in list(range(d + 1, B.shape[1])) + list(range(d - 1, -1, -1))
              if x not in row_docs and x // GL_RB == d // GL_RB and np.any(Y[x] != Y[d]))
    put("moved_to_neighbour", lambda Zf: _add_row(Zf, w, B[w, d] * (Y[dn] - Y[d])))
    # 4: a pass-1 id moved by one band (word w' -> w' + 4078): the document's Y reads another band's row of s X
    bc = B.tocsc()
    d4 = next(x for x in range(B.shape[1]) if bc.indptr[x + 1] > bc.indptr[x] and bc.indices[bc.indptr[x]] + GL_RB < V
              and np.any(X[bc.indices[bc.indptr[x]] + GL_RB] * s[bc.indices[bc.indptr[x]] + GL_RB] != X[bc.indices[bc.indptr[x]]] * s[bc.indices[bc.indptr[x]]]))
    w4 = int(bc.indices[bc.indptr[d4]])
    dY4 = s[w4 + GL_RB] * X[w4 + GL_RB].astype(np.float64) - s[w4] * X[w4].astype(np.float64)
    put("moved_by_a_band", lambda Zf: _add_col_outer(Zf, B, d4, dY4))
    # 5: s_w missing on one row (gl_reduce_cm_k)
    put("scale_missing", lambda Zf: _set_row(Zf, ws, Zf[ws].astype(np.float64) / s[ws]))
    # 6: a padding slot reads a non-zero row (another bank class) of s X into one document of pass 1
    d6 = d4
    r6 = next(r for r in range(V) if r % 16 != w4 % 16 and np.any(X[r] != 0))
    put("padding_reads_a_row", lambda Zf: _add_col_outer(Zf, B, d6, s[r6] * X[r6].astype(np.float64)))
    # 7: the half plane's columns 8 and 9 of the first panel swapped
    put("half_plane_swapped", lambda Zf: _swap_cols(Zf, 8, 9))
    # 8: the second panel computed from a stale X (the first panel's columns)
    put("second_panel_stale", lambda Zf: _set_cols(Zf, slice(10, 20), Zf[:, 0:10]))
    return [(k, f[k]) for k in which_order() if k in f], (w, d, ws)


def which_order():
    return ["dropped", "duplicated", "moved_to_neighbour", "moved_by_a_band", "scale_missing", "padding_reads_a_row",
            "half_plane_swapped", "second_panel_stale"]


def _add_row(Z, w, delta):
    Z = Z.copy()
    Z[w] = (Z[w].astype(np.float64) + delta).astype(np.float32)
    return Z


def _set_row(Z, w, v):
    Z = Z.copy()
    Z[w] = np.asarray(v).astype(np.float32)
    return Z


def _add_col_outer(Z, B, d, dY):
    """every word of document d gets B[w, d] dY added (a fault in document d's Y)."""
    Z = Z.copy()
    col = B.tocsc()[:, d]
    for w, v in zip(col.indices, col.data):
        Z[w] = (Z[w].astype(np.float64) + v * dY).astype(np.float32)
    return Z


def _swap_cols(Z, a, b):
    Z = Z.copy()
    Z[:, [a, b]] = Z[:, [b, a]]
    return Z


def _set_cols(Z, sl, v):
    Z = Z.copy()
    Z[:, sl] = v
    return Z


@pytest.mark.parametrize("fault", which_order())
def test_every_planted_fault_fails_the_exact_check(case, fault):
    B, s, X, Z, Z64, M = case["dy"]
    faults, _ = _faults(case, "dy")
    Zf = dict(faults)[fault](Z)
    assert not np.array_equal(Zf, Z), "the fault changed nothing"
    with pytest.raises(AssertionError, match="not bit-equal"):
        certify_exact(Zf, Z64, M)


@pytest.mark.parametrize("fault", ["dropped", "scale_missing"])
def test_dropped_ids_and_missing_scales_fail_the_bound_on_non_dyadic_values(case, fault):
    B, s, X, Z, Z64, M = case["nd"]
    faults, _ = _faults(case, "nd")
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        certify_gram(dict(faults)[fault](Z), Z64, M, B)


def test_relerr_misses_a_dropped_rare_word_that_the_bound_catches():
    """One rare word (a single entry, s_w = 1/256) among 2000 common ones: dropping its one id from the pass-2 stream zeroes its row of
    Z, a change of 1e-7 of the norm, far inside the old 1e-5 bar; the entry-wise bound catches it."""
    V, D = 2001, 5000
    rows, offs = pattern_random(V - 1, D, 5, 40, 31)
    rows, offs = [np.asarray(a) for a in (rows, offs)]
    cols = [rows[offs[i]:offs[i + 1]].tolist() for i in range(D)]
    cols[123].append(V - 1)  # the rare word: in document 123 only
    from gram_certificate import pattern_from_lists
    rows, offs = pattern_from_lists(V, cols)
    vals, s = sqrt_row_values(V, rows, 32)
    s[V - 1] = 1.0 / 256
    vals = s[rows.astype(np.int64)]
    X = normal_X(V, 10, 33)
    Z64, M, B = gram64(V, vals, rows, offs, X)
    Z = _oracle_Z(V, vals, rows, offs, X)
    certify_gram(Z, Z64, M, B)
    Zf = Z.copy()
    Zf[V - 1] = 0  # its only id dropped
    assert relerr(Zf, Z64) <= 1e-5
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        certify_gram(Zf, Z64, M, B)


def test_structure_check_catches_a_non_zero_empty_row_and_zero_column():
    V, rows, offs = 500, *pattern_ragged(500, 60, 1)
    vals, _ = dyadic_row_values(V, rows, 2)
    B = csc64(V, vals, rows, offs)
    X = dyadic_X(V, 4, 3, B=B, zero_cols=(2,))
    Z = _oracle_Z(V, vals, rows, offs, X)
    certify_structure(Z, B, X)
    empty = int(np.flatnonzero(np.diff(B.tocsr().indptr) == 0)[0])
    Zf = Z.copy()
    Zf[empty, 0] = 2.0 ** -30
    with pytest.raises(AssertionError, match="empty row"):
        certify_structure(Zf, B, X)
    Zf = Z.copy()
    Zf[7, 2] = 1.0
    with pytest.raises(AssertionError, match="zero column"):
        certify_structure(Zf, B, X)


# ---- coverage guard --------------------------------------------------------------------------------------------------------------
def _table_names():
    import isle_amd
    lib = isle_amd.load_library()
    n = lib.isle_hip_switch_info(-1, None, None, None)
    out = []
    for i in range(n):
        a = C.c_char_p()
        lib.isle_hip_switch_info(i, C.byref(a), None, None)
        out.append(a.value.decode())
    return out


def test_every_switch_of_the_gram_apply_is_swept_or_excluded_with_a_reason():
    names = _table_names()
    missing, stale = uncovered_gram_switches(names)
    assert not missing, "switches the Gram apply reads that the GPU certificate neither sweeps nor excludes: %s" % missing
    assert not stale, "swept / excluded switches the table does not know: %s" % stale
    assert {"ISLE_GRAM_LDS", "ISLE_GL_G1", "ISLE_GL_G2", "ISLE_GL_PLACE", "ISLE_GL_FILL_BUCKETS", "ISLE_GL_ROUNDS", "ISLE_GL_COLUMNS",
            "ISLE_CHUNK_COLS", "ISLE_GL_TEST_CUS"} <= set(GRAM_SWEEP)
    assert all(len(r) > 20 for r in GRAM_EXCLUDED.values()) and not set(GRAM_SWEEP) & set(GRAM_EXCLUDED)
    assert all(v for v in GRAM_SWEEP.values())


@pytest.mark.parametrize("name", sorted(GRAM_SWEEP))
def test_the_guard_fails_when_a_swept_switch_is_dropped(name):
    names = _table_names()
    sweep = {k: v for k, v in GRAM_SWEEP.items() if k != name}
    missing, _ = uncovered_gram_switches(names, sweep=sweep)
    assert missing == [name]
