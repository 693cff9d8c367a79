"""The Gram apply Z = B (B^T X) certified entry by entry against fp64 (tests/gram_certificate.py) in every form and switch value.

Dyadic inputs (B in {1/2, 1, 2}, small integer X) must give the fp64 product bit for bit in any summation order (certify_exact); where
marked, the same pattern with non-dyadic values must stay within the entry-wise fp32 bound (certify_gram).  Every switch is set before
the upload: the operator is built, and the form chosen, at the first apply after it (spmm.hip k_band_build).  ISLE_CHUNK_COLS is read
when a context is created (api.cpp isle_hip_create), so its cases run in a fresh HotPath.  Every geometry sits on a boundary the code
branches on; the comments name the line.

GRAM_CERT_REPORT=<path>: the largest |Z - Z64| / (u M) per form and switch of the non-dyadic cases is written there as JSON.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from gram_certificate import (GL_RB, GL_VP, GRAM_SWEEP, certify_exact, certify_gram, certify_structure, csc64, dyadic_X,
                              dyadic_entry_values, dyadic_row_values, gram64, normal_X, pattern_place, pattern_random, pattern_ragged,
                              sqrt_entry_values, sqrt_row_values)

pytestmark = pytest.mark.gpu

_PAT = {}   # geometry name -> (V, rows, offs)
_REF = {}   # (geometry, values, b) -> (vals, X, Z64, M, B): fp64 products cached per geometry
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GRAM_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def pattern(name):
    if name not in _PAT:
        _PAT[name] = _BUILDERS[name]()
    return _PAT[name]


def _mid():
    # >= 30 000 documents: several rounds of pass-1 workgroups under ISLE_GL_TEST_CUS (gl_plan.h gl_plan_pass1)
    return 6000, *pattern_random(6000, 30000, 5, 60, 101, must=(0, 4077, 4078, 5999))


_BUILDERS = {
    "mid": _mid,
    "ragged": lambda: (4500, *pattern_ragged(4500, 3000, 11)),
    "other": lambda: (3000, *pattern_random(3000, 2000, 1, 30, 102)),
    "place": lambda: (GL_RB, *pattern_place(103)),
    # G2 = 6 beyond 1024 document bands (s2.NB > 1024, gl_plan.h gl_plan_pass2_geometry): 1025 bands and more
    "G2six": lambda: (5000, *pattern_random(5000, 4_180_000, 1, 3, 104, must=(4999,))),
}
for _V in (4077, 4078, 4079, 8156, 8157):  # word bands of GL_RB = 4078 rows (pass 1's sources, gl_plan.h gl_plan_pass1)
    _BUILDERS["V%d" % _V] = (lambda V: lambda: (V, *pattern_random(V, 3000, 1, 12, V, must=tuple(sorted({4076, min(4077, V - 1), min(4078, V - 1), V - 1})))))(_V)
for _D in (1, 63, 64, 65, 4078, 4079):  # slices of 64 outputs and document bands of GL_RB (pass 2's sources, gl_plan.h gl_plan_pass2_geometry)
    _BUILDERS["D%d" % _D] = (lambda D: lambda: (3000, *pattern_random(3000, D, 1, 200, D)))(_D)
for _D in (61170, 61171):  # 15 and 16 document bands: band columns need s2.NB >= 16 (gl_plan.h gl_use_columns)
    _BUILDERS["D%d" % _D] = (lambda D: lambda: (3000, *pattern_random(3000, D, 1, 6, D)))(_D)
for _V in (GL_VP - 1, GL_VP, GL_VP + 1, 2 * GL_VP + 1):  # vocabulary parts of the LDS histograms (gl_hist_count_k grid, gram_lds.hip gl_cell_histogram)
    _BUILDERS["V%d" % _V] = (lambda V: lambda: (V, *pattern_random(V, 3000, 20, 60, V, must=(GL_VP - 2, GL_VP - 1, min(GL_VP, V - 1), V - 1))))(_V)
for _V in (1 << 20, (1 << 20) + 1):  # the pass-2 stream is filled by buckets only for V <= 2^20 (gram_lds.hip GlStream::fill_pass2)
    _BUILDERS["V%d" % _V] = (lambda V: lambda: (V, *pattern_random(V, 20000, 1, 5, V, must=((1 << 20) - 2, (1 << 20) - 1, V - 1))))(_V)


def reference(name, kind, b, seed=0, onehot=()):
    """kind: 'dy_row' / 'dy_entry' (dyadic) or 'nd_row' / 'nd_entry' (non-dyadic).  onehot: words w whose e_w are extra columns of X."""
    key = (name, kind, b, seed, tuple(onehot))
    if key not in _REF:
        V, rows, offs = pattern(name)
        if kind == "dy_row":
            vals = dyadic_row_values(V, rows, seed)[0]
        elif kind == "dy_entry":
            vals = dyadic_entry_values(rows, seed)
        elif kind == "nd_row":
            vals = sqrt_row_values(V, rows, seed)[0]
        else:
            vals = sqrt_entry_values(rows, seed)
        nz = max(0, b - len(onehot))
        if kind.startswith("dy"):
            X = dyadic_X(V, nz, seed + 1, B=csc64(V, vals, rows, offs), zero_cols=(1,) if nz > 2 else ())
        else:
            X = normal_X(V, nz, seed + 1, zero_cols=(1,) if nz > 2 else ())
        if onehot:
            E = np.zeros((V, len(onehot)), np.float32)
            E[list(onehot), np.arange(len(onehot))] = 1
            X = np.concatenate([X, E], axis=1)
        Z64, M, B = gram64(V, vals, rows, offs, X)
        _REF[key] = (vals, X, Z64, M, B)
    return _REF[key]


def certify_case(hp, name, form, b=10, dyadic="dy_row", nondyadic="nd_row", label=None, onehot=()):
    """Upload, apply, check the form; certify_exact on the dyadic input, then certify_gram on the non-dyadic one (if any)."""
    V, rows, offs = pattern(name)
    vals, X, Z64, M, B = reference(name, dyadic, b, onehot=onehot)
    hp.upload_csc(V, vals, rows, offs)
    Z = hp.gram_apply(X)
    assert hp.operator_form() == form
    certify_exact(Z, Z64, M)
    certify_structure(Z, B, X)
    if nondyadic:
        vals, X, Z64, M, B = reference(name, nondyadic, b, seed=1, onehot=onehot)
        hp.upload_csc(V, vals, rows, offs)
        Z = hp.gram_apply(X)
        assert hp.operator_form() == form
        r = certify_gram(Z, Z64, M, B)
        certify_structure(Z, B, X)
        key = label or ("form %d" % form)
        prev = REPORT.get(key, {"max_ratio": 0.0, "coeff_max": 0.0})
        REPORT[key] = {"max_ratio": max(prev["max_ratio"], r["max_ratio"]), "coeff_max": max(prev["coeff_max"], r["coeff_max"])}


# ---- column counts: every (LPE, half) instance and the panel split of gram_apply_dev (api.cpp:676) -----------------------------------
@pytest.mark.parametrize("form", [1, 0])
def test_every_column_count_from_1_to_32(hp, monkeypatch, form):
    if form == 0:
        monkeypatch.setenv("ISLE_GRAM_LDS", "0")
    V, rows, offs = pattern("ragged")
    for kind in ("dy_row", "nd_row"):
        vals, X, Z64, M, B = reference("ragged", kind, 32, seed=0 if kind == "dy_row" else 1)
        hp.upload_csc(V, vals, rows, offs)
        for b in range(1, 33):
            Xb = np.asfortranarray(X[:, :b])
            Z = hp.gram_apply(Xb)
            assert hp.operator_form() == form
            if kind == "dy_row":
                certify_exact(Z, Z64[:, :b], M[:, :b])
            else:
                r = certify_gram(Z, Z64[:, :b], M[:, :b], B)
                key = "form %d, b = 1..32" % form
                REPORT[key] = {"max_ratio": max(REPORT.get(key, {}).get("max_ratio", 0.0), r["max_ratio"]), "coeff_max": r["coeff_max"]}
            certify_structure(Z, B, Xb)


# ---- boundaries of the banded build -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4077, 4078, 4079, 8156, 8157])
def test_word_bands(hp, V):
    # e_w for w at 4077 (last row of band 0), 4078 (first of band 1) and V - 1 (last word)
    certify_case(hp, "V%d" % V, 1, b=13, onehot=tuple(sorted({min(4077, V - 1), min(4078, V - 1), V - 1})), label="form 1, word bands")


@pytest.mark.parametrize("D", [1, 63, 64, 65, 4078, 4079])
def test_document_slices_and_bands(hp, D):
    certify_case(hp, "D%d" % D, 1, label="form 1, document bands")


@pytest.mark.parametrize("D,columns", [(61170, None), (61171, None), (61171, "0")])
def test_band_columns(hp, monkeypatch, D, columns):
    # 15 bands: per-block chunking; 16: band columns shared through L2 (gl_plan.h gl_use_columns); ISLE_GL_COLUMNS=0 at 16
    if columns is not None:
        monkeypatch.setenv("ISLE_GL_COLUMNS", columns)
    certify_case(hp, "D%d" % D, 1, label="form 1, ISLE_GL_COLUMNS=%s" % (columns or "default"))


def test_more_than_1024_document_bands_take_six_items_per_lane(hp):
    # 4 180 000 documents = 1026 bands: s2.G = 6 by default (gl_plan.h gl_plan_pass2_geometry); once with non-dyadic values
    certify_case(hp, "G2six", 1, label="form 1, G2 = 6 (1026 document bands)")


@pytest.mark.parametrize("V", [GL_VP - 1, GL_VP, GL_VP + 1, 2 * GL_VP + 1])
def test_vocabulary_parts_of_the_histograms(hp, V):
    certify_case(hp, "V%d" % V, 1, b=4, label="form 1, vocabulary parts")


@pytest.mark.parametrize("V,buckets", [(1 << 20, None), ((1 << 20) + 1, None), (1 << 20, "0")])
def test_fill_by_buckets_up_to_2_pow_20_words(hp, monkeypatch, V, buckets):
    # gram_lds.hip GlStream::fill_pass2: buckets of word positions for V <= 2^20, the direct scatter above and under ISLE_GL_FILL_BUCKETS=0
    if buckets is not None:
        monkeypatch.setenv("ISLE_GL_FILL_BUCKETS", buckets)
    certify_case(hp, "V%d" % V, 1, b=2, label="form 1, ISLE_GL_FILL_BUCKETS=%s" % (buckets or "default"))


@pytest.mark.parametrize("place", [None, "0"])
def test_placement_and_register_sorts(hp, monkeypatch, place):
    # word rows of 32 ... 4078 documents in one document band, documents of 32 ... 65 words in one word band: slices on both sides of
    # GL_PLACE_MAXN = 8 super-rounds (gl_place_k) and of the register sorts (gl_sort2_k up to 16 ids a lane, gl_sort2_big_k beyond)
    if place is not None:
        monkeypatch.setenv("ISLE_GL_PLACE", place)
    certify_case(hp, "place", 1, label="form 1, ISLE_GL_PLACE=%s" % (place or "default"))


@pytest.mark.parametrize("cus", ["3", "7"])
@pytest.mark.parametrize("rounds", [None, "0"])
def test_rounds_of_workgroups(hp, monkeypatch, cus, rounds):
    # pass 1 laid out for a device of 3 or 7 CUs: whole rounds of adjacent waves, or strided under ISLE_GL_ROUNDS=0 (gl_plan.h gl_plan_pass1)
    monkeypatch.setenv("ISLE_GL_TEST_CUS", cus)
    if rounds is not None:
        monkeypatch.setenv("ISLE_GL_ROUNDS", rounds)
    certify_case(hp, "mid", 1, label="form 1, ISLE_GL_TEST_CUS=%s ISLE_GL_ROUNDS=%s" % (cus, rounds or "default"))


# ---- every switch value of the sweep on one matrix ----------------------------------------------------------------------------------
SWEEP_CASES = [(k, v) for k in sorted(GRAM_SWEEP) for v in GRAM_SWEEP[k]]


def _form_under(env):
    return 0 if env.get("ISLE_GRAM_LDS") == "0" else 1


@pytest.mark.parametrize("switch,value", [c for c in SWEEP_CASES if c[0] != "ISLE_CHUNK_COLS"])
def test_every_switch_value(hp, monkeypatch, switch, value):
    monkeypatch.setenv(switch, value)
    certify_case(hp, "mid", _form_under({switch: value}), label="form %d, %s=%s" % (_form_under({switch: value}), switch, value))


def test_per_entry_values_take_the_gather_form(hp):
    certify_case(hp, "mid", 0, dyadic="dy_entry", nondyadic="nd_entry", label="form 0, per-entry values")
    certify_case(hp, "ragged", 0, dyadic="dy_entry", nondyadic="nd_entry", label="form 0, per-entry values")


@pytest.mark.parametrize("chunk", GRAM_SWEEP["ISLE_CHUNK_COLS"])
def test_chunk_sizes_of_the_gather_form_in_fresh_contexts(monkeypatch, chunk):
    # read once, at isle_hip_create (api.cpp:403): set before the context exists
    from isle_amd import HotPath
    monkeypatch.setenv("ISLE_CHUNK_COLS", chunk)
    h = HotPath(0)
    try:
        certify_case(h, "mid", 0, dyadic="dy_entry", nondyadic="nd_entry", label="form 0, ISLE_CHUNK_COLS=%s" % chunk)
        monkeypatch.setenv("ISLE_GRAM_LDS", "0")
        certify_case(h, "ragged", 0, label="form 0, ISLE_CHUNK_COLS=%s" % chunk)
    finally:
        h.close()


# ---- reproducibility: Z depends on B alone (the id sort, gram_lds.hip gl_sort2_k) in every form -------------------------------------------
@pytest.mark.parametrize("switch,value", [(None, None)] + SWEEP_CASES)
def test_reupload_gives_the_same_bits(hp, monkeypatch, switch, value):
    from isle_amd import HotPath
    h = hp
    if switch is not None:
        monkeypatch.setenv(switch, value)
    if switch == "ISLE_CHUNK_COLS":
        monkeypatch.setenv("ISLE_GRAM_LDS", "0")
        h = HotPath(0)
    try:
        V, rows, offs = pattern("mid")
        vals, X, _, _, _ = reference("mid", "nd_row", 10, seed=1)
        Vo, ro, oo = pattern("other")
        vo = reference("other", "nd_entry", 10, seed=2)[0]
        h.upload_csc(V, vals, rows, offs)
        Z1 = h.gram_apply(X)
        h.upload_csc(Vo, vo, ro, oo)
        h.gram_apply(np.ones((Vo, 3), np.float32))
        h.upload_csc(V, vals, rows, offs)
        Z2 = h.gram_apply(X)
        assert h.operator_form() == (0 if switch in ("ISLE_GRAM_LDS", "ISLE_CHUNK_COLS") else 1)
        assert np.array_equal(Z1.view(np.uint32), Z2.view(np.uint32))
    finally:
        if h is not hp:
            h.close()


# ---- Frobenius norm and argument edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid", "ragged"])
def test_frobenius_is_the_fp64_sum_rounded_once(hp, name):
    # isle_hip_frobenius (api.cpp:649): fp64 sums of squares, one rounding to fp32
    V, rows, offs = pattern(name)
    for kind in ("dy_row", "dy_entry"):
        vals = reference(name, kind, 10)[0]
        hp.upload_csc(V, vals, rows, offs)
        f64 = float(np.sum(vals.astype(np.float64) ** 2))
        assert hp.frobenius() == np.float32(f64)  # the fp64 sum of dyadic squares is exact in any order
    vals = reference(name, "nd_row", 10, seed=1)[0]
    hp.upload_csc(V, vals, rows, offs)
    f64 = float(np.sum(vals.astype(np.float64) ** 2))
    f = np.float32(hp.frobenius())
    assert abs(float(f) - f64) <= float(np.spacing(np.float32(f64)))


def test_column_counts_outside_1_to_32_are_refused(hp):
    V, rows, offs = pattern("other")
    hp.upload_csc(V, reference("other", "dy_row", 10)[0], rows, offs)
    X = np.zeros((V, 33), np.float32, order="F")
    Z = np.zeros_like(X)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert hp._lib.isle_hip_gram_apply(hp._h, p(X), 0, p(Z)) == -1  # ISLE_E_ARG
    assert hp._lib.isle_hip_gram_apply(hp._h, p(X), 33, p(Z)) == -1
    assert not Z.any()


@pytest.mark.parametrize("V,cols", [(1, [[0]]), (2, [[1], [], [0, 1]]), (3, [[], [2], []])])
def test_the_smallest_matrices_the_upload_accepts(hp, monkeypatch, V, cols):
    # the upload takes V >= 1 and any monotone offsets (api.cpp upload_common); the banded form needs nnz, D, V > 0 (k_gl_detect)
    from gram_certificate import pattern_from_lists
    rows, offs = pattern_from_lists(V, cols)
    for form in (1, 0):
        if form == 0:
            monkeypatch.setenv("ISLE_GRAM_LDS", "0")
        vals = dyadic_row_values(V, rows, 5)[0]
        X = dyadic_X(V, 3, 6, zero_cols=(1,))
        Z64, M, B = gram64(V, vals, rows, offs, X)
        hp.upload_csc(V, vals, rows, offs)
        Z = hp.gram_apply(X)
        assert hp.operator_form() == form
        certify_exact(Z, Z64, M)
        certify_structure(Z, B, X)
