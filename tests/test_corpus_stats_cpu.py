"""The counting rule of the distinct top-five sets (isle_hip_top_five_count_rule, a host function of the library) against the reference's
loop transliterated literally (SparseMatrix::count_distint_top_five_words, src/sparseMatrix.cpp:198-208), and the binding of the corpus
diagnostics' symbols.  No GPU: the library loads and its host functions run on any machine."""
import ctypes as C

import numpy as np
import pytest

import isle_amd
from isle_amd._lib import SYMBOLS


def literal(q, m):
    """The reference's loop over the sorted tuples q (any comparable values), word for word."""
    n = len(q)
    num = 0
    it = prev = 0
    while it != n:
        if q[it] == q[prev]:
            it += 1
            continue
        if it - prev >= m:
            prev = it
            num += 1
        it += 1
    if prev - it >= m:  # never fires: prev <= it
        num += 1
    return num


def tuples_of(runs):
    """Sorted stand-ins for the tuples: run r holds runs[r] copies of the value r."""
    return np.repeat(np.arange(len(runs)), np.asarray(runs, np.int64)).tolist()


def rule(runs, m):
    lib = isle_amd.load_library()
    runs = np.ascontiguousarray(runs, np.uint64)
    out = C.c_uint64(12345)
    rc = lib.isle_hip_top_five_count_rule(runs.ctypes.data_as(C.c_void_p) if runs.size else None, runs.size, m, C.byref(out))
    return rc, out.value


def test_symbols_are_bound():
    lib = isle_amd.load_library()
    for name in ("isle_hip_log_combinatorial", "isle_hip_distinct_top_five", "isle_hip_top_five_count_rule"):
        assert name in SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert lib.isle_hip_log_combinatorial(None, None, None) != 0          # no context: ISLE_E_ARG, no crash
    assert lib.isle_hip_distinct_top_five(None, 0, None, None, None, None, None, None) != 0


@pytest.mark.parametrize("runs,m,want", [
    ([], 2, 0),                        # n = 0
    ([1], 2, 0),
    ([1, 1, 1, 1, 1], 2, 2),           # all distinct: jumps of m
    ([1, 1, 1, 1, 1], 5, 0),           # m = n
    ([1, 1, 1, 1, 1], 500, 0),         # m > n
    ([7], 2, 0),                       # one run
    ([3, 3, 3], 2, 2),
    ([2, 9, 1, 1], 5, 2),              # a run longer than m: 0 -> 5 -> 11
    ([1] * 12, 3, 3),
])
def test_known_answers(runs, m, want):
    assert literal(tuples_of(runs), m) == want
    assert rule(runs, m) == (0, want)


def test_random_run_lengths_match_the_literal_loop():
    rng = np.random.default_rng(2024)
    ms = [2, 3, 5, 10, 20, 50, 100, 200, 500]
    checked = 0
    for trial in range(3000):
        kind = trial % 4
        nr = int(rng.integers(0, 60))
        if kind == 0:
            runs = np.ones(nr, np.int64)                                   # all length 1
        elif kind == 1:
            runs = rng.integers(1, 4, size=nr)                             # short runs
        elif kind == 2:
            runs = rng.geometric(0.05, size=nr)                            # runs often longer than m
        else:
            runs = np.where(rng.random(nr) < 0.1, rng.integers(100, 700, size=nr), rng.integers(1, 12, size=nr))
        q = tuples_of(runs)
        for m in (ms[trial % len(ms)], int(rng.integers(2, 40)), len(q) + 2):   # m larger than n included
            assert rule(runs, m) == (0, literal(q, m)), (runs.tolist(), m)
            checked += 1
    assert checked == 9000


def test_argument_errors():
    lib = isle_amd.load_library()
    runs = np.array([1, 2], np.uint64)
    out = C.c_uint64()
    p = runs.ctypes.data_as(C.c_void_p)
    assert lib.isle_hip_top_five_count_rule(p, 2, 1, C.byref(out)) != 0     # m < 2 (an assert in the reference)
    assert lib.isle_hip_top_five_count_rule(p, 2, 2, None) != 0             # null out
    assert lib.isle_hip_top_five_count_rule(None, 2, 2, C.byref(out)) != 0  # null runs with n_runs > 0
    zero = np.array([1, 0, 2], np.uint64)
    assert lib.isle_hip_top_five_count_rule(zero.ctypes.data_as(C.c_void_p), 3, 2, C.byref(out)) != 0   # empty run
