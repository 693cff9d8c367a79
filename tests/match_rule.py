"""The rule of isle_hip_compare_models / isle_hip_match_topics in numpy, and the case table of its tests (a plain module: importable
without the library and without a GPU).  isle_amd/csrc/match_host.h states the same rule in C++; tests/test_match_rule_cpu.py holds
the two to each other and this one to a brute-force statement on Python numbers.

Distances: dist[i][j] = sum_w |(double)a[w, i] - (double)b[w, j]|, NaN where column i of a or column j of b holds a non-finite entry.
The dyadic cases hold integer multiples of 2^-12 only: every partial sum is exact in double, so any order of summation gives the same
bits and the tests compare with ==.
Matching: greedy over the finite entries in the order (value, i, j), -0 equal to +0; `rounds` counts the rounds of mutually best pairs
that matched something, which is how the device gets to the same matching."""
from collections import namedtuple

import numpy as np

MC_TILE = 64       # isle_amd/csrc/match_host.h (test_match_rule_cpu.py reads the header's text)
MC_CHUNK = 64
MAX_TOPICS = 8192
MAX_VOCAB = 0xfffffff0
PARTIAL_BYTES = 1 << 30
SLICE_WAVES = 4
SLICES = (0, 1, 2, 3, 7)
MODEL_NAMES = {0: "catch", 1: "average", 2: "host", 3: "loaded"}


# ---- distances -----------------------------------------------------------------------------------------------------------------------
def dist_rule(a, b):
    """a (V, ka), b (V, kb) float32 -> (ka, kb) float64"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a64.shape[1], b64.shape[1]), np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(a64.shape[1]):
            out[i] = np.abs(a64[:, i:i + 1] - b64).sum(axis=0)
    out[~np.isfinite(a64).all(axis=0), :] = np.nan
    out[:, ~np.isfinite(b64).all(axis=0)] = np.nan
    return out


# ---- matching ------------------------------------------------------------------------------------------------------------------------
def mean_of(match_a, match_dist):
    s, n = 0.0, 0
    for i in range(len(match_a)):           # ascending i, in double
        if match_a[i] >= 0:
            s, n = s + float(match_dist[i]), n + 1
    return (s / n if n else float("nan")), n


def match_rule(dist):
    """(na, nb) float64 -> dict(match_a, match_b, match_dist, n_matched, mean_dist, rounds)"""
    d = np.asarray(dist, np.float64)
    na, nb = d.shape
    ii, jj = np.nonzero(np.isfinite(d))
    order = np.lexsort((jj, ii, d[ii, jj] + 0.0))      # + 0.0: -0 becomes +0, as < sees them
    ma, mb, md = np.full(na, -1, np.int32), np.full(nb, -1, np.int32), np.full(na, np.nan)
    for e in order:
        i, j = int(ii[e]), int(jj[e])
        if ma[i] < 0 and mb[j] < 0:
            ma[i], mb[j], md[i] = j, i, d[i, j]
    mean, n = mean_of(ma, md)
    return dict(match_a=ma, match_b=mb, match_dist=md, n_matched=n, mean_dist=mean, rounds=rounds_of(d)[1])


def rounds_of(dist):
    """The device's mechanism: rounds of mutually best pairs -> (match_a, the rounds that matched a pair)."""
    d = np.asarray(dist, np.float64) + 0.0
    na, nb = d.shape
    big = np.where(np.isfinite(d), d, np.inf)
    ma, mb, rounds = np.full(na, -1, np.int32), np.full(nb, -1, np.int32), 0
    while True:
        free = np.where((ma[:, None] < 0) & (mb[None, :] < 0) & np.isfinite(d), big, np.inf)
        row_best = np.where(np.isfinite(free).any(axis=1), free.argmin(axis=1), -1)     # argmin: the first of equal values
        col_best = np.where(np.isfinite(free).any(axis=0), free.argmin(axis=0), -1)
        got = [(i, int(row_best[i])) for i in range(na) if row_best[i] >= 0 and col_best[row_best[i]] == i]
        if not got:
            return ma, rounds
        for i, j in got:
            ma[i], mb[j] = j, i
        rounds += 1


# ---- the slice rule and the refusals' texts -----------------------------------------------------------------------------------------
def slices_rule(V, ka, kb, num_cus, asked):
    tiles = -(-ka // MC_TILE) * -(-kb // MC_TILE)
    chunks = max(1, -(-V // MC_CHUNK))
    s = asked if asked >= 1 else -(-SLICE_WAVES * max(1, num_cus) // tiles)
    return max(1, min(s, chunks, max(1, PARTIAL_BYTES // (ka * kb * 8))))


def slice_bounds(V, slices):
    per = -(-max(1, -(-V // MC_CHUNK)) // slices) * MC_CHUNK
    return [min(V, s * per) for s in range(slices + 1)]


def check_side(side, which, host_given, cols, resident, res_vocab, res_cols, vocab):
    if which not in MODEL_NAMES:
        return "compare_models: side %s: unknown model %d" % (side, which)
    if not 1 <= cols <= MAX_TOPICS:
        return "compare_models: side %s: %d columns outside 1 .. %d" % (side, cols, MAX_TOPICS)
    name = MODEL_NAMES[which]
    if which == 2:
        return "" if host_given else "compare_models: side %s: null host model" % side
    if not resident:
        return "compare_models: side %s: no %s model is resident" % (side, name)
    if vocab != res_vocab:
        return "compare_models: side %s: vocab = %d, the %s model's is %d" % (side, vocab, name, res_vocab)
    if cols != res_cols:
        return "compare_models: side %s: %d columns, the %s model has %d" % (side, cols, name, res_cols)
    return ""


def check_compare(a, b, vocab):
    """a, b: (which, host_given, cols, resident, res_vocab, res_cols)"""
    if vocab == 0 or vocab > MAX_VOCAB:
        return "compare_models: vocab = %d outside 1 .. %d" % (vocab, MAX_VOCAB)
    return check_side("a", *a, vocab) or check_side("b", *b, vocab)


def check_match(dist_given, na, nb):
    if not (1 <= na <= MAX_TOPICS and 1 <= nb <= MAX_TOPICS):
        return "match_topics: %d x %d outside 1 .. %d on each side" % (na, nb, MAX_TOPICS)
    return "" if dist_given else "match_topics: null dist_host"


def check_slices(slices):
    return "model_dist_slices: slices = %d is negative" % slices if slices < 0 else ""


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
DistCase = namedtuple("DistCase", "name a b same")       # a (V, ka), b (V, kb) F-order float32; same: b is a
MatchCase = namedtuple("MatchCase", "name dist")


def dyadic(rng, V, k):
    """random integer multiples of 2^-12 in [0, 1], about half of them zero"""
    m = rng.integers(0, 4097, size=(V, k)).astype(np.float64) / 4096.0
    m[rng.random((V, k)) < 0.5] = 0.0
    return np.asfortranarray(m, np.float32)


def _dist_cases():
    rng = np.random.default_rng(20260)
    T, Ch = MC_TILE, MC_CHUNK
    Vs = [1, 2, 3, 4, 5, Ch - 1, Ch, Ch + 1, 2 * Ch + 3, 4 * Ch + 1]
    ks = [(1, 1), (2, 1), (1, 2), (2, 2), (T - 1, T), (T, T), (T + 1, T - 1), (T, T + 1), (1, 2 * T + 1), (2 * T + 1, 1), (2 * T + 1, T + 1), (T + 1, 2 * T + 1)]
    out = []
    for n, (ka, kb) in enumerate(ks):           # every pair of sides at three vocabularies, every vocabulary at three pairs and more
        for V in (Vs[n % len(Vs)], Vs[(n + 3) % len(Vs)], Vs[(n + 7) % len(Vs)]):
            out.append(DistCase("V%d_%dx%d" % (V, ka, kb), dyadic(rng, V, ka), dyadic(rng, V, kb), False))
    # non-finite entries: a NaN in one column of each side, an inf in another; the vocabulary is odd (misaligned columns) and spans chunks
    V, ka, kb = 2 * Ch + 3, T + 1, 5
    a, b = dyadic(rng, V, ka), dyadic(rng, V, kb)
    a[7, 2], a[V - 1, T] = np.nan, np.inf
    b[0, 4], b[Ch, 1] = np.nan, -np.inf
    out.append(DistCase("nonfinite", a, b, False))
    m = dyadic(rng, Ch + 1, T + 1)
    out.append(DistCase("same", m, m, True))
    # ties: a's columns are word permutations of one column and b's columns are constant, two of them the same constant: all rows of
    # dist are equal and so are two of its columns
    base = dyadic(rng, 4 * Ch + 1, 1)[:, 0]
    a = np.asfortranarray(np.stack([base[rng.permutation(base.size)] for _ in range(9)], axis=1))
    b = np.asfortranarray(np.stack([np.full(base.size, v, np.float32) for v in (0.0, 0.25, 0.25, 1.0)], axis=1))
    out.append(DistCase("ties", a, b, False))
    return out


def _generic_case():
    rng = np.random.default_rng(7)
    a, b = rng.random((1000, 5)), rng.random((1000, 7))
    return DistCase("generic", np.asfortranarray(a / a.sum(axis=0), np.float32), np.asfortranarray(b / b.sum(axis=0), np.float32), False)


def _match_cases():
    rng = np.random.default_rng(11)
    out = []
    for n, (na, nb) in enumerate([(5, 5), (17, 9), (9, 17), (64, 65), (70, 3)]):
        out.append(MatchCase("ints%d_%dx%d" % (n, na, nb), rng.integers(0, 4, size=(na, nb)).astype(np.float64)))
    z = np.where(rng.random((12, 13)) < 0.5, -0.0, 0.0)
    z[rng.random((12, 13)) < 0.2] = 1.0
    out.append(MatchCase("zeros", z))
    d = rng.integers(0, 5, size=(8, 11)).astype(np.float64)
    d[3, :] = np.nan
    out.append(MatchCase("nan_row", d))
    d = rng.integers(0, 5, size=(11, 8)).astype(np.float64)
    d[:, 0] = np.nan
    d[:, 5] = np.nan
    out.append(MatchCase("nan_col", d))
    out.append(MatchCase("all_nan", np.full((6, 4), np.nan)))
    d = rng.integers(0, 3, size=(10, 10)).astype(np.float64)
    d[rng.random((10, 10)) < 0.3] = np.inf
    d[rng.random((10, 10)) < 0.2] = -np.inf
    d[4, :] = np.inf
    out.append(MatchCase("infs", d))
    out.append(MatchCase("one", np.array([[2.5]])))
    out.append(MatchCase("one_nan", np.array([[np.nan]])))
    i = np.arange(130, dtype=np.float64)
    out.append(MatchCase("i_plus_j", i[:, None] + i[None, :]))
    # a permuted near-diagonal, 129 x 65: row perm[j] is column j's partner at a small distance, everything else is far
    perm = rng.permutation(129)[:65]
    d = 10.0 + rng.random((129, 65))
    d[perm, np.arange(65)] = rng.random(65) * 0.5
    out.append(MatchCase("near_diagonal", d))
    return out


DIST_CASES = _dist_cases()
GENERIC = _generic_case()
MATCH_CASES = _match_cases()
