"""The free k-means++ draw (no injected seeds) replayed in fp64, seed by seed (no GPU, no library import; numpy, and for the
generic corpus alone scipy and tools.synth, imported where it is built).

isle_hip_kmeanspp_projected (isle_amd/csrc/api_kmeans.cpp) draws its seeds from the prefix sums of the squared distances: a round folds the
seeds of the round before into min_dist, scans it in double, throws ndraw dice `total * fraction()` and looks each one up.  All of that is
comparison and index logic and can be held to `==` once the rounding in front of it is gone:

  exact inputs   B holds small non-negative integers (<= 15, at most 12 words of U's span per document) and U is the first k columns of the
                 V x V identity.  Then P[d, j] = B[j, d] in every projection form, every norm, dot product and squared distance is an
                 integer far below 2^24 — `(-2 s + cn) + nd` of the update kernels is exact in any summation order, on the matrix cores and
                 in bf16 terms —, the fp64 scan of integers is exact in any order, `total * fraction` is one IEEE double product on the host
                 and in search_frac_k, and `die - my_off` of kmpp_draw_by_ranks subtracts an integer from a double below 2^53.  replay()
                 gives THE answer: the ordered seeds, the rounds, float32(total - last distance) of the last round, min_dist with the last
                 batch not folded in, and C_lowd = P[seeds].
  generic inputs admissible() is teacher-forced on the device's own seed list: per die the set of documents whose interval of the prefix
                 sums can contain it when every min_dist moves by E = ISLE_SLACK_REL (|p_d|^2 + max_s |p_s|^2) (kmeans_certificate.
                 certify_kmeanspp), accumulated over the prefix.  With E at 1e-4 of the norms these sets span a few documents at D ~ 6000
                 (measured: up to 5 at k = 65, up to 7 at k = 300 on the small corpus), so this certificate catches a stale min_dist or a wrong
                 distribution under real rounding and does NOT catch an off-by-one; the exact cases do that.

What the replay settles about the library's rule, and the tests rely on:

- On exact inputs a round that adds no seed happens only when the total is zero.  Every seed chosen so far is folded in before the dice
  are thrown and its own distance is exactly 0, so a die below the total lands in a document of positive width, which is no seed yet: the
  first die of a round always adds one.  With a zero total every die is 0, the search runs off the end and the clamp picks D - 1 (on
  several ranks the rank that holds the last document answers: `exhausted-37` in tests/kmpp_shard_cases.py).  So on these inputs a round
  without a new seed (k_kmpp_update with nc = 0) is followed only by more such rounds and the refusal after 100 k of them:
  `exhausted-38` is the one run that reaches it.  Under real rounding `(-2 s + cn) + nd` of a seed against itself can leave a tiny
  positive width, so there a round that adds nothing and a successful run behind it are improbable, not impossible; no test here
  reaches that (by reading, k_kmpp_update returns at nc = 0 before it touches what the rounds keep for Lloyd).  Duplicates inside a round
  (two dice in one document) are common on clustered corpora and are what the `clustered` cases hold.
- The fractions of the last round that are left when the k-th seed arrives are consumed, but the generator dies with the call: not
  consuming them changes nothing a caller can see.  replay() reports the number consumed and the CPU test holds a rule that stops early to
  that count; no case can fail on it.

`ndraw > 40` on one rank, where the draw falls to kmpp_draw_by_ranks without the host-dice switch, is reached by `k-1540` alone (BIG_CASES).
Not reached by any case: a fraction that rounds to 1.0 (both words 2^31 - 1), so that the die equals a positive total.
"""
import math
import os
import re

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_TILE = 4096   # isle_amd/csrc/scan.h: SCAN_T * SCAN_ITEMS
SCAN_T = 256       # blocks per trip of scan_blk_k's carry loop
FIRST_MUL = 84619573


def header_slack():
    text = open(os.path.join(_ROOT, "isle_amd", "csrc", "hamerly.h")).read()
    m = re.search(r"#define\s+ISLE_SLACK_REL\s+([0-9.]+(?:[eE][-+]?[0-9]+)?)[fF]?", text)
    assert m, "ISLE_SLACK_REL not found in hamerly.h"
    return float(np.float32(float(m.group(1))))


# ---- the generator (api_internal.h HostRng: glibc's TYPE_3 additive feedback generator) ----------------------------------------------------
class HostRng:
    M32 = 0xFFFFFFFF

    def __init__(self, seed64, swap_words=False):
        seed = int(seed64) & self.M32
        if seed == 0:
            seed = 1
        w = [0] * 34
        w[0] = seed - (1 << 32) if seed >= (1 << 31) else seed  # (int32_t)seed
        for i in range(1, 31):
            v = int(math.fmod(16807 * w[i - 1], 2147483647))  # C's %, the sign of the dividend
            if v < 0:
                v += 2147483647
            w[i] = v
        for i in range(31, 34):
            w[i] = w[i - 31]
        self.r = [x & self.M32 for x in w]
        self.k = 0
        self.swap_words = swap_words
        self.fractions = 0
        for _ in range(34, 344):
            self.step()

    def step(self):
        v = (self.r[(self.k + 34 - 31) % 34] + self.r[(self.k + 34 - 3) % 34]) & self.M32
        self.r[self.k % 34] = v
        self.k = (self.k + 1) % 34
        return v

    def next31(self):
        return self.step() >> 1

    def fraction(self):
        R1 = 2147483648.0
        lo = float(self.next31())  # the low word is drawn first
        hi = float(self.next31())
        if self.swap_words:
            lo, hi = hi, lo
        self.fractions += 1
        return (lo + hi * R1) / (R1 * R1)


def host_rand(seed, n):
    """n outputs of rand() after srand(seed): what isle_hip_host_rand returns."""
    g = HostRng(seed)
    return np.array([g.next31() for _ in range(n)], np.uint32)


def first_seed(rng_seed, D):
    return (HostRng(rng_seed).next31() * FIRST_MUL) % D


def ndraw_at(s, k):
    """dice of a round that starts with s seeds (api_kmeans.cpp:224-225)."""
    n = 0
    while n < 1 + math.sqrt(float(s - 5 if s - 5 > 0 else 0)):
        n += 1
    return min(n, 2 + int(math.ceil(math.sqrt(float(k)))))


class Exhausted(Exception):
    """the library's ISLE_E_NUMERIC "k-means++ cannot find k distinct seeds" after 100 k rounds"""


# ---- the replay ---------------------------------------------------------------------------------------------------------------------------
WRONG_RULES = ("search-lo", "stale-fold", "total-minus-last", "swapped-words", "redraw", "stop-early", "carry-dropped", "not-squared")


def _fold(md, P, pn, ids, f32):
    if not len(ids):
        return md
    C = P[np.asarray(ids, np.int64)]
    if f32:  # the library's rule in float32: ((-2 s + |c|^2) + |p|^2) clamped at 0
        s = (P @ C.T).astype(np.float32)
        t = np.maximum((np.float32(-2.0) * s + pn[np.asarray(ids, np.int64)][None, :]) + pn[:, None], np.float32(0.0))
    else:
        t = np.maximum((pn[:, None] + pn[np.asarray(ids, np.int64)][None, :]) - 2.0 * (P @ C.T), 0.0)
    return np.minimum(md, t.min(axis=1))


def _prefix(md, wrong):
    cum = np.zeros(md.shape[0] + 1, np.float64)
    w = md.astype(np.float64)
    if wrong == "not-squared":
        w = np.sqrt(w)
    np.cumsum(w, out=cum[1:])
    if wrong == "carry-dropped" and md.shape[0] > SCAN_T * SCAN_TILE:  # the second trip of scan_blk_k starts from 0 again
        cum[SCAN_T * SCAN_TILE + 1:] -= cum[SCAN_T * SCAN_TILE]
        cum[SCAN_T * SCAN_TILE] = cum[SCAN_T * SCAN_TILE - 1]
    return cum


def replay(P, k, rng_seed, f32=False, wrong=None):
    """api_kmeans.cpp:183-265 in numpy.  P (D, k'): the projected documents (float64; f32: taken as float32 and the distances formed
    in float32 as the kernels form them).  -> dict(seeds, rounds, duplicates, zero_add_rounds, zero_total_rounds, dice (per round),
    fractions, min_dist (float32, the last batch not folded in), residual (float32), batches (the seeds each round added), md_by_round).
    Raises Exhausted after 100 k rounds.  wrong: one of WRONG_RULES, for the tests that show each of them is caught."""
    assert wrong is None or wrong in WRONG_RULES, wrong
    P = np.ascontiguousarray(P, np.float32 if f32 else np.float64)
    D = P.shape[0]
    assert 1 <= k <= D
    pn = np.einsum("ij,ij->i", P, P).astype(P.dtype)
    rng = HostRng(rng_seed, swap_words=wrong == "swapped-words")
    centers = [(rng.next31() * FIRST_MUL) % D]
    chosen = set(centers)
    batch, held = list(centers), []
    md = np.full(D, np.finfo(np.float32).max, P.dtype)
    rounds = dup = zero_add = zero_total = 0
    dice_log, batches = [], [list(centers)]
    total = last = 0.0
    while len(centers) < k:
        rounds += 1
        if wrong == "stale-fold" and rounds > 1:  # a batch reaches min_dist one round late
            md = _fold(md, P, pn, held, f32)
            held = batch
        else:
            md = _fold(md, P, pn, batch, f32)
        cum = _prefix(md, wrong)
        total, last = float(cum[D]), float(md[D - 1])
        zero_total += total == 0.0
        nd = ndraw_at(len(centers), k)
        dice_log.append(nd)
        batch = []
        i = redrawn = 0
        while i < nd:
            if wrong == "stop-early" and len(centers) >= k:
                break
            f = rng.fraction()
            i += 1
            if len(centers) >= k:
                continue
            t = total - last if wrong == "total-minus-last" else total
            x = min(max(t * f, 0.0), t)
            lo = int(np.searchsorted(cum, x, side="right"))  # the first index whose prefix sum exceeds the die
            pick = min(lo if wrong == "search-lo" else lo - 1, D - 1)
            if pick in chosen:
                dup += 1
                if wrong == "redraw" and total > 0.0 and redrawn < 64:  # (all the mass left may sit in seeds of this round)
                    i -= 1
                    redrawn += 1
                continue
            centers.append(pick)
            chosen.add(pick)
            batch.append(pick)
        zero_add += not batch
        batches.append(list(batch))
        if rounds > 100 * k:
            raise Exhausted("k-means++ cannot find %d distinct seeds" % k)
    return dict(seeds=np.array(centers, np.uint64), rounds=rounds, duplicates=dup, zero_add_rounds=zero_add, zero_total_rounds=zero_total,
                dice=dice_log, fractions=rng.fractions, min_dist=md.astype(np.float32), residual=float(np.float32(total - last)),
                batches=batches)


def replay_brute(P, k, rng_seed):
    """The same rule with nothing shared but the generator: Python floats, math.fsum for every prefix sum, a linear scan for the search.
    For the small cases."""
    P = [[float(x) for x in row] for row in np.asarray(P, np.float64)]
    D = len(P)
    rng = HostRng(rng_seed)
    centers = [(rng.next31() * FIRST_MUL) % D]
    md = [float(np.finfo(np.float32).max)] * D
    batch = list(centers)
    rounds, total, last = 0, 0.0, 0.0
    while len(centers) < k:
        rounds += 1
        for c in batch:
            for d in range(D):
                md[d] = min(md[d], max(math.fsum((a - b) * (a - b) for a, b in zip(P[d], P[c])), 0.0))
        total, last = math.fsum(md), md[D - 1]
        nd = ndraw_at(len(centers), k)
        batch = []
        for f in [rng.fraction() for _ in range(nd)]:
            if len(centers) >= k:
                break
            x = min(max(total * f, 0.0), total)
            pick = D - 1
            for d in range(D):  # the last document whose prefix sum does not exceed the die
                if math.fsum(md[:d + 1]) > x:
                    pick = d
                    break
            if pick not in centers:
                centers.append(pick)
                batch.append(pick)
        if rounds > 100 * k:
            raise Exhausted()
    return dict(seeds=np.array(centers, np.uint64), rounds=rounds, min_dist=np.array(md, np.float32), residual=float(np.float32(total - last)))


# ---- exact inputs -------------------------------------------------------------------------------------------------------------------------
MAX_VAL, MAX_WORDS = 15, 12


def _rows(rng, n, k, row_constant):
    """n integer rows of k coordinates: up to MAX_WORDS non-zeros in 1 .. MAX_VAL.  row_constant: the value depends on the coordinate only
    (every row of B holds one value: the LDS-banded form of the operator, and with it the thin-product rounds, can be had)."""
    P = np.zeros((n, k), np.float64)
    m = min(k, MAX_WORDS)
    words = rng.integers(0, k, (n, m))
    keep = rng.random((n, m)) < 0.7
    keep[:, 0] = True
    vals = 1 + words % MAX_VAL if row_constant else rng.integers(1, MAX_VAL + 1, (n, m))
    r = np.repeat(np.arange(n), m).reshape(n, m)
    P[r[keep], words[keep]] = vals[keep]
    return P


def _distinct_rows(rng, n, k, row_constant):
    P = _rows(rng, 4 * n + 8, k, row_constant)
    _, first = np.unique(P, axis=0, return_index=True)
    first = np.sort(first)
    assert first.size >= n, "cannot draw %d distinct rows at k = %d" % (n, k)
    return P[first[:n]]


def _case(name, D, k, rng_seed, kind="random", row_constant=True, **kw):
    return dict(name=name, D=D, k=k, rng_seed=rng_seed, kind=kind, row_constant=row_constant, **kw)


def final_round_dice_k(n):
    """the smallest k whose last round is certain to throw exactly n dice, and no round more: the last round starts with at least k - n
    and at most k - 1 seeds."""
    for k in range(7, 4000):
        if ndraw_at(k - 1, k) == n and ndraw_at(max(k - n, 1), k) == n:
            return k
    raise AssertionError(n)


CLUSTER_PROTOS, CLUSTER_OUTLIERS = 6, 30
CLUSTER_DISTINCT = CLUSTER_PROTOS + CLUSTER_OUTLIERS

# rng_seed: searched on the CPU (search_rng_seed) for the edge the case is named for; test_kmpp_certificate_cpu.py asserts each is reached
CASES = [
    _case("tile-4095", 4095, 9, 1, row_constant=False),
    _case("tile-4096", 4096, 9, 2, row_constant=False),
    _case("tile-4097", 4097, 9, 3, row_constant=False),
    _case("tiny-1", 1, 1, 1, kind="distinct", row_constant=False),
    _case("tiny-2", 2, 2, 1, kind="distinct", row_constant=False),
    _case("tiny-63", 63, 3, 1, kind="distinct", row_constant=False),
    _case("tiny-64", 64, 3, 2, kind="distinct", row_constant=False),
    _case("tiny-65", 65, 3, 3, kind="distinct", row_constant=False),
    _case("zeros-front-back", 3001, 9, 18, kind="zeros"),  # the first seed is document 44, a front copy
    _case("zeros-back-front", 3001, 9, 10, kind="zeros"),  # ... a back copy
    _case("clustered-20", 5000, 20, 7, kind="clustered"),
    _case("clustered-36", 5000, 36, 1, kind="clustered"),
    _case("exhausted-37", 5000, CLUSTER_DISTINCT + 1, 1, kind="clustered"),
    _case("exhausted-38", 5000, CLUSTER_DISTINCT + 2, 2, kind="clustered", raises=True),
    _case("dice-16", 6001, final_round_dice_k(16), 1),
    _case("dice-17", 6001, final_round_dice_k(17), 1),
    _case("k-65", 6001, 65, 1),
    _case("k-225", 6001, 225, 1),
    _case("k-300", 6001, 300, 1),
    _case("k-1000", 3001, 1000, 1),
    _case("clustered-260", 5000, 260, 1, kind="clustered", protos=40, outliers=400),
]
# the long ones, each a test of its own
BIG_CASES = [
    _case("blocks-257", SCAN_T * SCAN_TILE + 1, 8, 1, kind="copies", protos=20000),
    _case("k-1540", 1600, 1540, 1, kind="distinct"),
]
ALL_CASES = {c["name"]: c for c in CASES + BIG_CASES}

# the forms of the rounds: every switch route_kmpp_plan or route_kmpp_sparse (route_host.h) depends on
SWITCHES = {"KN_KMPP_HOST_DICE": "ISLE_KMPP_HOST_DICE", "KN_KMPP_TRACK": "ISLE_KMPP_TRACK", "KN_KMPP_SPARSE": "ISLE_KMPP_SPARSE"}
BASE_FORMS = [{}, {"ISLE_KMPP_HOST_DICE": "1"}, {"ISLE_KMPP_SPARSE": "0"}, {"ISLE_KMPP_SPARSE": "1"}, {"ISLE_KMPP_SPARSE": "1", "ISLE_KMPP_HOST_DICE": "1"}]
TRACK_FORMS = [{"ISLE_KMPP_TRACK": "0"}, {"ISLE_KMPP_TRACK": "1"}, {"ISLE_KMPP_SPARSE": "1", "ISLE_KMPP_TRACK": "0"},
               {"ISLE_KMPP_SPARSE": "1", "ISLE_KMPP_TRACK": "1"}]


def forms_of(case):
    return BASE_FORMS + (TRACK_FORMS if case["k"] > 224 else [])
_P_CACHE = {}


def exact_P(case):
    """The integer projection (D, k) float64 of a case (cached: the reference of a case is computed once and left unchanged)."""
    key = case["name"]
    if key in _P_CACHE:
        return _P_CACHE[key]
    D, k, rc = case["D"], case["k"], case["row_constant"]
    rng = np.random.default_rng(D * 1009 + k)
    kind = case["kind"]
    if kind == "random":
        P = _rows(rng, D, k, rc)
    elif kind == "distinct":
        P = _distinct_rows(rng, D, k, rc)
    elif kind == "copies":
        P = _rows(rng, case["protos"], k, rc)[rng.integers(0, case["protos"], D)]
    elif kind == "zeros":  # documents 0 .. 70 and the last 70 are copies of one row
        P = _rows(rng, D, k, rc)
        P[:71] = P[100]
        P[D - 70:] = P[100]
    elif kind == "clustered":  # a few prototype rows copied to all documents but the outliers; document D - 1 is a copy
        npro, nout = case.get("protos", CLUSTER_PROTOS), case.get("outliers", CLUSTER_OUTLIERS)
        rows = _distinct_rows(rng, npro + nout, k, rc)
        P = rows[rng.integers(0, npro, D)]
        P[:npro] = rows[:npro]  # every prototype occurs
        where = np.sort(rng.choice(np.arange(npro, D - 1), nout, replace=False))
        P[where] = rows[npro:]
    else:
        raise AssertionError(kind)
    P.setflags(write=False)
    if D * k <= 8 << 20:
        _P_CACHE[key] = P
    return P


def exact_inputs(case):
    """-> (V, vals, rows, offs, U): the CSC upload and the basis of a case, after asserting that the case is exact: every entry of P an
    integer, every squared distance that can occur (|p|^2 + |c|^2 + 2 |p.c| <= (|p| + |c|)^2) below 2^24, the grand total below 2^53.
    B carries two more words than U spans, with entries in every third document: the projection must not see them."""
    P = exact_P(case)
    D, k = P.shape
    assert np.array_equal(P, np.floor(P)) and P.min() >= 0 and P.max() <= MAX_VAL
    assert int((P != 0).sum(axis=1).max()) <= 20
    pn = np.einsum("ij,ij->i", P, P)
    worst = 4.0 * float(pn.max())
    assert worst < 2.0 ** 24, worst
    assert worst * D < 2.0 ** 53
    V = max(k + 2, 8)
    d, w = np.nonzero(P)  # row-major: documents ascending, words ascending within a document
    junk = np.arange(0, D, 3)
    d_all = np.concatenate([d, junk])
    w_all = np.concatenate([w, np.full(junk.size, k + 1)])
    v_all = np.concatenate([P[d, w], np.full(junk.size, 7.0)])
    order = np.lexsort((w_all, d_all))
    offs = np.zeros(D + 1, np.int64)
    np.cumsum(np.bincount(d_all, minlength=D), out=offs[1:])
    U = np.zeros((V, k), np.float32, order="F")
    U[np.arange(k), np.arange(k)] = 1.0
    return V, v_all[order].astype(np.float32), w_all[order].astype(np.uint32), offs, U


_REPLAYS = {}


def expected(case):
    """replay() of an exact case, computed once.  A case with raises=True gives the Exhausted instance instead."""
    key = case["name"]
    if key not in _REPLAYS:
        try:
            _REPLAYS[key] = replay(exact_P(case), case["k"], case["rng_seed"])
        except Exhausted as e:
            _REPLAYS[key] = e
    return _REPLAYS[key]


def search_rng_seed(case, accept, tries=200):
    """the first rng_seed in 1 .. tries whose replay accept()s (how the seeds in CASES were found)."""
    P = exact_P(case)
    for s in range(1, tries + 1):
        try:
            r = replay(P, case["k"], s)
        except Exhausted as e:
            r = e
        if accept(r, s):
            return s
    raise AssertionError("no rng_seed in 1 .. %d reaches the edge of %s" % (tries, case["name"]))


# ---- the weak certificate for generic inputs ------------------------------------------------------------------------------------------------
AMBIGUOUS_CAP = 0.02


def admissible(P64, k, rng_seed, seeds, rounds, slack=None):
    """Teacher-forced on a seed list (the device's): P64 (D, k) the fp64 projection.  Round by round the seeds taken so far are folded into
    the fp64 min_dist; every distance may sit anywhere in [max(md - E, 0), md + E], E = slack (|p_d|^2 + max_s |p_s|^2) over the seeds
    folded in, so a prefix sum and a suffix sum each lie between the sums of those ends.  The set of a die is every document whose
    interval can hold it.  The next seed of the list must lie in its die's set; a die that takes none must have an already
    chosen document in its set; the list must be used up in exactly `rounds` rounds.  A die is ambiguous when its set holds the list's next
    seed AND an already chosen document (the forcing takes the seed); with_chosen counts every die whose set holds a chosen document at all.  -> dict(dice, ambiguous, share, widest, with_chosen, allowance: the
    summed E of the last round, for the residual, total, last)."""
    slack = header_slack() if slack is None else slack
    P64 = np.asarray(P64, np.float64)
    D = P64.shape[0]
    seeds = [int(s) for s in seeds]
    assert len(seeds) == k and len(set(seeds)) == k and max(seeds) < D
    pn = np.einsum("ij,ij->i", P64, P64)
    rng = HostRng(rng_seed)
    first = (rng.next31() * FIRST_MUL) % D
    assert seeds[0] == first, "first seed %d, the rule gives %d" % (seeds[0], first)
    pos, batch = 1, [first]
    md = np.full(D, np.inf)
    dice = amb = widest = with_chosen = 0
    total = last = allowance = 0.0
    for r in range(1, rounds + 1):
        assert pos < k, "the seeds were complete after %d rounds, the device reports %d" % (r - 1, rounds)
        md = _fold(md, P64, pn, batch, False)
        E = slack * (pn + pn[np.asarray(seeds[:pos], np.int64)].max())
        cumL = np.concatenate([[0.0], np.cumsum(np.maximum(md - E, 0.0))])
        cumH = np.concatenate([[0.0], np.cumsum(md + E)])
        total, last, allowance = float(md.sum()), float(md[D - 1]), float(E.sum() + E[D - 1])
        batch = []
        for f in [rng.fraction() for _ in range(ndraw_at(pos, k))]:
            if pos >= k:
                continue
            dice += 1
            # document i holds the die iff A_i <= f T < A_(i+1), i.e. (1 - f) A_i - f R_i <= 0 < (1 - f) A_(i+1) - f R_(i+1) with the prefix A
            # and the suffix R = T - A, sums over disjoint documents: each side at the favourable ends of its two sums (both keys ascend)
            a = min(int(np.searchsorted((1.0 - f) * cumH[1:] - f * (cumL[D] - cumL[1:]), 0.0, side="left")), D - 1)
            b = min(max(int(np.searchsorted((1.0 - f) * cumL[:-1] - f * (cumH[D] - cumH[:-1]), 0.0, side="right")) - 1, a), D - 1)
            widest = max(widest, b - a + 1)
            taken = np.asarray(seeds[:pos], np.int64)
            has_chosen = bool(((taken >= a) & (taken <= b)).any())
            with_chosen += has_chosen
            if a <= seeds[pos] <= b:
                amb += has_chosen
                batch.append(seeds[pos])
                pos += 1
            else:
                assert has_chosen, ("round %d: the die %.17g x total admits documents %d .. %d; the next seed is %d and no chosen document "
                                    "lies there" % (r, f, a, b, seeds[pos]))
    assert pos == k, "%d of %d seeds placed in %d rounds" % (pos, k, rounds)
    return dict(dice=dice, ambiguous=amb, share=amb / max(dice, 1), widest=widest, with_chosen=with_chosen, allowance=allowance,
                total=total, last=last)


# ---- the generic corpus -----------------------------------------------------------------------------------------------------------------------
# rng_seed: the first in 1 .. 60 at which the float32 simulation of the library's rule has the smallest ambiguous share, searched on the CPU
# before any device run.  k = 65: none of 64 dice.  k = 300: 5 of 300 (1.7 %); over the 60 seeds the simulation gives 5 to 14 of 300 — with
# 300 of 6001 documents chosen and sets of 3 to 7 documents, a set holds a chosen document for one die in 30 — so the cap of 2 % (6 dice)
# is met by this seed and two others only.  The sets are the tight ones (admissible: prefix and suffix sums each at their favourable end);
# with the slack of the prefix and of the total simply added the simulation has 26 to 36 ambiguous dice of 300.  At these seeds the
# plainer count — every die whose set holds ANY chosen document (with_chosen) — is 0 of 64 and 6 of 300, inside the cap as well, and the
# tests assert both.
GENERIC_SEEDS = {65: 2, 300: 4}
_GENERIC = {}


def generic_inputs(k):
    """The small corpus of the k-means certificate (V = 2003, D = 6001, row-constant values) with a random orthonormal U of k columns.
    -> dict(V, D, vals, rows, offs, U (float32, column-major), P64 (the fp64 projection under the float32 U), rng_seed)."""
    if k not in _GENERIC:
        import sys
        if _ROOT not in sys.path:
            sys.path.insert(0, _ROOT)
        import scipy.sparse as sp
        from tools.synth import make_B
        B = make_B(2003, 6100, 20, 3)
        D = 6001
        n = int(B["offs"][D])
        vals, rows, offs = B["vals"][:n].copy(), B["rows"][:n].copy(), B["offs"][:D + 1].copy()
        U = np.asfortranarray(np.linalg.qr(np.random.default_rng(17 * k).standard_normal((2003, k)))[0], dtype=np.float32)
        X = sp.csc_matrix((vals.astype(np.float64), rows.astype(np.int64), offs.astype(np.int64)), shape=(2003, D))
        _GENERIC.clear()
        _GENERIC[k] = dict(V=2003, D=D, vals=vals, rows=rows, offs=offs, U=U, P64=np.asarray(X.T @ U.astype(np.float64)),
                           rng_seed=GENERIC_SEEDS[k])
    return _GENERIC[k]
