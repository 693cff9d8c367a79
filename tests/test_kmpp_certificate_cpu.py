"""The replay of the free k-means++ draw (tests/kmpp_certificate.py) checked on the CPU: the generator against the library's and the C
library's, the replay against a brute-force form, every case against the edge it is named for, the float32 simulation of the library's
rule against both certificates, and each of eight wrong rules shown to fail."""
import ctypes
import math

import numpy as np
import pytest

import kmpp_certificate as kc
import route_reads
from kmpp_certificate import ALL_CASES, BIG_CASES, CASES, SCAN_T, SCAN_TILE, Exhausted, admissible, exact_P, expected, replay

SMALL = [c for c in CASES if not c.get("raises")]


def same(a, b):
    return (np.array_equal(a["seeds"], b["seeds"]) and a["rounds"] == b["rounds"] and a["residual"] == b["residual"]
            and np.array_equal(a["min_dist"].view(np.uint32), b["min_dist"].view(np.uint32)))


def test_generator_is_the_librarys_and_glibcs():
    import isle_amd
    lib = isle_amd.load_library()
    libc = ctypes.CDLL("libc.so.6")
    libc.rand.restype = ctypes.c_int
    for seed in (0, 1, 2, 7, 12345, 2 ** 31 - 1, 2 ** 31 + 5, 2 ** 32 + 3):
        n = 700
        out = np.empty(n, np.uint32)
        assert lib.isle_hip_host_rand(ctypes.c_uint64(seed), n, out.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(kc.host_rand(seed, n), out), seed
        if 0 < seed < 2 ** 32:
            libc.srand(ctypes.c_uint(seed))
            assert np.array_equal(out, np.array([libc.rand() for _ in range(n)], np.uint32)), seed
    assert int(kc.host_rand(1, 1)[0]) == 1804289383


def test_fraction_draws_the_low_word_first():
    g, h = kc.HostRng(5), kc.HostRng(5)
    a, b = h.next31(), h.next31()
    assert g.fraction() == (a + b * 2147483648.0) / 2.0 ** 62
    assert kc.HostRng(5, swap_words=True).fraction() == (b + a * 2147483648.0) / 2.0 ** 62


def test_draw_schedule():
    assert [kc.ndraw_at(s, 1000) for s in (1, 5, 6, 7, 9, 10, 14, 15, 230, 231, 966, 967)] == [1, 1, 2, 3, 3, 4, 4, 5, 16, 17, 32, 33]
    assert kc.ndraw_at(999, 1000) == 33 and kc.ndraw_at(10 ** 6, 9) == 5  # the cap 2 + ceil(sqrt(k))
    k16, k17 = kc.final_round_dice_k(16), kc.final_round_dice_k(17)
    assert (ALL_CASES["dice-16"]["k"], ALL_CASES["dice-17"]["k"]) == (k16, k17)
    assert max(kc.ndraw_at(s, k16) for s in range(1, k16)) == 16 and max(kc.ndraw_at(s, k17) for s in range(1, k17)) == 17


@pytest.mark.parametrize("case", CASES + BIG_CASES, ids=lambda c: c["name"])
def test_case_is_exact_and_uploads_its_projection(case):
    """exact_inputs asserts the exactness; the CSC it returns, multiplied by the U it returns, is the integer projection."""
    import scipy.sparse as sp
    V, vals, rows, offs, U = kc.exact_inputs(case)
    D, k = case["D"], case["k"]
    assert U.shape == (V, k) and np.array_equal(U.T @ U, np.eye(k, dtype=np.float32))
    assert offs.shape == (D + 1,) and np.all(np.diff(offs) >= 0) and rows.max() < V and (rows >= k).any()
    X = sp.csc_matrix((vals.astype(np.float64), rows.astype(np.int64), offs), shape=(V, D))
    assert np.array_equal(np.asarray((X.T @ sp.csr_matrix(U.astype(np.float64))).todense()), exact_P(case))
    for d in (0, D // 2, D - 1):
        assert np.all(np.diff(rows[offs[d]:offs[d + 1]].astype(np.int64)) > 0)
    if case["row_constant"]:  # every word holds one value: the LDS-banded operator can be had
        first = np.zeros(V)
        first[rows] = vals
        assert np.array_equal(first[rows], vals)


def test_every_case_reaches_its_edge():
    E = {n: expected(c) for n, c in ALL_CASES.items()}
    for n in ("tile-4095", "tile-4096", "tile-4097"):
        D = ALL_CASES[n]["D"]
        assert D == int(n[5:]) and ALL_CASES[n]["k"] == 9 and E[n]["rounds"] >= 3
    assert [math.ceil(ALL_CASES[n]["D"] / SCAN_TILE) for n in ("tile-4095", "tile-4096", "tile-4097")] == [1, 1, 2]
    assert 4095 % 64 and 4097 % 64
    b = ALL_CASES["blocks-257"]
    assert math.ceil(b["D"] / SCAN_TILE) == SCAN_T + 1 and E["blocks-257"]["rounds"] >= 2  # the carry loop of scan_blk_k makes a second trip
    assert np.unique(exact_P(b), axis=0).shape[0] <= b["protos"]
    for D in (1, 2, 63, 64, 65):
        c = ALL_CASES["tiny-%d" % D]
        assert c["D"] == D and c["k"] == min(D, 3) and E[c["name"]]["rounds"] == c["k"] - 1
    for n, front in (("zeros-front-back", True), ("zeros-back-front", False)):
        c, e = ALL_CASES[n], E[n]
        D, P = c["D"], exact_P(c)
        assert np.array_equal(P[:71], np.broadcast_to(P[0], (71, c["k"]))) and np.array_equal(P[D - 70:], np.broadcast_to(P[0], (70, c["k"])))
        first = int(e["seeds"][0])
        assert first <= 70 if front else first >= D - 70
        copies = np.flatnonzero((P == P[0]).all(axis=1))
        assert not np.isin(e["seeds"][1:].astype(np.int64), copies).any()  # no die lands in a document of zero width
        assert e["min_dist"][0] == 0 and e["min_dist"][D - 1] == 0  # last_md = 0: the residual is the whole total
        assert e["residual"] == float(np.float32(e["min_dist"].astype(np.float64).sum()))
    for n in ("clustered-20", "clustered-36", "clustered-260"):
        assert E[n]["duplicates"] >= 3, (n, E[n]["duplicates"])
    assert np.unique(exact_P(ALL_CASES["clustered-36"]), axis=0).shape[0] == kc.CLUSTER_DISTINCT
    e37, c37 = E["exhausted-37"], ALL_CASES["exhausted-37"]
    assert np.unique(exact_P(c37), axis=0).shape[0] == kc.CLUSTER_DISTINCT == c37["k"] - 1
    assert e37["zero_total_rounds"] == 1 and int(e37["seeds"][-1]) == c37["D"] - 1 and c37["D"] - 1 not in e37["seeds"][:-1]
    assert e37["residual"] == 0.0 and not e37["min_dist"].any()
    assert isinstance(E["exhausted-38"], Exhausted) and ALL_CASES["exhausted-38"]["k"] == kc.CLUSTER_DISTINCT + 2
    assert max(E["dice-16"]["dice"]) == 16 and max(E["dice-17"]["dice"]) == 17
    assert max(E["k-65"]["dice"]) <= 16 < max(E["k-300"]["dice"]) and ALL_CASES["k-225"]["k"] == 225 and ALL_CASES["clustered-260"]["k"] > 224
    assert max(E["k-1000"]["dice"]) == 33 and math.ceil(1000 / 64) == 16
    assert max(E["k-1540"]["dice"]) > 40
    for n, e in E.items():
        if not isinstance(e, Exhausted):
            # a round adds nothing only at a zero total, and then the run cannot end (module docstring)
            assert e["zero_add_rounds"] == 0 and e["fractions"] == sum(e["dice"]), n
            assert len(set(e["seeds"].tolist())) == ALL_CASES[n]["k"]


def test_exhausted_run_spins_in_rounds_that_add_nothing():
    c = ALL_CASES["exhausted-38"]
    P = exact_P(c)
    short = replay(P, c["k"] - 1, c["rng_seed"])  # the same dice: 37 seeds are found, the last by the clamp at a zero total
    assert short["zero_total_rounds"] == 1 and int(short["seeds"][-1]) == c["D"] - 1
    with pytest.raises(Exhausted):
        replay(P, c["k"], c["rng_seed"])


BRUTE = [c for c in SMALL if c["D"] <= 65] + [dict(ALL_CASES["k-65"], name="k-65-cut", D=300, k=14)]


@pytest.mark.parametrize("case", BRUTE, ids=lambda c: c["name"])
def test_replay_agrees_with_the_brute_force_form(case):
    """Python floats, math.fsum prefix sums and a linear scan; k-65-cut: 14 seeds among the first 300 documents of k-65."""
    P = exact_P(ALL_CASES["k-65"])[:300] if case["name"] == "k-65-cut" else exact_P(case)
    for seed in (case["rng_seed"], 11, 12):
        assert same(replay(P, case["k"], seed), kc.replay_brute(P, case["k"], seed)), (case["name"], seed)


@pytest.mark.parametrize("case", SMALL + BIG_CASES, ids=lambda c: c["name"])
def test_float32_simulation_equals_the_replay_on_exact_cases(case):
    """numpy float32 distances in the kernels' order of operations: on exact inputs nothing rounds, so every output is the replay's."""
    assert same(replay(exact_P(case), case["k"], case["rng_seed"], f32=True), expected(case))


@pytest.mark.parametrize("k", sorted(kc.GENERIC_SEEDS))
def test_float32_simulation_passes_the_weak_certificate_inside_the_cap(k):
    g = kc.generic_inputs(k)
    r = replay(g["P64"].astype(np.float32), k, g["rng_seed"], f32=True)
    a = admissible(g["P64"], k, g["rng_seed"], r["seeds"], r["rounds"])
    print("k = %d: %d of %d dice ambiguous, widest set %d documents" % (k, a["ambiguous"], a["dice"], a["widest"]))
    assert a["share"] <= kc.AMBIGUOUS_CAP and a["with_chosen"] / a["dice"] <= kc.AMBIGUOUS_CAP and a["widest"] <= 16
    assert abs(r["residual"] - (a["total"] - a["last"])) <= a["allowance"] + 2.0 ** -24 * a["total"]
    for wrong in ("stale-fold", "not-squared"):
        w = replay(g["P64"].astype(np.float32), k, g["rng_seed"], f32=True, wrong=wrong)
        with pytest.raises(AssertionError):
            admissible(g["P64"], k, g["rng_seed"], w["seeds"], w["rounds"])


def _failing(wrong, cases):
    out = []
    for c in cases:
        try:
            if not same(replay(exact_P(c), c["k"], c["rng_seed"], wrong=wrong), expected(c)):
                out.append(c["name"])
        except Exhausted:
            out.append(c["name"])
    return out


@pytest.mark.parametrize("wrong", [w for w in kc.WRONG_RULES if w not in ("stop-early", "carry-dropped")])
def test_wrong_rule_fails_named_cases(wrong):
    cases = [c for c in SMALL if c["k"] <= 300]
    bad = _failing(wrong, cases)
    print("%s fails %d of %d cases: %s" % (wrong, len(bad), len(cases), ", ".join(bad)))
    assert bad
    must = {"search-lo": ["tile-4096", "tiny-2", "k-65"], "stale-fold": ["tile-4097", "clustered-20"], "total-minus-last": ["k-300"],
            "swapped-words": ["tile-4095", "tiny-64"], "redraw": ["clustered-20", "clustered-36", "clustered-260"],
            "not-squared": ["tile-4096", "dice-17"]}[wrong]
    assert set(must) <= set(bad), sorted(set(must) - set(bad))


def test_dropped_block_carry_fails_blocks_257_alone():
    assert _failing("carry-dropped", [ALL_CASES["blocks-257"]]) == ["blocks-257"]
    assert _failing("carry-dropped", [ALL_CASES["tile-4097"], ALL_CASES["k-65"]]) == []  # no second trip below 256 blocks


def test_unconsumed_fractions_show_in_the_count_only():
    """The generator is local to a call: stopping at the k-th seed changes the number of fractions drawn and nothing a caller sees."""
    hit = 0
    for c in SMALL:
        e, w = expected(c), replay(exact_P(c), c["k"], c["rng_seed"], wrong="stop-early")
        assert same(e, w)
        hit += w["fractions"] < e["fractions"] == sum(e["dice"])
    assert hit >= 3


def test_every_switch_of_the_rounds_is_swept():
    """route_kmpp_plan and route_kmpp_sparse (route_host.h) are the rules of these rounds: every switch either depends on has a form."""
    rules = route_reads.route_rules()
    need = rules["route_kmpp_plan"] | rules["route_kmpp_sparse"]
    assert need == set(kc.SWITCHES), need ^ set(kc.SWITCHES)
    swept = {a for f in kc.BASE_FORMS + kc.TRACK_FORMS for a in f}
    assert swept == {kc.SWITCHES[s] for s in need}
    for name in swept:  # both settings of a 0 / 1 switch, or the switch set beside the default
        vals = {f[name] for f in kc.BASE_FORMS + kc.TRACK_FORMS if name in f}
        assert vals == ({"1"} if name == "ISLE_KMPP_HOST_DICE" else {"0", "1"}), (name, vals)


def test_the_sharded_edge_case_has_a_seed_on_either_side_of_the_cut():
    import kmpp_shard_cases as ksc
    bnd = ksc.bounds("L2", ksc.EDGE_CASE)
    seeds = expected(ALL_CASES[ksc.EDGE_CASE])["seeds"].astype(np.int64)
    assert int(bnd[1]) - 1 in seeds and int(bnd[1]) in seeds and 0 < bnd[1] < bnd[2]
    e = expected(ALL_CASES["zeros-front-back"])
    assert int(e["seeds"][0]) > 0 and e["min_dist"][0] == 0  # L3: the one-document shard holds no seed and has a zero total
    assert "exhausted-37" in ksc.NAMES  # a zero total on several ranks: the rank that holds the last document answers
