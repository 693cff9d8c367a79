"""The rule of isle_hip_compare_models / isle_hip_match_topics without the library and without a GPU.  tests/match_rule.py states it in
numpy; here it is held to a brute-force statement on Python numbers (the sort-and-sweep and, so that the equivalence is on record, the
rounds of mutually best pairs the device runs), the cases of its table are shown to hit what they aim at, and
isle_amd/csrc/match_host.h (match_greedy, model_dist_plain, the refusals' texts, the slice rule) is held to the rule on every case
through isle_amd/host/match_host_main.cpp, built here with the address and undefined-behaviour sanitizers (a stand-alone program, script
on stdin, lines out).  Every comparison is == : ids, bits of doubles, texts."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import match_rule as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_doubles(a, b):
    """equal bit for bit, NaNs compared as positions"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    a, b = a.reshape(-1), b.reshape(-1)
    return np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def brute_sweep(d):
    """sort the finite entries by (value, i, j) as Python floats (-0.0 == 0.0 there too), sweep"""
    na, nb = d.shape
    edges = sorted((float(d[i, j]), i, j) for i in range(na) for j in range(nb) if math.isfinite(d[i, j]))
    ma, mb = [-1] * na, [-1] * nb
    for _, i, j in edges:
        if ma[i] < 0 and mb[j] < 0:
            ma[i], mb[j] = j, i
    return ma, mb


def brute_rounds(d):
    """rounds of mutually best pairs on Python numbers -> (match_a, rounds that matched)"""
    na, nb = d.shape
    ma, mb, rounds = [-1] * na, [-1] * nb, 0
    while True:
        def best(own, others, at):
            cand = [(float(at(o)), o) for o in others if math.isfinite(at(o))]
            return min(cand)[1] if cand else -1
        free_i, free_j = [i for i in range(na) if ma[i] < 0], [j for j in range(nb) if mb[j] < 0]
        rb = {i: best(i, free_j, lambda j: d[i, j]) for i in free_i}
        cb = {j: best(j, free_i, lambda i: d[i, j]) for j in free_j}
        got = [(i, j) for i, j in rb.items() if j >= 0 and cb[j] == i]
        if not got:
            return ma, rounds
        for i, j in got:
            ma[i], mb[j] = j, i
        rounds += 1


@pytest.mark.parametrize("case", mr.MATCH_CASES, ids=lambda c: c.name)
def test_the_numpy_matching_is_the_brute_force_statement_and_the_rounds_reach_it(case):
    want = mr.match_rule(case.dist)
    ma, mb = brute_sweep(case.dist)
    assert want["match_a"].tolist() == ma and want["match_b"].tolist() == mb
    assert all(same_doubles(want["match_dist"][i], case.dist[i, ma[i]] if ma[i] >= 0 else np.nan) for i in range(len(ma)))
    assert want["n_matched"] == sum(j >= 0 for j in ma)
    ra, rounds = brute_rounds(case.dist)
    assert ra == ma and rounds == want["rounds"]                       # the device's mechanism gives the sweep's matching
    assert mr.rounds_of(case.dist)[0].tolist() == ma


def test_sweep_and_rounds_agree_on_random_small_matrices():
    rng = np.random.default_rng(3)
    for n in range(200):
        na, nb = rng.integers(1, 7, size=2)
        d = rng.integers(0, 3, size=(na, nb)).astype(np.float64)
        d[rng.random((na, nb)) < 0.15] = np.nan
        d[rng.random((na, nb)) < 0.1] = -0.0
        if n % 5 == 0:
            d[rng.integers(na), :] = np.nan
        assert brute_rounds(d)[0] == brute_sweep(d)[0] == mr.match_rule(d)["match_a"].tolist(), d


def test_every_case_hits_what_it_aims_at():
    by = {c.name: c for c in mr.MATCH_CASES}
    r = mr.match_rule(by["i_plus_j"].dist)
    assert r["rounds"] == 130 and r["match_a"].tolist() == list(range(130)) and r["n_matched"] == 130
    assert any(np.unique(c.dist[np.isfinite(c.dist)]).size < np.isfinite(c.dist).sum() / 3 for c in mr.MATCH_CASES if c.name.startswith("ints"))   # many ties
    z = by["zeros"].dist
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    rz = mr.match_rule(z)
    assert np.signbit(rz["match_dist"][rz["match_a"] >= 0]).any()                     # a matched -0 is reported with its own bits
    assert mr.match_rule(by["nan_row"].dist)["match_a"][3] == -1 and mr.match_rule(by["nan_row"].dist)["n_matched"] == 7
    rc = mr.match_rule(by["nan_col"].dist)
    assert rc["match_b"][0] == -1 and rc["match_b"][5] == -1 and rc["n_matched"] == 6
    ra = mr.match_rule(by["all_nan"].dist)
    assert ra["n_matched"] == 0 and math.isnan(ra["mean_dist"]) and ra["rounds"] == 0 and (ra["match_a"] == -1).all()
    ri = mr.match_rule(by["infs"].dist)
    assert ri["match_a"][4] == -1 and np.isfinite(ri["match_dist"][ri["match_a"] >= 0]).all() and np.isinf(by["infs"].dist).any()
    assert {c.dist.shape[0] > c.dist.shape[1] for c in mr.MATCH_CASES} == {True, False} and by["one"].dist.shape == (1, 1)
    rn = mr.match_rule(by["near_diagonal"].dist)
    assert by["near_diagonal"].dist.shape == (129, 65) and rn["n_matched"] == 65 and rn["rounds"] <= 2 and (rn["match_dist"][rn["match_a"] >= 0] < 0.5).all()
    # distances: the vocabularies and the sides the kernel's edges ask for
    T, Ch = mr.MC_TILE, mr.MC_CHUNK
    Vs = {c.a.shape[0] for c in mr.DIST_CASES}
    assert {1, 2, 3, 4, 5, Ch - 1, Ch, Ch + 1, 2 * Ch + 3, 4 * Ch + 1} <= Vs
    sides = {(c.a.shape[1], c.b.shape[1]) for c in mr.DIST_CASES}
    assert {(1, 2 * T + 1), (2 * T + 1, 1), (T, T), (T - 1, T), (T, T + 1), (1, 1), (2, 2)} <= sides and len(mr.DIST_CASES) <= 48
    for c in mr.DIST_CASES:
        for m in (c.a, c.b):
            f = m[np.isfinite(m)].astype(np.float64)
            assert np.array_equal(f * 4096, np.round(f * 4096)) and f.min() >= 0 and f.max() <= 1 and m.flags.f_contiguous
    by = {c.name: c for c in mr.DIST_CASES}
    d = mr.dist_rule(by["nonfinite"].a, by["nonfinite"].b)
    nan_rows, nan_cols = np.isnan(d).all(axis=1), np.isnan(d).all(axis=0)
    assert np.nonzero(nan_rows)[0].tolist() == [2, T] and np.nonzero(nan_cols)[0].tolist() == [1, 4]
    assert np.isfinite(d[~nan_rows][:, ~nan_cols]).all()
    assert by["same"].same and by["same"].a is by["same"].b and (np.diag(mr.dist_rule(by["same"].a, by["same"].b)) == 0).all()
    t = mr.dist_rule(by["ties"].a, by["ties"].b)
    assert (t == t[0]).all() and t[0, 1] == t[0, 2] and np.unique(t[0]).size == 3
    assert mr.match_rule(t)["match_a"].tolist() == np.argsort(t[0], kind="stable").tolist() + [-1] * 5      # ties go to the smaller row, then the smaller column
    g = mr.GENERIC
    assert g.a.shape == (1000, 5) and g.b.shape == (1000, 7) and abs(g.a.sum(axis=0) - 1).max() < 1e-5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("match_host") / "match_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "match_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    text = "\n".join(" ".join(str(t) for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o.pop("cmd") for o in out] == [line[0] for line in script]
    return out


def lst(a):
    a = np.asarray(a).reshape(-1)
    return [a.size] + [int(x) for x in a]


COMPARE_ARGS = [  # vocab, side a, side b: (which, host_given, cols, resident, res_vocab, res_cols)
    (100, (2, 1, 5, 0, 0, 0), (2, 1, 7, 0, 0, 0)), (0, (2, 1, 5, 0, 0, 0), (2, 1, 7, 0, 0, 0)), (0xfffffff1, (2, 1, 5, 0, 0, 0), (2, 1, 7, 0, 0, 0)),
    (100, (4, 1, 5, 0, 0, 0), (2, 1, 7, 0, 0, 0)), (100, (2, 1, 5, 0, 0, 0), (-1, 1, 7, 0, 0, 0)), (100, (2, 1, 0, 0, 0, 0), (2, 1, 7, 0, 0, 0)),
    (100, (2, 1, 5, 0, 0, 0), (2, 1, 8193, 0, 0, 0)), (100, (2, 1, 8192, 0, 0, 0), (2, 1, 8192, 0, 0, 0)), (100, (2, 0, 5, 0, 0, 0), (2, 1, 7, 0, 0, 0)),
    (100, (2, 1, 5, 0, 0, 0), (2, 0, 7, 0, 0, 0)), (100, (0, 0, 5, 0, 100, 5), (3, 0, 7, 1, 100, 7)), (100, (0, 0, 5, 1, 100, 5), (1, 0, 5, 0, 100, 5)),
    (100, (0, 0, 5, 1, 100, 5), (3, 0, 7, 0, 100, 7)), (100, (0, 0, 5, 1, 100, 5), (3, 0, 7, 1, 99, 7)), (100, (0, 0, 5, 1, 101, 5), (3, 0, 7, 1, 100, 7)),
    (100, (0, 0, 6, 1, 100, 5), (3, 0, 7, 1, 100, 7)), (100, (0, 0, 5, 1, 100, 5), (3, 0, 7, 1, 100, 8)), (100, (0, 0, 5, 1, 100, 5), (0, 0, 5, 1, 100, 5)),
    (100, (1, 0, 5, 1, 100, 5), (3, 0, 7, 1, 100, 7))]
COMPARE_TEXTS = [
    "", "compare_models: vocab = 0 outside 1 .. 4294967280", "compare_models: vocab = 4294967281 outside 1 .. 4294967280",
    "compare_models: side a: unknown model 4", "compare_models: side b: unknown model -1", "compare_models: side a: 0 columns outside 1 .. 8192",
    "compare_models: side b: 8193 columns outside 1 .. 8192", "", "compare_models: side a: null host model", "compare_models: side b: null host model",
    "compare_models: side a: no catch model is resident", "compare_models: side b: no average model is resident",
    "compare_models: side b: no loaded model is resident", "compare_models: side b: vocab = 100, the loaded model's is 99",
    "compare_models: side a: vocab = 100, the catch model's is 101", "compare_models: side a: 6 columns, the catch model has 5",
    "compare_models: side b: 7 columns, the loaded model has 8", "", ""]
SLICE_ARGS = [(V, ka, kb, cus, asked) for V in (1, 63, 64, 65, 1000, 50000, 100000, 0xfffffff0) for ka, kb in ((1, 1), (200, 200), (1000, 1000), (64, 65), (8192, 8192))
              for cus in (1, 256) for asked in (0, 1, 2, 3, 7, 2000)]


def test_the_header_answers_as_the_rule_does(exe):
    script = [["consts"]]
    script += [["compare", v] + list(a) + list(b) for v, a, b in COMPARE_ARGS]
    margs = [(1, 1, 1), (1, 0, 5), (1, 5, 0), (1, 8193, 1), (1, 8192, 8192), (0, 3, 3), (0, 0, 3)]
    script += [["matchargs"] + list(m) for m in margs]
    script += [["slicesargs", s] for s in (0, 1, 7, -1)]
    n_head = len(script)
    script += [["slices"] + list(s) for s in SLICE_ARGS]
    n_slices = len(script)
    dist_cases = mr.DIST_CASES + [mr.GENERIC]
    for c in dist_cases:
        script.append(["dist", c.a.shape[0], c.a.shape[1], c.b.shape[1]] + lst(c.a.reshape(-1, order="F").view(np.uint32)) + lst(c.b.reshape(-1, order="F").view(np.uint32)))
    n_dist = len(script)
    for c in mr.MATCH_CASES:
        script.append(["match", c.dist.shape[0], c.dist.shape[1]] + lst(bits(c.dist)))
    out = run(exe, script)
    assert out[0] == dict(tile=mr.MC_TILE, chunk=mr.MC_CHUNK, max_topics=mr.MAX_TOPICS, max_vocab=mr.MAX_VOCAB, partial_bytes=mr.PARTIAL_BYTES,
                          slice_waves=mr.SLICE_WAVES, models=[0, 1, 2, 3])
    at = 1
    got = [o["text"] for o in out[at:at + len(COMPARE_ARGS)]]
    assert got == [mr.check_compare(a, b, v) for v, a, b in COMPARE_ARGS] == COMPARE_TEXTS
    at += len(COMPARE_ARGS)
    assert [o["text"] for o in out[at:at + len(margs)]] == [mr.check_match(*m) for m in margs] == [
        "", "match_topics: 0 x 5 outside 1 .. 8192 on each side", "match_topics: 5 x 0 outside 1 .. 8192 on each side",
        "match_topics: 8193 x 1 outside 1 .. 8192 on each side", "", "match_topics: null dist_host", "match_topics: 0 x 3 outside 1 .. 8192 on each side"]
    at += len(margs)
    assert [o["text"] for o in out[at:n_head]] == [mr.check_slices(s) for s in (0, 1, 7, -1)] == ["", "", "", "model_dist_slices: slices = -1 is negative"]
    for (V, ka, kb, cus, asked), o in zip(SLICE_ARGS, out[n_head:n_slices]):
        s, b = o["slices"], o["bounds"]
        assert s == mr.slices_rule(V, ka, kb, cus, asked) and b == mr.slice_bounds(V, s), (V, ka, kb, cus, asked)
        assert s >= 1 and b[0] == 0 and b[-1] == V and all(x <= y for x, y in zip(b, b[1:])) and len(b) == s + 1       # covers V, monotone
        assert all(x % mr.MC_CHUNK == 0 or x == V for x in b) and o["words"] % mr.MC_CHUNK == 0 and s <= max(1, -(-V // mr.MC_CHUNK))
        assert s * ka * kb * 8 <= mr.PARTIAL_BYTES or s == 1
        if asked >= 1 and ka * kb * 8 * asked <= mr.PARTIAL_BYTES:
            assert s == min(asked, max(1, -(-V // mr.MC_CHUNK)))
    assert out[n_head + SLICE_ARGS.index((50000, 200, 200, 256, 0))]["slices"] == 64 and out[n_head + SLICE_ARGS.index((100000, 1000, 1000, 256, 0))]["slices"] == 4
    for c, o in zip(dist_cases, out[n_slices:n_dist]):
        want = mr.dist_rule(c.a, c.b)
        got = np.array(o["dist"], np.uint64).view(np.float64).reshape(want.shape)
        if c.name == "generic":      # not exactly representable sums: the plain loop's order against numpy's, within the rule's own bound
            assert (np.abs(got - want) <= 2 * 1000 * 2.0 ** -53 * want).all()
        else:
            assert same_doubles(got, want), c.name
    for c, o in zip(mr.MATCH_CASES, out[n_dist:]):
        want = mr.match_rule(c.dist)
        assert o["match_a"] == want["match_a"].tolist() and o["match_b"] == want["match_b"].tolist() and o["n_matched"] == want["n_matched"], c.name
        assert same_doubles(np.array(o["match_dist"], np.uint64).view(np.float64), want["match_dist"]), c.name
        assert same_doubles(np.array([o["mean_dist"]], np.uint64).view(np.float64), np.array([want["mean_dist"]])), c.name


def test_the_headers_carry_the_same_constants():
    host = open(os.path.join(ROOT, "isle_amd", "csrc", "match_host.h")).read()
    assert "constexpr int MC_TILE = %d;" % mr.MC_TILE in host and "constexpr int MC_CHUNK = %d;" % mr.MC_CHUNK in host
    assert "constexpr int MC_MAX_TOPICS = %d;" % mr.MAX_TOPICS in host and "out of scope" in host.lower() and "hungarian" in host.lower()
    assert "MC_MODEL_CATCH = 0, MC_MODEL_AVG = 1, MC_MODEL_HOST = 2, MC_MODEL_LOADED = 3" in host
    lib = open(os.path.join(ROOT, "include", "isle_hip.h")).read()
    for name, value in (("ISLE_MODEL_CATCH", 0), ("ISLE_MODEL_AVG", 1), ("ISLE_MODEL_HOST", 2), ("ISLE_MODEL_LOADED", 3)):
        assert "#define %s %d" % (name, value) in lib
    for f in ("match_host.h", "route_host.h"):      # plain C++: includable from a stand-alone program
        assert "hip/hip_runtime" not in open(os.path.join(ROOT, "isle_amd", "csrc", f)).read()
    assert "route_model_dist_slices" in open(os.path.join(ROOT, "isle_amd", "csrc", "route_host.h")).read()
