"""Two topic models compared on the device (isle_hip_compare_models / isle_hip_match_topics / isle_hip_model_dist_slices;
HotPath.compare_models, match_topics, model_dist_slices; isle_amd/csrc/model_compare.hip) held to the rule of tests/match_rule.py.

The dyadic cases hold integer multiples of 2^-12: every partial sum is exact in double, so the device's distances equal numpy's bit for
bit whatever the order, for every number of word slices.  The generic case is held to exact rational arithmetic within the bound the
rule guarantees, |dist - exact| <= 1.01 V 2^-53 exact (V 2^-53 for V additions of at most half an ulp of the running sum each, 1 % for
the second-order term): derived, not measured.  The matcher is held to the sort-and-sweep statement on every case, bits and rounds."""
from fractions import Fraction
from functools import partial

import ctypes as C
import numpy as np
import pytest

import match_rule as mr
import rank_launch
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu
_FAILED = []
_REF = {}


def want_dist(case):
    if case.name not in _REF:
        _REF[case.name] = mr.dist_rule(case.a, case.b)     # computed once, shared, never written
        _REF[case.name].setflags(write=False)
    return _REF[case.name]


def same_doubles(a, b):
    """equal bit for bit, NaNs compared as positions"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


def same_match(got, want, rounds=True):
    return (np.array_equal(got["match_a"], want["match_a"]) and np.array_equal(got["match_b"], want["match_b"]) and same_doubles(got["match_dist"], want["match_dist"])
            and got["n_matched"] == want["n_matched"] and same_doubles([got["mean_dist"]], [want["mean_dist"]]) and (not rounds or got["rounds"] == want["rounds"]))


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the slices are a setting of the context"""
    from isle_amd import HotPath
    h = HotPath(0)
    try:
        yield h
    finally:
        h.model_dist_slices(0)
        h.close()


@pytest.mark.parametrize("slices", mr.SLICES)
def test_dyadic_distances_equal_numpy_bit_for_bit(ctx, slices):
    ctx.model_dist_slices(slices)
    try:
        for c in mr.DIST_CASES:
            got = ctx.compare_models(c.a, c.a if c.same else c.b, match=False)
            want = want_dist(c)
            assert got["match_a"] is None and got["dist"].shape == want.shape
            assert same_doubles(got["dist"], want), (c.name, slices)
            if c.same:
                d = np.diag(got["dist"])
                assert (d == 0).all() and not np.signbit(d).any()
            if c.name == "nonfinite":
                assert np.isnan(got["dist"][[2, mr.MC_TILE], :]).all() and np.isnan(got["dist"][:, [1, 4]]).all() and np.isnan(got["dist"]).sum() == 2 * 5 + 2 * (mr.MC_TILE + 1) - 4
    finally:
        ctx.model_dist_slices(0)


def test_generic_floats_within_the_derived_bound_and_reproducible(ctx):
    g = mr.GENERIC
    V = g.a.shape[0]
    fa = [[Fraction(float(x)) for x in g.a[:, i]] for i in range(g.a.shape[1])]
    fb = [[Fraction(float(x)) for x in g.b[:, j]] for j in range(g.b.shape[1])]
    exact = [[sum(abs(x - y) for x, y in zip(ca, cb)) for cb in fb] for ca in fa]
    try:
        for slices in mr.SLICES:
            ctx.model_dist_slices(slices)
            one = ctx.compare_models(g.a, g.b, match=False)["dist"]
            two = ctx.compare_models(g.a, g.b, match=False)["dist"]
            assert one.tobytes() == two.tobytes(), slices
            worst = 0.0
            for i, row in enumerate(exact):
                for j, ref in enumerate(row):
                    err = abs(Fraction(float(one[i, j])) - ref)
                    worst = max(worst, float(err / ref))
                    assert err <= Fraction(101, 100) * V * Fraction(1, 2 ** 53) * ref, (slices, i, j, float(err / ref))
            print("slices %d: worst relative error %.3g, bound %.3g" % (slices, worst, 1.01 * V * 2.0 ** -53))
    finally:
        ctx.model_dist_slices(0)


def test_sums_that_must_round_stay_within_the_derived_bound(ctx):
    """The generic case above happens to sum exactly in double (24-bit terms of similar size, 1000 of them).  Here the exact sums are not
    representable: 20 011 words (odd: misaligned columns), entries spread over many binades.  The same derived bound, every slice count."""
    rng = np.random.default_rng(21)
    V = 20011
    a = np.asfortranarray(rng.random((V, 3)) ** 12 * 1000, np.float32)
    b = np.asfortranarray(rng.random((V, 2)) ** 12, np.float32)
    exact = [[sum(abs(Fraction(float(x)) - Fraction(float(y))) for x, y in zip(a[:, i], b[:, j])) for j in range(2)] for i in range(3)]
    assert all(Fraction(float(ref)) != ref for row in exact for ref in row)          # no exact sum is a double: the device has to round
    try:
        for slices in mr.SLICES:
            ctx.model_dist_slices(slices)
            got = ctx.compare_models(a, b, match=False)["dist"]
            assert got.tobytes() == ctx.compare_models(a, b, match=False)["dist"].tobytes(), slices
            for i, row in enumerate(exact):
                for j, ref in enumerate(row):
                    err = abs(Fraction(float(got[i, j])) - ref)
                    print("slices %d (%d, %d): relative error %.3g, bound %.3g" % (slices, i, j, float(err / ref), 1.01 * V * 2.0 ** -53))
                    assert err <= Fraction(101, 100) * V * Fraction(1, 2 ** 53) * ref, (slices, i, j)
    finally:
        ctx.model_dist_slices(0)


@pytest.mark.parametrize("case", mr.MATCH_CASES, ids=lambda c: c.name)
def test_the_matcher_is_the_sort_and_sweep_statement(ctx, case):
    got, want = ctx.match_topics(case.dist), mr.match_rule(case.dist)
    assert same_match(got, want), (case.name, got["rounds"], want["rounds"], got["n_matched"], want["n_matched"])
    if case.name == "i_plus_j":
        assert got["rounds"] == 130 and got["match_a"].tolist() == list(range(130))


def test_compare_models_with_matching_is_the_rule_on_the_rules_distances(ctx):
    for c in mr.DIST_CASES:
        got = ctx.compare_models(c.a, c.a if c.same else c.b)
        want = mr.match_rule(want_dist(c))
        assert same_doubles(got["dist"], want_dist(c)) and same_match(got, want), c.name
        only = ctx.compare_models(c.a, c.a if c.same else c.b, fetch_dist=False)          # the matrix never leaves the device
        assert only["dist"] is None and same_match(only, want), c.name
    t = want_dist([c for c in mr.DIST_CASES if c.name == "ties"][0])
    assert (t == t[0]).all() and t[0, 1] == t[0, 2]                                       # tied distances: rows equal, two columns equal


# ---- a trained model: the corpus of the tiny10 fixture (2000 words, 5000 documents, 10 topics, seed 0) through the pipeline up to topic_model
def _trained(hp, empty_topic):
    from isle_amd.hot_path import catchword_rank, model_rank_threshold
    from tools.synth import Corpus
    V, D, k = 2000, 5000, 10
    c = Corpus(V, D, k, 0)
    cnt, rows, offs = c.A()
    hp.upload_counts(V, cnt, rows, offs)
    hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    assign = (c.planted()[oc] % (k - 1 if empty_topic else k)).astype(np.uint32)
    hp.find_catchwords(k, max(catchword_rank(D, k), 1), assign=assign, fetch_thresholds=False)
    return hp.construct_topic_model(k, max(model_rank_threshold(D, k), 1), D, fetch_sums=False)["model"], V, k


def test_trained_model_against_its_permutation_and_its_own_text(ctx):
    catch, V, k = _trained(ctx, empty_topic=False)
    assert np.isfinite(catch).all()
    perm = np.random.default_rng(1).permutation(k)
    got = ctx.compare_models("catch", np.asfortranarray(catch[:, perm]))
    assert got["match_a"].tolist() == np.argsort(perm).tolist() and got["match_b"].tolist() == perm.tolist()      # column j of b is topic perm[j]
    assert (got["match_dist"] == 0).all() and got["n_matched"] == k and got["mean_dist"] == 0.0
    same = ctx.compare_models("catch", "catch")
    assert (np.diag(same["dist"]) == 0).all() and same["match_a"].tolist() == list(range(k))
    # against the model loaded back from its own text
    ctx.load_model_text(ctx.model_text("catch", "sparse"), V, k, "sparse")
    loaded = ctx.loaded_model()
    got = ctx.compare_models("catch", "loaded")
    want = mr.dist_rule(catch, loaded)
    bound = 2 * 1.01 * V * 2.0 ** -53          # the device and numpy each within 1.01 V 2^-53 of the exact sum
    assert (np.abs(got["dist"] - want) <= bound * want).all()
    assert got["match_a"].tolist() == list(range(k)) and got["n_matched"] == k and got["rounds"] >= 1
    assert got["match_a"].tolist() == mr.match_rule(want)["match_a"].tolist()
    assert (np.abs(got["match_dist"] - np.diag(want)) <= bound * np.diag(want)).all() and got["mean_dist"] == mr.mean_of(got["match_a"], got["match_dist"])[0]


def test_trained_model_against_the_average_model(ctx):
    catch, V, k = _trained(ctx, empty_topic=True)
    avg = ctx.avg_topic_model(k)
    assert np.isnan(avg[:, k - 1]).all() and np.isfinite(avg[:, :k - 1]).all()
    got = ctx.compare_models("catch", "avg")
    assert got["dist"].shape == (k, k) and np.isnan(got["dist"][:, k - 1]).all() and got["match_b"][k - 1] == -1
    bad_rows = ~np.isfinite(catch).all(axis=0)
    assert np.array_equal(np.isnan(got["dist"]).all(axis=1), bad_rows) and (got["match_a"][bad_rows] == -1).all()
    want = mr.dist_rule(catch, avg)
    assert np.array_equal(np.isnan(got["dist"]), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got["dist"][ok] - want[ok]) <= 2 * 1.01 * V * 2.0 ** -53 * want[ok]).all()
    assert got["n_matched"] == min((~bad_rows).sum(), k - 1) and np.isnan(got["match_dist"][got["match_a"] < 0]).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _raw_compare(hp, which_a, a, cols_a, which_b, b, cols_b, vocab):
    n, mean, rounds = C.c_uint64(), C.c_double(), C.c_uint32()
    p = lambda m: None if m is None else m.ctypes.data_as(C.c_void_p)
    hp._chk(hp._lib.isle_hip_compare_models(hp._h, which_a, p(a), cols_a, which_b, p(b), cols_b, vocab, None, None, None, None, C.byref(n), C.byref(mean),
                                            C.byref(rounds)))


def test_refusals_leave_everything_as_it_was(ctx):
    from isle_amd import HotPath, IsleHipError
    catch, V, k = _trained(ctx, empty_topic=False)        # a catch model, no average model; the loaded model of this context may exist
    before = ctx.model_top_words(5, with_weights=True)
    H = np.asfortranarray(np.ones((V, 3), np.float32))
    fresh = HotPath(0)                                    # nothing resident at all
    try:
        calls = [
            (ctx, lambda: _raw_compare(ctx, 7, None, k, 2, H, 3, V), mr.check_compare((7, 0, k, 0, 0, 0), (2, 1, 3, 0, 0, 0), V)),
            (fresh, lambda: _raw_compare(fresh, 0, None, k, 2, H, 3, V), mr.check_compare((0, 0, k, 0, 0, 0), (2, 1, 3, 0, 0, 0), V)),
            (fresh, lambda: _raw_compare(fresh, 2, H, 3, 3, None, k, V), mr.check_compare((2, 1, 3, 0, 0, 0), (3, 0, k, 0, 0, 0), V)),
            (ctx, lambda: ctx.compare_models("catch", "avg"), mr.check_compare((0, 0, k, 1, V, k), (1, 0, k, 0, V, k), V)),
            (ctx, lambda: ctx.compare_models("catch", np.asfortranarray(np.ones((V + 1, 3), np.float32))), mr.check_compare((0, 0, k, 1, V, k), (2, 1, 3, 0, 0, 0), V + 1)),
            (ctx, lambda: _raw_compare(ctx, 0, None, k + 1, 2, H, 3, V), mr.check_compare((0, 0, k + 1, 1, V, k), (2, 1, 3, 0, 0, 0), V)),
            (ctx, lambda: _raw_compare(ctx, 2, H, 3, 2, H, 3, 0), mr.check_compare((2, 1, 3, 0, 0, 0), (2, 1, 3, 0, 0, 0), 0)),
            (ctx, lambda: _raw_compare(ctx, 2, H, 3, 2, H, 3, 0xfffffff1), mr.check_compare((2, 1, 3, 0, 0, 0), (2, 1, 3, 0, 0, 0), 0xfffffff1)),
            (ctx, lambda: ctx.compare_models(np.empty((V, 0), np.float32, order="F"), H), mr.check_compare((2, 1, 0, 0, 0, 0), (2, 1, 3, 0, 0, 0), V)),
            (ctx, lambda: _raw_compare(ctx, 2, H, 3, 2, H, 8193, V), mr.check_compare((2, 1, 3, 0, 0, 0), (2, 1, 8193, 0, 0, 0), V)),
            (ctx, lambda: _raw_compare(ctx, 2, None, 3, 2, H, 3, V), mr.check_compare((2, 0, 3, 0, 0, 0), (2, 1, 3, 0, 0, 0), V)),
            (ctx, lambda: _raw_compare(ctx, 2, H, 3, 2, None, 3, V), mr.check_compare((2, 1, 3, 0, 0, 0), (2, 0, 3, 0, 0, 0), V)),
            (ctx, lambda: ctx.match_topics(np.empty((0, 3))), mr.check_match(False, 0, 3)),
            (ctx, lambda: ctx.match_topics(np.empty((3, 0))), mr.check_match(False, 3, 0)),
            (ctx, lambda: ctx._chk(ctx._lib.isle_hip_match_topics(ctx._h, None, 8193, 1, None, None, None, None, None, None)), mr.check_match(False, 8193, 1)),
            (ctx, lambda: ctx._chk(ctx._lib.isle_hip_match_topics(ctx._h, None, 3, 3, None, None, None, None, None, None)), mr.check_match(False, 3, 3)),
            (ctx, lambda: ctx.model_dist_slices(-1), mr.check_slices(-1)),
        ]
        small = mr.MATCH_CASES[0]
        for n, (hp, call, text) in enumerate(calls):
            assert text, n                                   # the rule refuses each of them
            with pytest.raises(IsleHipError) as e:
                call()
            assert str(e.value) == "isle_hip error -1: " + text, n
            assert same_match(hp.match_topics(small.dist), mr.match_rule(small.dist)), n           # a valid call still answers
        got, want = ctx.compare_models("catch", H, match=False)["dist"], mr.dist_rule(catch, H)
        assert (np.abs(got - want) <= 2 * 1.01 * V * 2.0 ** -53 * want).all()     # the device and numpy each within 1.01 V 2^-53 of the exact sum
    finally:
        fresh.close()
    after = ctx.model_top_words(5, with_weights=True)
    assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()      # nothing resident was disturbed


# ---- several ranks: every rank answers for itself, the average model is refused ---------------------------------------------------------
RANKS_V, RANKS_D, RANKS_K = 1500, 3000, 6


def _ranks_host_model():
    return mr.dyadic(np.random.default_rng(5), RANKS_V, 7)


def _worker(hp, rank, world, res):
    from isle_amd import IsleHipError
    from isle_amd.hot_path import catchword_rank, model_rank_threshold
    from tools.synth import Corpus
    V, D, k = RANKS_V, RANKS_D, RANKS_K
    c = Corpus(V, D, k, 2)
    cnt, rows, offs = c.A()
    cnt, rows, offs = np.asarray(cnt, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    b, e = D * rank // world, D * (rank + 1) // world
    hp.upload_counts(V, cnt[offs[b]:offs[e]], rows[offs[b]:offs[e]], offs[b:e + 1] - offs[b], doc_offset=b, docs_global=D)
    hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    hp.find_catchwords(k, max(catchword_rank(D, k), 1), assign=c.planted()[oc].astype(np.uint32), fetch_thresholds=False)
    res["model"] = hp.construct_topic_model(k, max(model_rank_threshold(D, k), 1), e - b, fetch_sums=False)["model"]
    got = hp.compare_models("catch", _ranks_host_model())
    for name in ("dist", "match_a", "match_b", "match_dist"):
        res[name] = got[name]
    res["scalars"] = np.array([got["n_matched"], got["rounds"]], np.int64)
    res["mean"] = np.array([got["mean_dist"]])
    try:
        hp.compare_models("avg", _ranks_host_model())
        res["avg"] = np.array("accepted")
    except IsleHipError as err:
        res["avg"] = np.array(str(err))


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("model_compare_ranks"))
    job = partial(rank_launch.launch, "model compare W2", "compare_W2", 2, tmp, rank_launch.module_command("test_gpu_model_compare", 2))
    return launch_each([(2, "W2", job)], _FAILED)


def test_two_ranks_answer_as_one_rank_does(ctx, launches):
    ranks = ranks_of(launches, 2)
    assert len(ranks) == 2 and ranks[0]["model"].tobytes() == ranks[1]["model"].tobytes()        # the catch model is replicated
    H = _ranks_host_model()
    for q, res in enumerate(ranks):
        one = ctx.compare_models(np.asfortranarray(res["model"]), H)                             # the single-rank answer on the same two models
        assert np.isfinite(one["dist"]).any()
        for name in ("dist", "match_a", "match_b", "match_dist"):
            assert one[name].tobytes() == res[name].tobytes(), (q, name)
        assert res["scalars"].tolist() == [one["n_matched"], one["rounds"]] and same_doubles(res["mean"], [one["mean_dist"]]), q
        assert str(res["avg"]) == "isle_hip error -1: compare_models: single-rank only", q
