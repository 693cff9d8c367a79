"""Held-out scores per document on the device (isle_hip_score_docs; HotPath.score_docs / completion_score; isle_amd/csrc/score_docs.hip)
against the rule of tests/score_rule.py.  On every case of the table and in every mode z_out, tokens, unscored_tokens, unscored_entries and
floored equal the rule bit for bit, as do the "prob" scores without normalise; a second call gives the same bits in every mode; the "log"
scores lie within g / (1 - g) sum c |ln z| of the exact sums (mpmath), g = (2 K + 1 + ceil(n / 64) + 6) 2^-53, K = 4 (score_rule.K_LOG_ULP).
The largest observed share of that bound is printed (run with -s), not asserted beyond the bound.  Both sources of the weights and both of
the entries give the same bits on the same data, with doc_begin > 0; every refusal carries its text and leaves A and the inference entries
as they were; every fault found on the device names the first offender; completion_score equals its steps done by hand and prefers the
planted model to the same model with its rows shuffled among the words.  tests/test_score_rule_cpu.py holds the rule itself to the header
and shows that wrong orders and precisions change the bits compared here."""
import mpmath
import numpy as np
import pytest

import score_rule as sr
from isle_amd import IsleHipError, hot_path

pytestmark = pytest.mark.gpu
EXACT = ("tokens", "unscored_tokens", "unscored_entries", "floored")
MEASURE = {sr.LOG: "log", sr.PROB: "prob"}


def call(hp, c, mode, with_z=True, **kw):
    args = dict(model=c.model, weights=c.weights_arg(), entries=c.entries_arg(), measure=MEASURE[mode[0]], normalise=bool(mode[1]), floor=mode[2],
                with_z=with_z)
    args.update(kw)
    return hp.score_docs(**args)


def same(got, want, what, score=True, z=True):
    assert got["score"].dtype == np.float64 and got["unscored_entries"].dtype == np.uint32 and got["floored"].dtype == np.uint32, what
    for key in EXACT + (("z",) if z else ()) + (("score",) if score else ()):
        g = got[key] if got[key].dtype == np.uint32 else got[key].view(np.uint64)
        assert np.array_equal(g, want[key]), (what, key)


def within_bound(c, z, floor, score, what):
    """-> the largest |score - exact| / bound over the documents that have a bound"""
    worst = 0.0
    for r, (ex, ab, bound) in enumerate(sr.exact_log(c, z, floor)):
        err = abs(mpmath.mpf(float(score[r])) - ex)
        assert err <= bound, (what, r, float(err), float(bound))
        if ab:
            worst = max(worst, float(err / bound))
        else:
            assert score[r].view(np.uint64) == 0, (what, r)  # no scored entry: +0.0, the bits
    return worst


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: c.name)
def test_every_case_of_the_table_is_the_rule(hp, case):
    worst = 0.0
    for mode in sr.MODES:
        want = sr.rule(case, *mode)
        exact_score = mode[0] == sr.PROB and not mode[1]
        got = call(hp, case, mode)
        same(got, want, (case.name, mode), score=exact_score)
        again = call(hp, case, mode)
        for key in EXACT + ("z", "score"):
            assert got[key].tobytes() == again[key].tobytes(), (case.name, mode, key, "a second call")
        assert got["total_score"] == hot_path.score_total(got["score"]) and got["total_tokens"] == float(sr.fold(got["tokens"], sequential=True))
        if mode[0] == sr.LOG:
            worst = max(worst, within_bound(case, got["z"], mode[2], got["score"], (case.name, mode)))
            with np.errstate(all="ignore"):
                ppl = np.exp(-np.float64(got["total_score"]) / np.float64(got["total_tokens"]))
            assert got["perplexity"] == float(ppl) or (np.isnan(ppl) and np.isnan(got["perplexity"]))
        else:
            assert got["perplexity"] is None
    print("score_docs %s: the largest |score - exact| is %.4f of the log bound" % (case.name, worst))


def test_without_z_the_same_numbers(hp):
    c = sr.BY_NAME["v65_k5"]
    for mode in sr.MODES:
        a, b = call(hp, c, mode), call(hp, c, mode, with_z=False)
        assert "z" not in b and all(a[k].tobytes() == b[k].tobytes() for k in EXACT + ("score",))


# ---- the resident sources: A and the entries of infer_resident, documents [B0, E0) ------------------------------------------------------------
V, D, K, SEED = 500, 700, 5, 3
B0, E0 = 37, 650


def planted(seed=SEED):
    return sr.planted(V, D, K, seed)


@pytest.fixture(scope="module")
def resident(hp):
    m, cnt, word, off = planted()
    m[:, 3] = np.where(np.arange(V) % 7 == 0, 0.0, m[:, 3])  # some exact zeros
    hp.upload_counts(V, cnt, word, off)
    with pytest.raises(IsleHipError, match="score_docs: no resident result"):
        hp.score_docs(m, weights="infer", entries="resident")
    inf = hp.infer_resident(m, docs=(B0, E0), min_weight=0.0)
    assert inf["nentries"] > 1000
    sl = slice(int(off[B0]), int(off[E0]))
    entries = (cnt[sl], word[sl], off[B0:E0 + 1] - off[B0])
    return dict(model=m, A=(cnt, word, off), inf=inf, weights=(inf["offs"], inf["topic"], inf["weight"]), entries=entries)


def intact(hp, res):
    a = hp.get_A()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, res["A"]))
    again = hp.infer_entries(E0 - B0, res["inf"]["nentries"])
    assert all(x.tobytes() == res["inf"][name].tobytes() for x, name in zip(again, ("offs", "topic", "weight")))


def test_both_sources_of_the_weights_and_of_the_entries_give_the_same_bits(hp, resident):
    m = resident["model"]
    c = sr.Case("resident", m, resident["weights"], resident["entries"])
    for mode in sr.MODES:
        kw = dict(measure=MEASURE[mode[0]], normalise=bool(mode[1]), floor=mode[2])
        want = sr.rule(c, *mode)
        hh = hp.score_docs(m, resident["weights"], resident["entries"], with_z=True, **kw)
        same(hh, want, ("host, host", mode), score=mode[0] == sr.PROB and not mode[1])
        for what, got in (("infer, resident", hp.score_docs(m, "infer", "resident", **kw)),
                          ("infer, resident, docs", hp.score_docs(m, "infer", "resident", docs=(B0, E0), **kw)),
                          ("infer, host", hp.score_docs(m, "infer", resident["entries"], **kw)),
                          ("host, resident", hp.score_docs(m, resident["weights"], "resident", docs=(B0, E0), **kw))):
            for key in EXACT + ("score",):
                assert got[key].tobytes() == hh[key].tobytes(), (what, mode, key)
        if mode[0] == sr.LOG:
            within_bound(c, hh["z"], mode[2], hh["score"], ("resident", mode))
    intact(hp, resident)


def test_every_refusal_carries_its_text_and_leaves_what_is_resident(hp, resident):
    m, w, e = resident["model"], resident["weights"], resident["entries"]
    probe = sr.BY_NAME["v65_k3"]
    want = sr.rule(probe, sr.PROB, 0, 0.0)
    for name, a, kw, text in sr.REFUSALS:
        args = dict(model=a["model"], weights=(a["woff"], a["wtopic"], a["wweight"]), entries=(a["cnt"], a["word"], a["off"]))
        args.update(kw)
        with pytest.raises(IsleHipError) as err:
            hp.score_docs(**args)
        assert "isle_hip error -1" in str(err.value) and text in str(err.value), (name, str(err.value))
        intact(hp, resident)
    n = E0 - B0
    for name, call_it, text in (
            ("ncols", lambda: hp.score_docs(np.zeros((65, 1025), np.float32), probe.weights_arg(), probe.entries_arg()), r"ncols = 1025 not in \[1, 1024\]"),
            ("rows", lambda: hp.score_docs(m, "infer", (e[0][:e[2][5]], e[1][:e[2][5]], e[2][:6])),
             "num_rows = 5, the resident inference result has %d rows" % n),
            ("begin", lambda: hp.score_docs(m, "infer", "resident", docs=(B0 + 1, E0 + 1)),
             "doc_begin = %d, the resident inference result begins at document %d" % (B0 + 1, B0)),
            ("range", lambda: hp.score_docs(m, w, "resident", docs=(D - 1, D - 1 + n)), r"documents \[%d, %d \+ %d\) of %d" % (D - 1, D - 1, n, D)),
            ("vocab", lambda: hp.score_docs(np.zeros((V + 1, K), np.float32), w, "resident", docs=(B0, E0)),
             "the model has %d words, the count matrix %d" % (V + 1, V)),
            ("topics", lambda: hp.score_docs(np.zeros((V, K + 1), np.float32), "infer", "resident"),
             "ncols = %d, the resident inference result has %d topics" % (K + 1, K))):
        with pytest.raises(IsleHipError, match="score_docs: .*" + text):
            call_it()
        intact(hp, resident)
    z = np.zeros(8, np.float64)
    zp, lib, h = z.ctypes.data, hp._lib, hp._h
    one = np.ones(1, np.float32).ctypes.data
    for ws, es, text in ((1, 1, "unknown weights source 1"), (7, 1, "unknown weights source 7"), (2, 2, "unknown entries source 2")):
        with pytest.raises(IsleHipError, match="score_docs: " + text):
            hp._chk(lib.isle_hip_score_docs(h, 2, one, 1, 1, ws, 0, None, None, None, es, 0, None, None, None, 0, 0, 0.0, zp, zp, zp, zp, zp, None))
    with pytest.raises(IsleHipError, match="score_docs: null w_offsets with 3 rows"):
        hp._chk(lib.isle_hip_score_docs(h, 2, one, 1, 1, 2, 3, None, None, None, 1, 0, None, None, None, 0, 0, 0.0, zp, zp, zp, zp, zp, None))
    with pytest.raises(IsleHipError, match="score_docs: null score / tokens"):
        hp._chk(lib.isle_hip_score_docs(h, 2, one, 1, 1, 2, 3, zp, None, None, 1, 0, None, None, zp, 0, 0, 0.0, None, zp, zp, zp, zp, None))
    with pytest.raises(IsleHipError, match="score_docs: z_out with ISLE_SCORE_RESIDENT"):
        hp._chk(lib.isle_hip_score_docs(h, 2, resident["model"].ctypes.data, V, K, 0, n, None, None, None, 0, B0, None, None, None, 0, 0, 0.0, zp, zp, zp,
                                        zp, zp, zp))
    with pytest.raises(ValueError, match="with_z needs a caller's CSC"):
        hp.score_docs(m, "infer", "resident", with_z=True)
    intact(hp, resident)
    same(call(hp, probe, (sr.PROB, 0, 0.0)), want, "after the refusals")


def test_every_fault_found_on_the_device_names_the_first_offender(hp, resident):
    probe = sr.BY_NAME["v65_k3"]
    want = sr.rule(probe, sr.LOG, 1, sr.FLOOR)
    for name, a, text in sr.FAULTS:
        with pytest.raises(IsleHipError) as err:
            hp.score_docs(a["model"], (a["woff"], a["wtopic"], a["wweight"]), (a["cnt"], a["word"], a["off"]), measure="prob")
        assert "isle_hip error -1" in str(err.value) and text in str(err.value), (name, str(err.value))
        same(call(hp, probe, (sr.LOG, 1, sr.FLOOR)), want, "after " + name, score=False)
    intact(hp, resident)


# ---- document completion ---------------------------------------------------------------------------------------------------------------------------
def test_completion_score_is_its_steps_by_hand_and_prefers_the_planted_model(hp):
    m, cnt, word, off = planted(SEED + 1)
    floor = 1e-9
    got = hp.completion_score(V, cnt, word, off, m, seed=5, num=1, den=2, floor=floor)
    obs, held = hot_path.split_held_out(cnt, word, off, 5, 1, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got["held"], held)) and all(x.tobytes() == y.tobytes() for x, y in zip(hp.get_A(), obs))
    assert 0.4 * cnt.size < held[0].size < 0.6 * cnt.size and got["nconverged"] > 0
    w = hp.infer_entries(D, hp.infer_resident(m, min_weight=0.0, fetch_entries=False)["nentries"])  # the same inference again: the same entries
    c = sr.Case("completion", m, w, held)
    want = sr.rule(c, sr.LOG, 1, floor)
    byhand = hp.score_docs(m, w, held, measure="log", normalise=True, floor=floor, with_z=True)
    same(byhand, want, "by hand", score=False)
    for key in EXACT + ("score",):
        assert got[key].tobytes() == byhand[key].tobytes(), key
    within_bound(c, byhand["z"], floor, got["score"], "completion")
    assert got["total_tokens"] == float(held[0].astype(np.float64).sum()) and got["unscored_entries"].sum() == 0
    shuffled = m[np.random.RandomState(1).permutation(V)]
    other = hp.completion_score(V, cnt, word, off, shuffled, seed=5, num=1, den=2, floor=floor)
    assert other["total_tokens"] == got["total_tokens"]
    assert np.isfinite(got["perplexity"]) and got["perplexity"] < other["perplexity"]
    print("completion_score: perplexity %.2f planted, %.2f with the rows shuffled, uniform %d" % (got["perplexity"], other["perplexity"], V))
