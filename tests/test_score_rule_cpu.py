"""The rule of isle_hip_score_docs without the library and without a GPU.  tests/score_rule.py states it in numpy; here
isle_amd/csrc/score_host.h (the host statement, the argument checks with their texts, the first offenders, the held-out split, the total) is
held to it bit for bit through isle_amd/host/score_host_main.cpp, built here with the address and undefined-behaviour sanitizers (a
stand-alone program, script on stdin, lines out); the Python split is held to the header's; five deliberately wrong rules are shown to differ
from the rule on the cases, so that a comparison of bits tests the order of the product, of the sum, and the precision of the logarithm; and
the numpy rule's own "log" scores lie within the stated bound of the exact sums (mpmath).  Comparisons are == on integers and on the bits of
doubles."""
import json
import os
import subprocess

import mpmath
import numpy as np
import pytest

import score_rule as sr
from isle_amd import hot_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("z", "score", "tokens", "unscored_entries", "unscored_tokens", "floored")


@pytest.fixture(scope="module")
def rules():
    """the numpy rule of every (case, mode), computed once and left unchanged"""
    return {(c.name, m): sr.rule(c, *m) for c in sr.CASES for m in sr.MODES}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("score_host") / "score_host_main")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "score_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    text = "".join(" ".join(str(x) for x in line) + "\n" for line in script)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["cmd"] for o in out] == [line[0] for line in script]
    return out


def lst(a):
    a = np.asarray(a).reshape(-1)
    return [a.size] + a.tolist()


def bits(a):
    return lst(np.ascontiguousarray(a, np.float32).view(np.uint32))


def dbits(x):
    return int(np.float64(x).view(np.uint64))


def arrays(a):
    """the six lists of a command: the weight rows, then the entries"""
    return lst(a["woff"]) + lst(a["wtopic"]) + bits(a["wweight"]) + lst(a["off"]) + lst(a["word"]) + bits(a["cnt"])


def case_arrays(c):
    return dict(woff=c.woff, wtopic=c.wtopic, wweight=c.wweight, off=c.off, word=c.word, cnt=c.cnt)


def test_the_table_holds_the_shapes_it_is_there_for(rules):
    docs = {int(n) for c in sr.CASES for n in np.diff(c.off)}
    rows = {int(n) for c in sr.CASES for n in np.diff(c.woff)}
    assert {0, 1, 63, 64, 65, 129, 4097} <= docs and {0, 1, 2, 255, 256, 257, 1024, 200} <= rows
    assert {c.k for c in sr.CASES} >= {1, 3, 4, 5, 200, 1024} and {c.V for c in sr.CASES} >= {1, 65, 5000}
    assert all(c.off[-1] == c.off[-2] for c in (sr.BY_NAME["v1_k1"], sr.BY_NAME["v5000_k1024_tiles"]))  # the last document empty
    absent = sr.BY_NAME["absent_words"]
    assert rules[absent.name, (sr.PROB, 0, 0.0)]["unscored_entries"].sum() > 0 and rules[absent.name, (sr.PROB, 0, 0.0)]["floored"].sum() == 0
    assert rules[absent.name, (sr.PROB, 0, sr.FLOOR)]["unscored_entries"].sum() == 0 and rules[absent.name, (sr.PROB, 0, sr.FLOOR)]["floored"].sum() > 0
    nan = rules["nan_column", (sr.LOG, 0, 0.0)]
    # rows 0 and 2 store the NaN topic and are wholly unscored; rows 1 and 3 do not, and the NaN column does not reach them
    assert nan["unscored_entries"][0] == 65 and nan["unscored_entries"][2] == 7 and nan["unscored_entries"][1] < 32 and nan["unscored_entries"][3] < 64
    assert np.isfinite(nan["score"].view(np.float64)).all() and (nan["score"].view(np.float64)[[1, 3]] < 0).all()
    zero = sr.BY_NAME["zero_rows"]
    assert rules[zero.name, (sr.PROB, 1, 0.0)]["unscored_entries"].tolist()[1:3] == [3, 64]  # rows of zero weights: no weights under normalise
    assert rules[zero.name, (sr.LOG, 1, sr.FLOOR)]["floored"].tolist()[1:3] == [3, 64]


def test_the_exact_fma_of_the_rule_is_the_c_library_s(exe):
    """score_rule.fma (integers, one correctly rounded division) against std::fma through the header's score_step: one weight row of one
    topic under normalise is a single step from 0.0, two topics chain a second one onto a rounded first"""
    rs = np.random.RandomState(11)
    V, n = 300, 300
    m = (rs.random_sample((V, 2)) * 3).astype(np.float32)
    c = sr.Case("fma", m, (np.array([0, 2]), np.array([0, 1]), np.array([0.3, 0.9], np.float32)),
                (np.ones(n, np.float32), np.arange(n), np.array([0, n])))
    got = run(exe, [["score", 2, V, sr.PROB, 1, dbits(0.0)] + bits(c.model.reshape(-1, order="F")) + arrays(case_arrays(c))])[0]
    want = sr.rule(c, sr.PROB, 1, 0.0)
    assert got["z"] == want["z"].tolist()
    unfused = sr.products(c, 1, "descending")  # (a different order: only to show that the values are not trivially equal)
    assert not np.array_equal(sr.d2b(unfused), want["z"])


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: c.name)
def test_the_header_is_the_numpy_rule_bit_for_bit(case, rules, exe):
    script = [["score", case.k, case.V, m[0], m[1], dbits(m[2])] + bits(case.model.reshape(-1, order="F")) + arrays(case_arrays(case)) for m in sr.MODES]
    for m, got in zip(sr.MODES, run(exe, script)):
        want = rules[case.name, m]
        for key in KEYS:
            if key == "score" and m[0] == sr.LOG:
                continue  # (the C library's log is not numpy's to the bit; test_the_log_scores_lie_within_the_bound holds both to the exact sum)
            assert got[key] == want[key].tolist(), (case.name, m, key)


def test_the_refusals_and_the_first_offenders_carry_their_texts(exe):
    probe = sr.BY_NAME["v65_k3"]
    script, want = [], []
    for name, a, kw, text in sr.REFUSALS:
        if "offsets" in name:
            which = "w_offsets" if name.startswith("w_") else "offsets"
            script.append(["offsets", which] + lst(a["woff"] if which == "w_offsets" else a["off"]))
        else:
            script.append(["args", 2, 1, kw.get("measure", 0), kw.get("normalise", 0), dbits(kw.get("floor", 0.0)), probe.k])
        want.append(text)
    for ncols in (0, 1025):
        script.append(["args", 2, 1, 0, 0, dbits(0.0), ncols])
        want.append("score_docs: ncols = %d not in [1, 1024]" % ncols)
    script += [["args", 1, 1, 0, 0, dbits(0.0), 3], ["args", 0, 2, 0, 0, dbits(0.0), 3], ["args", 0, 0, 1, 1, dbits(sr.FLOOR), 1024]]
    want += ["score_docs: unknown weights source 1 (ISLE_TOPDOCS_INFER or ISLE_TOPDOCS_HOST)", "score_docs: unknown entries source 2", ""]
    for name, a, text in sr.FAULTS:
        script.append(["faults", probe.k, probe.V] + arrays(a))
        want.append(text)
    script.append(["faults", probe.k, probe.V] + arrays(case_arrays(probe)))
    want.append("")
    got = run(exe, script)
    assert [g["text"] for g in got] == want


def test_split_held_out_is_the_header_s_and_a_partition(exe):
    rs = np.random.RandomState(3)
    D, V = 300, 5000
    lengths = rs.randint(0, 40, D)
    lengths[-1] = 0
    cnt, word, off = sr._entries(rs, V, lengths.tolist())
    assert cnt.size > 4000
    doc = np.repeat(np.arange(D), np.diff(off))
    for seed, num, den, base in ((0, 1, 2, 0), (12345678901234567890, 1, 5, 0), (7, 3, 4, 1 << 31), (7, 0, 3, 5), (7, 3, 3, 5)):
        held = run(exe, [["held", seed, num, den, base] + lst(doc) + lst(word)])[0]["held"]
        mask = hot_path.held_out_mask(doc, word, seed, num, den, base)
        assert mask.tolist() == [bool(h) for h in held]
        (oc, ow, oo), (hc, hw, ho) = hot_path.split_held_out(cnt, word, off, seed, num, den, base)
        assert oo[-1] + ho[-1] == cnt.size and np.array_equal(np.diff(oo) + np.diff(ho), np.diff(off))
        assert np.array_equal(hw, word[mask]) and np.array_equal(hc, cnt[mask]) and np.array_equal(ow, word[~mask]) and np.array_equal(oc, cnt[~mask])
        for d in (0, 17, D - 2):  # per document: observed and held are disjoint, together the input, in its order
            o, h = set(ow[oo[d]:oo[d + 1]].tolist()), set(hw[ho[d]:ho[d + 1]].tolist())
            assert not (o & h) and sorted(o | h) == word[off[d]:off[d + 1]].tolist()
        if num == 0:
            assert ho[-1] == 0
        if num == den:
            assert oo[-1] == 0
    assert 0.4 < hot_path.held_out_mask(doc, word, 0, 1, 2).mean() < 0.6
    a = hot_path.held_out_mask(doc[off[100]:], word[off[100]:], 5, 1, 2, 0)       # documents 100 .. as a part of the corpus ...
    b = hot_path.held_out_mask(doc[off[100]:] - 100, word[off[100]:], 5, 1, 2, 100)  # ... and as a shard of its own: the same split
    assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="held-out share"):
        hot_path.split_held_out(cnt, word, off, 0, 3, 2)


def test_score_total_is_the_ascending_sequential_sum(exe):
    v = (np.random.RandomState(4).random_sample(1000) - 0.3) * 10.0 ** np.random.RandomState(5).randint(-8, 8, 1000)
    want = sr.fold(v, sequential=True)
    assert run(exe, [["total"] + lst(sr.d2b(v))])[0]["total"] == [int(sr.d2b(want)[0])]
    assert sr.d2b(want)[0] != sr.d2b(sr.fold(v[::-1], sequential=True))[0]  # (the order shows on these values)
    assert run(exe, [["total", 0]])[0]["total"] == [0]


@pytest.mark.parametrize("wrong", sr.WRONG)
def test_a_wrong_rule_differs_from_the_rule_on_the_cases(wrong, rules):
    """1 z accumulated in fp32; 2 topics descending; 3 a plain sequential document sum; 4 log of z rounded to fp32; 5 normalise ignored"""
    mode = {"z_fp32": (sr.PROB, 0, 0.0), "descending": (sr.PROB, 0, 0.0), "sequential": (sr.PROB, 0, 0.0), "log_fp32": (sr.LOG, 0, 0.0),
            "no_normalise": (sr.PROB, 1, 0.0)}[wrong]
    key = "score" if wrong in ("sequential", "log_fp32") else "z"
    differ = [c.name for c in sr.CASES if not np.array_equal(sr.rule(c, *mode, wrong=wrong)[key], rules[c.name, mode][key])]
    assert len(differ) >= 3, (wrong, differ)
    if wrong == "sequential":  # a document of at most 64 entries and one of two entries per lane at most: there the fold IS order-sensitive too
        c = sr.BY_NAME["v5000_k200_long"]
        assert sr.rule(c, *mode, wrong=wrong)["score"][0] != rules[c.name, mode]["score"][0]


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: c.name)
def test_the_log_scores_lie_within_the_bound(case, rules):
    """|score - exact| <= g / (1 - g) sum c |ln z|, g = (2 K + 1 + ceil(n / 64) + 6) 2^-53: the numpy rule itself, whose log is within 1 ulp"""
    worst = 0.0
    for m in sr.MODES:
        if m[0] != sr.LOG:
            continue
        got = rules[case.name, m]
        score = got["score"].view(np.float64)
        for r, (ex, ab, bound) in enumerate(sr.exact_log(case, got["z"].view(np.float64), m[2])):
            err = abs(mpmath.mpf(float(score[r])) - ex)
            assert err <= bound, (case.name, m, r, float(err), float(bound))
            if ab:
                worst = max(worst, float(err / bound))
            else:
                assert got["score"][r] == 0  # no scored entry: +0.0, the bits
    assert worst < 0.5
