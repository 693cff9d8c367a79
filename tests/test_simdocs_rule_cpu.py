"""The rule of isle_hip_similar_docs without the library and without a GPU.  tests/simdocs_rule.py states it in numpy; here its elementwise form
is held to its scalar form, its DOT to sums of fractions.Fraction rounded once (where a case says every partial sum is exact), its candidate
and tie rules to a brute-force sort of Python tuples, and isle_amd/csrc/simdocs_host.h — the host statement, the argument checks with
their texts — and route_host.h's route_simdocs_table are held to all of that through isle_amd/host/simdocs_host_main.cpp, built here with the
address and undefined-behaviour sanitizers (a stand-alone program, script on stdin, lines out).  A W-rank simulation merges the rule on cut
rows and finds the uncut rule.  Every comparison is == on integers: documents, score bits, counts."""
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import simdocs_rule as sr
from topdocs_rule import f2b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
ALL = [(c, m) for c in sr.CASES for m in sr.MEASURES.values()]
SMALL = [c for c in sr.CASES if c.rows * c.Q <= 5000]


def same(got, want, what):
    for key in ("docs", "scores", "counts", "candidates"):
        assert np.array_equal(got[key], want[key]), (what, key)


@pytest.fixture(scope="module")
def rules():
    """the numpy rule of every (case, measure), computed once and left unchanged"""
    return {(c.name, m): sr.rule(c, m) for c, m in ALL}


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_the_elementwise_rule_is_the_scalar_rule(case, rules):
    for m in sr.MEASURES.values():
        same(rules[case.name, m], sr.rule_scalar(case, m), (case.name, m))


def lists_of(case):
    rows = [list(zip(case.topic[case.off[r]:case.off[r + 1]].tolist(), case.weight[case.off[r]:case.off[r + 1]].tolist())) for r in range(case.rows)]
    qs = [list(zip(case.q_topic[case.q_off[q]:case.q_off[q + 1]].tolist(), case.q_weight[case.q_off[q]:case.q_off[q + 1]].tolist())) for q in range(case.Q)]
    return rows, qs


def ord_py(b):
    return b ^ (M32 if b >> 31 else 0x80000000)


@pytest.mark.parametrize("case", [c for c in SMALL if c.exact], ids=lambda c: c.name)
def test_dot_is_the_exact_sum_rounded_once_and_the_lists_are_a_brute_force_sort(case, rules):
    """candidates by structure (a common STORED topic, not the excluded document), DOT by fractions, the order by Python's tuple sort"""
    rows, qs = lists_of(case)
    got = rules[case.name, sr.DOT]
    ex = case.exclude
    for q, query in enumerate(qs):
        qd = dict(query)
        cand = []
        for r, row in enumerate(rows):
            doc = case.doc_base + r
            common = [t for t, _ in row if t in qd]
            if not common or (int(ex[q]) != M32 and int(ex[q]) == doc):
                continue
            exact = sum((Fraction(a) * Fraction(qd[t]) for t, a in row if t in qd), Fraction(0))
            score = np.float32(float(exact))  # float(Fraction) rounds once to double (exactly, here), the cast once to fp32
            assert Fraction(float(score)) == exact, (case.name, q, r, "the case says every sum is exact")
            bits = int(f2b([score])[0]) if score != 0 else 0  # (an exact sum of zero is +0.0: -0.0 counts as 0)
            cand.append((-ord_py(bits), doc, bits))
        cand.sort()
        m = min(case.n, len(cand))
        assert int(got["counts"][q]) == m and int(got["candidates"][q]) == len(cand), (case.name, q)
        assert got["docs"][q, :m].tolist() == [x[1] for x in cand[:m]], (case.name, q)
        assert got["scores"][q, :m].tolist() == [x[2] for x in cand[:m]], (case.name, q)
        assert (got["docs"][q, m:] == M32).all() and (got["scores"][q, m:] == 0).all()


def test_the_cases_hit_what_they_aim_at(rules):
    by_aim = {}
    for c in sr.CASES:
        by_aim.setdefault(c.aim, []).append(c)
    assert {c.Q for c in by_aim["lanes"]} == {1, 2, 3, 5, 33, 64}
    for c in by_aim["lanes"]:
        G = 64 // sr.qp_of(c.Q)
        assert c.rows in (1, G - 1, G, G + 1)
    assert {int(x) for c in by_aim["lengths"] for x in np.diff(c.off)} >= {0, 1, 63, 64, 65, 200}
    assert any(c.num_topics * sr.qp_of(c.Q) * 4 == 65536 and "auto" in c.forms for c in by_aim["lengths"])
    assert any(c.num_topics * sr.qp_of(c.Q) * 4 == 65536 + 4 * sr.qp_of(c.Q) and "auto" in c.forms for c in by_aim["lengths"])
    assert all(c.num_topics == 1024 and c.Q == 64 for c in by_aim["global"])
    assert any(c.rows == 4000 for c in by_aim["many_rows"]) and by_aim["n256"][0].n == 256
    z = rules["zero_weights", sr.DOT]
    assert int(z["candidates"][3]) == 0 and int(z["candidates"][4]) == 0            # a topic nobody stores; a query without entries
    assert z["docs"][0, :int(z["counts"][0])].tolist() == [12, 10, 15, 17]               # scores 6, then +0 three times: documents ascending
    assert z["scores"][0, 1:4].tolist() == [0, 0, 0] and 11 not in z["docs"][0].tolist()  # a row sharing nothing is no candidate
    f = rules["fewer_than_n", sr.DOT]
    assert (f["counts"] < 20).all() and (f["counts"] > 0).all()
    assert (rules["no_match", sr.COSINE]["counts"] == 0).all()
    for c in by_aim["tie"]:
        r = rules[c.name, sr.COSINE]
        m = int(r["counts"][0])
        assert len(set(r["scores"][0, :m].tolist())) < m and np.array_equal(r["docs"][0], r["docs"][2]) and np.array_equal(r["scores"][0], r["scores"][2])
        run = r["scores"][0, :m] == r["scores"][0, 0]
        assert (np.diff(r["docs"][0, :m][run].astype(np.int64)) > 0).all()
    assert BYN("ties_n5").doc_base + BYN("ties_n5").rows - 1 == 0xFFFFFFF0 and 0xFFFFFFF0 - BYN("ties_n5").doc_base < 703
    e = BYN("exclude_hits_and_misses")
    free = sr.rule(sr.Case("free", e.num_topics, e.n, e.doc_base, e.source_arg(), (e.q_off, e.q_topic, e.q_weight)), sr.DOT)
    got = rules[e.name, sr.DOT]
    assert (free["candidates"] - got["candidates"]).tolist() == [1, 0, 0, 1]
    d = rules["query_rows_default", sr.COSINE]
    c = BYN("query_rows_default")
    for q, r in enumerate(c.query_rows.tolist()):
        assert c.doc_base + r not in d["docs"][q].tolist()
    assert np.array_equal(d["docs"][0], d["docs"][3])
    assert sorted(int(c.off[-1]) for c in by_aim["tile"]) == [2046, 2048, 2050, 4096, 6144]
    assert [int(rules[c.name, sr.DOT]["candidates"][0]) for c in by_aim["tile"]] == [1023, 1024, 1025, 2048, 3072]
    zn = rules["zero_norm", sr.COSINE]
    assert zn["docs"][0, :4].tolist() == [1, 0, 2, 3] and zn["scores"][0, 1:4].tolist() == [0, 0, 0]  # rows of zeros: den == 0 gives +0.0
    assert int(zn["scores"][0, 0]) == int(f2b([np.float32(1) / (np.float32(1) * np.sqrt(np.float32(2)))])[0])
    w = np.concatenate([c.weight for c in sr.CASES] + [c.q_weight for c in sr.CASES])
    assert ((w == 0) | (w >= 2.0 ** -60)).all() and np.isfinite(w).all()


def BYN(name):
    return sr.BY_NAME[name]


@pytest.mark.parametrize("name", sr.SHARDED)
@pytest.mark.parametrize("world", (2, 3))
def test_the_rule_on_cut_rows_merged_is_the_uncut_rule(name, world, rules):
    case = BYN(name)
    for m in sr.MEASURES.values():
        same(sr.merged(case, m, sr.cuts(case, world)), rules[case.name, m], (name, world, m))
    if world == 3 and case.aim == "tie":
        b = sr.cuts(case, 3)
        assert b[1] == b[2] == 3 and int(case.off[3]) == 0  # a share of rows without entries, a share without rows


# ---- the header, through its stand-alone main --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("simdocs_host") / "simdocs_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "simdocs_host_main.cpp")], capture_output=True, text=True, timeout=300)
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


def test_the_host_statement_is_the_numpy_rule_bit_for_bit(exe, rules):
    script = []
    for c, m in ALL:
        ex = c.exclude
        script.append(["select", m, c.n, c.doc_base] + lst(c.off) + lst(c.topic) + bits(c.weight) + lst(c.q_off) + lst(c.q_topic) + bits(c.q_weight)
                      + (lst(ex) if (ex != M32).any() else [0]))
    for (c, m), o in zip(ALL, run(exe, script)):
        want = rules[c.name, m]
        for key in ("docs", "scores", "counts", "candidates"):
            assert o[key] == want[key].reshape(-1).tolist(), (c.name, m, key)


def test_the_checks_and_their_texts(exe):
    pats = [0x00000000, 0x80000000, 0x00000001, 0x3F800000, 0x4EFFFFFF, 0x4F000000, 0x7F800000, 0x7FC00000, 0xFFC00000, 0xBF800000, 0x80000001]
    good = ["args", 2, 1, 3, 5, 2, 1, 0, 1200]
    q_ok = lst([0, 1, 3]) + lst([0, 1, 2]) + bits([1, 2, 1])
    script = [["ok"] + lst(pats), ["qp", 1], ["qp", 3], ["qp", 33], ["qp", 64], good,
              ["args", 7, 1, 3, 5, 2, 1, 0, 1200], ["args", 2, 3, 3, 5, 2, 1, 0, 1200], ["args", 2, 1, 0, 5, 2, 1, 0, 1200],
              ["args", 2, 1, 3, 5, 0, 1, 0, 1200], ["args", 2, 1, 3, 5, 65, 1, 0, 1200], ["args", 2, 1, 3, 0, 2, 1, 0, 1200],
              ["args", 2, 1, 3, 257, 2, 1, 0, 1200], ["args", 2, 1, 3, 256, 2, 33, 0, 1200], ["args", 2, 1, 3, 5, 2, 1, 0xFFFFFFF1 - 1199, 1200],
              ["args", 2, 1, 3, 5, 2, 1, 0xFFFFFFF1 - 1200, 1200],
              ["form", 0], ["form", 2], ["form", 3], ["form", -1],
              ["qrows", 1200] + lst([5, 1199]), ["qrows", 1200] + lst([5, 1200, 4000]),
              ["queries", 3] + q_ok,
              ["queries", 3] + lst([1, 1, 3]) + lst([0, 1, 2]) + bits([1, 2, 1]),
              ["queries", 3] + lst([0, 2, 1, 3]) + lst([0, 1, 2]) + bits([1, 2, 1]),
              ["queries", 3] + lst([0, 1, 3]) + lst([0, 1, 3]) + bits([1, -2, 1]),      # topic range before the weight
              ["queries", 3] + lst([0, 1, 3]) + lst([0, 2, 1]) + bits([-1, 2, 1]),      # order before the weight
              ["queries", 3] + lst([0, 1, 3]) + lst([0, 1, 2]) + bits([1, 2, float("inf")]),
              ["queries", 3] + lst([0, 0, 0]) + [0] + [0]]
    out = run(exe, script)
    assert out[0]["ok"] == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]  # +0, -0, a denormal, 1, the largest below 2^31; 2^31, inf, NaNs, -1, a negative denormal
    assert [o["qp"] for o in out[1:5]] == [1, 4, 64, 64]
    texts = [o["text"] for o in out[5:]]
    assert texts[0] == "" and texts[10] == ""
    for got, piece in zip(texts[1:10], ["unknown source 7", "unknown measure 3", "num_topics = 0 < 1", "num_queries = 0 not in [1, 64]",
                                        "num_queries = 65 not in [1, 64]", "n = 0 not in [1, 256]", "n = 257 not in [1, 256]",
                                        "33 ranks x n = 256 are more than 8192 keys per query", "+ 1200 rows exceed 4294967281"]):
        assert got.startswith("similar_docs: ") and piece in got, (got, piece)
    assert texts[11:15] == ["", "", "simdocs_table_form: unknown form 3", "simdocs_table_form: unknown form -1"]
    assert texts[15] == "" and texts[16] == "similar_docs: query_rows[1] = 1200 is not below the 1200 rows"
    assert texts[17] == ""
    assert texts[18] == "similar_docs: q_offsets[0] = 1, not 0" and texts[19] == "similar_docs: q_offsets descend at query 1"
    assert texts[20] == "similar_docs: query entry 2 (query 1) has topic 3 >= num_topics 3"
    assert texts[21] == "similar_docs: query entry 2 (query 1), topic 1: the topics of a query must ascend strictly"
    assert texts[22] == "similar_docs: entry 2 (query 1) has weight inf: a weight is finite, >= 0 and < 2^31"
    assert texts[23] == ""
    # the refusals of the table that the host decides: the text the GPU test expects is the header's
    script = []
    for r in sr.REFUSALS:
        q = r.kw.get("queries")
        if isinstance(q, tuple) and 1 <= q[0].size - 1 <= 64:
            script.append(["queries", 3] + lst(q[0]) + lst(q[1]) + bits(q[2]))
            assert r.text in run(exe, script[-1:])[0]["text"], r.name


def test_the_table_lives_in_lds_up_to_64_kib(exe):
    script = []
    want = []
    for Q in (1, 2, 3, 5, 33, 64):
        qp = sr.qp_of(Q)
        at = 65536 // (4 * qp)  # num_topics at the budget: num_topics Qp 4 = 65536
        script += [["table", Q, at, 0], ["table", Q, at + 1, 0], ["table", Q, at, 1], ["table", Q, at + 1, 1], ["table", Q, at, 2], ["table", Q, 1, 2]]
        want += [0, 1, 0, 1, 1, 1]
    script += [["table", 64, 256, 0], ["table", 64, 257, 0], ["table", 64, 1024, 0], ["table", 64, 1024, 1], ["table", 64, 200, 0]]
    want += [0, 1, 1, 1, 0]
    assert [o["home"] for o in run(exe, script)] == want
