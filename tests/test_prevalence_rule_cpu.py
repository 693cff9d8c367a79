"""The rule of isle_hip_topic_prevalence without the library and without a GPU.  tests/prevalence_rule.py states it in numpy; here its
elementwise form is held to its scalar form, its sums to sums of fractions.Fraction within the bound the header states, the normalised sums
to the number of rows that have weight, the dominant counts to the rows that have entries, and the cases marked `order` are shown to differ
from a plain ascending sequential sum, so that a comparison of bits tests the order of summation.  isle_amd/csrc/prevalence_host.h (the host
statement, the argument checks with their texts, prev_tile) is held to all of that through isle_amd/host/prevalence_host_main.cpp, built here
with the address and undefined-behaviour sanitizers (a stand-alone program, script on stdin, lines out).  Comparisons are == on integers and
on the bits of doubles."""
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import prevalence_rule as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = Fraction(1, 2 ** 53)
ALL = [(c, n) for c in pr.CASES for n in (0, 1)]


def gamma(m):
    return m * U / (1 - m * U)


def same(got, want, what):
    for key in pr.FIELDS:
        assert got[key].dtype == np.uint64 and np.array_equal(got[key], want[key]), (what, key)


@pytest.fixture(scope="module")
def rules():
    """the numpy rule of every (case, normalise), computed once and left unchanged"""
    return {(c.name, n): pr.rule(c, n) for c, n in ALL}


@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c.name)
def test_the_elementwise_rule_is_the_scalar_rule(case, rules):
    for n in (0, 1):
        same(rules[case.name, n], pr.rule_scalar(case, n), (case.name, n))


def members(c):
    lab = c.labels()
    return {g: np.nonzero(lab == g)[0].tolist() for g in range(c.num_groups) if (lab == g).any()}


@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c.name)
def test_the_sums_lie_within_the_stated_bound_of_the_exact_sums(case, rules):
    """without normalise: |sum - exact| <= exact c u / (1 - c u), c = count[g,t], u = 2^-53 (Higham's bound for any order)"""
    got = rules[case.name, 0]
    total = got["sum"].view(np.float64)
    exact = {}
    lab = case.labels().tolist()
    for r in range(case.rows):
        if lab[r] == pr.NONE:
            continue
        for e in range(int(case.off[r]), int(case.off[r + 1])):
            key = (lab[r], int(case.topic[e]))
            exact[key] = exact.get(key, Fraction(0)) + Fraction(float(case.weight[e]))
    for g in range(case.num_groups):
        for t in range(case.num_topics):
            ex = exact.get((g, t), Fraction(0))
            assert abs(Fraction(float(total[g, t])) - ex) <= ex * gamma(int(got["count"][g, t])), (case.name, g, t)
            if (g, t) not in exact:
                assert int(got["sum"][g, t]) == 0  # +0.0, the bits


@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c.name)
def test_the_normalised_sums_of_a_group_add_up_to_its_rows_that_have_weight(case, rules):
    """sum_t sum[g,t] against the rows of g with rs > 0.  A term is w / rs rounded once with rs the rounded sum of len - 1 additions: by
    Higham's Lemma 3.3 a relative error theta_{1 + 2 (len - 1)}; the tree adds theta_c: the bound is n gamma(c_max + 2 len_max), the sum
    over t taken exactly."""
    got = rules[case.name, 1]
    total = got["sum"].view(np.float64)
    rs = pr.row_sums(case)
    length = np.diff(case.off)
    for g, rows in members(case).items():
        n_pos = int((rs[rows] > 0).sum())
        s = sum((Fraction(float(x)) for x in total[g]), Fraction(0))
        m = int(got["count"][g].max()) + 2 * int(length[rows].max())
        assert abs(s - n_pos) <= n_pos * gamma(m), (case.name, g)
    for g in range(case.num_groups):
        assert int(got["docs"][g]) == len(members(case).get(g, []))


def test_the_cases_marked_order_differ_from_a_sequential_sum(rules):
    """so that == on the bits of sum tests the radix-64 order; and the tree of at most 65 values IS the sequential sum"""
    marked = [c for c in pr.CASES if c.order]
    assert {c.name for c in marked} >= {"one_group_130", "one_group_4096", "one_group_4097", "k65", "k200", "k1024", "k1025", "k4100_one_group"}
    for c in marked:
        seq = pr.rule_scalar(c, 0, sequential=True)
        assert not np.array_equal(seq["sum"], rules[c.name, 0]["sum"]), c.name
        for key in ("docs", "count", "dominant"):
            assert np.array_equal(seq[key], rules[c.name, 0][key])
    for name in ("one_group_63", "one_group_64", "one_group_65", "rows1"):
        assert np.array_equal(pr.rule_scalar(pr.BY_NAME[name], 0, sequential=True)["sum"], rules[name, 0]["sum"]), name


@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c.name)
def test_the_dominant_counts_of_a_group_are_its_rows_that_have_entries(case, rules):
    length = np.diff(case.off)
    for n in (0, 1):
        got = rules[case.name, n]
        assert got["dominant"].sum(axis=1).tolist() == [int((length[members(case).get(g, [])] > 0).sum()) for g in range(case.num_groups)]
        assert (got["dominant"] <= got["count"]).all() and (got["count"] <= got["docs"][:, None]).all()
        assert int(got["docs"].sum()) + int(got["unlabelled"][0]) == case.rows


def test_the_cases_hit_what_they_aim_at(rules):
    sizes = {c.rows for c in pr.CASES if c.groups is None}
    assert sizes >= {0, 1, 63, 64, 65, 4096, 4097}
    t = pr.BY_NAME["three_groups_0_64_65"]
    r = rules[t.name, 0]
    assert r["docs"].tolist() == [0, 64, 65] and int(r["unlabelled"][0]) > 0 and (np.diff(t.groups.astype(np.int64)) != 0).sum() > 60
    g = pr.BY_NAME["g1000_on_700_rows"]
    assert g.num_groups == 1000 and g.rows == 700 and int((rules[g.name, 0]["docs"] == 0).sum()) > 400
    assert {c.num_topics for c in pr.CASES} >= {1, 64, 65, 200, 1024, 1025}
    for k in (64, 65, 200, 1024, 1025):
        c = pr.BY_NAME["k%d" % k]
        assert int(c.topic.max()) == k - 1                                   # the last topic is stored
        assert k <= 65 or int(np.diff(c.off).max()) > 64                      # rows longer than a wave
    s = pr.BY_NAME["special_rows"]
    length = np.diff(s.off)
    assert (length == 0).any() and (s.weight.view(np.uint32) == 0x80000000).any()
    sp, sn = rules[s.name, 0], rules[s.name, 1]
    assert sp["dominant"].tolist() == [[0, 1, 0, 2], [1, 1, 1, 0]]          # row 3: topics 1 and 3 tie, the smaller wins; rows 1, 7: -0.0 = +0.0
    assert sn["sum"][0, 0] == pr.d2b([2.0 ** -40 / (2.0 ** -40 + 2.0 ** 20)])[0]
    assert sn["sum"][1, 0] == pr.d2b([1.5 / 7.5])[0]                        # row 1 is all zeros: its terms are +0.0, not NaN
    assert (sp["sum"] >> 63 == 0).all() and (sn["sum"] >> 63 == 0).all()    # no -0.0 anywhere
    lds = [c for c in pr.CASES if c.num_groups * (2 * c.num_topics + 1) * 4 <= 32768]
    assert len(lds) >= 8 and len(lds) <= len(pr.CASES) - 2                  # both homes of the row pass's counters
    w = np.concatenate([c.weight for c in pr.CASES])
    assert np.isfinite(w).all() and (w >= 0).all() and float(w[w > 0].min()) < 2.0 ** -39 and float(w.max()) >= 2.0 ** 19


# ---- the header, through its stand-alone main --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("prevalence_host") / "prevalence_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "prevalence_host_main.cpp")], capture_output=True, text=True, timeout=300)
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


def rows_of(c):
    return lst(c.off) + lst(c.topic) + bits(c.weight) + (lst(c.groups) if c.groups is not None else [0])


def test_the_host_statement_is_the_numpy_rule_bit_for_bit(exe, rules):
    script = [["prev", c.num_topics, c.num_groups, n] + rows_of(c) for c, n in ALL]
    for (c, n), o in zip(ALL, run(exe, script)):
        want = rules[c.name, n]
        assert o["unlabelled"] == int(want["unlabelled"][0]), c.name
        for key in ("docs", "count", "dominant", "sum"):
            assert o[key] == want[key].reshape(-1).tolist(), (c.name, n, key)


def test_the_checks_the_texts_and_the_tile(exe):
    pats = [0x00000000, 0x80000000, 0x00000001, 0x3F800000, 0x4EFFFFFF, 0x4F000000, 0x7F800000, 0x7FC00000, 0xFFC00000, 0xBF800000, 0x80000001]
    script = [["ok"] + lst(pats),
              ["tile", 1, 0], ["tile", 200, 0], ["tile", 1024, 0], ["tile", 1025, 0], ["tile", 8192, 1], ["tile", 200, 2], ["tile", 64, 2], ["tile", 63, 2],
              ["levels", 0], ["levels", 1], ["levels", 64], ["levels", 65], ["levels", 4096], ["levels", 4097], ["levels", 262144], ["levels", 262145],
              ["levels", 0xFFFFFFFF],
              ["lds", 1, 200], ["lds", 3, 7], ["lds", 2, 2047], ["lds", 2, 2048], ["lds", 1000, 4], ["lds", 8192, 0],
              ["args", 2, 200, 50, 1, 1, 1, 1000], ["args", 0, 1, 1, 0, 0, 1, 0], ["args", 1, 8192, 2048, 0, 1, 1, 5],
              ["args", 7, 200, 50, 1, 1, 1, 1000], ["args", 2, 200, 50, 2, 1, 1, 1000], ["args", 2, 200, 50, -1, 1, 1, 1000],
              ["args", 2, 0, 50, 1, 1, 1, 1000], ["args", 2, 8193, 1, 1, 1, 1, 1000], ["args", 2, 200, 0, 1, 1, 1, 1000],
              ["args", 2, 8192, 2049, 0, 1, 1, 5], ["args", 2, 200, 2, 0, 0, 1, 1000], ["args", 2, 200, 1, 0, 0, 2, 1000],
              ["args", 2, 200, 1, 0, 0, 1, 2 ** 32],
              ["form", 0], ["form", 1], ["form", 2], ["form", 3], ["form", -1]]
    out = run(exe, script)
    assert out[0]["ok"] == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]  # +0, -0, a denormal, 1, the largest below 2^31; 2^31, inf, NaNs, -1, a negative denormal
    assert [o["tile"] for o in out[1:9]] == [1, 200, 1024, 1024, 1024, 64, 64, 63]
    assert [o["levels"] for o in out[9:18]] == [0, 1, 1, 2, 2, 3, 3, 4, 6]
    assert [o["lds"] for o in out[18:24]] == [1, 1, 1, 0, 0, 1]
    texts = [o["text"] for o in out[24:]]
    assert texts[:3] == ["", "", ""]
    for got, piece in zip(texts[3:13], ["unknown source 7", "normalise = 2, not 0 or 1", "normalise = -1, not 0 or 1", "num_topics = 0 not in [1, 8192]",
                                        "num_topics = 8193 not in [1, 8192]", "num_groups = 0 < 1", "2049 groups x 8192 topics are more than 16777216 cells",
                                        "null groups with num_groups = 2", "2 ranks: a bit-equal sum across ranks", "4294967296 rows, 2^32 or more"]):
        assert got.startswith("topic_prevalence: ") and piece in got, (got, piece)
    assert texts[13:] == ["", "", "", "prevalence_tile_form: unknown form 3", "prevalence_tile_form: unknown form -1"]


def test_the_first_offender_is_named_as_the_rule_names_it(exe):
    script = [["faults", c.num_topics, c.num_groups] + rows_of(c) for c in pr.REFUSALS + [pr.BY_NAME["special_rows"], pr.BY_NAME["three_groups_0_64_65"]]]
    texts = [o["text"] for o in run(exe, script)]
    assert texts[-2:] == ["", ""]
    for c, got in zip(pr.REFUSALS, texts):
        assert got == pr.first_fault_text(c) and got, (c.name, got)
    by = dict(zip([c.name for c in pr.REFUSALS], texts))
    assert by["bad_label"] == "topic_prevalence: row 17 has label 3 >= num_groups 3 (0xffffffff: no group)"
    assert by["label_none_is_no_fault_but_7_is"].startswith("topic_prevalence: row 299 has label 7")
    assert re.fullmatch(r"topic_prevalence: entry \d+ \(row \d+\) has weight -1: a weight is finite, >= 0 and < 2\^31", by["negative_weight_first_of_two"])
    assert "has weight nan" in by["nan_weight"] and "has weight 2.14748e+09" in by["weight_2_pow_31"]
    assert "has topic 6 >= num_topics 6" in by["topic_out_of_range"] and "the topics of a row must ascend strictly" in by["topics_do_not_ascend"]
    assert by["label_before_entry"].startswith("topic_prevalence: row 280 has label 4")


def test_the_header_carries_the_defines_and_the_rule_is_plain_cpp():
    head = open(os.path.join(ROOT, "include", "isle_hip.h")).read()
    for line in ("#define ISLE_GROUP_NONE 0xffffffffu", "#define ISLE_PREVALENCE_MAX_CELLS (1u << 24)", "#define ISLE_PREVALENCE_TILE_AUTO 0",
                 "#define ISLE_PREVALENCE_TILE_WIDE 1", "#define ISLE_PREVALENCE_TILE_NARROW 2", "int isle_hip_prevalence_tile_form(isle_ctx* ctx, int form);"):
        assert line in head, line
    assert re.search(r"int isle_hip_topic_prevalence\(isle_ctx\* ctx, int source[^;]*uint64_t\* dominant,\s*double\* sum\);", head)
    host = open(os.path.join(ROOT, "isle_amd", "csrc", "prevalence_host.h")).read()
    assert "#include <hip" not in host and "isle_ctx*" not in host and "route_host.h" not in host  # plain C++, and the tile rule is its own
    assert "constexpr uint32_t PREV_FAN = 64;" in host and "prev_tile(uint32_t num_topics, int asked)" in host
    assert "c u / (1 - c u)" in host                                                                # the bound is stated
    route = open(os.path.join(ROOT, "isle_amd", "csrc", "route_host.h")).read()
    assert route.rstrip().endswith("inline NdKey route_neardup_key(int asked) { return asked == 2 ? ND_FORM_NARROW : ND_FORM_FULL; }")
    assert "prev_tile" not in route and "PREV_" not in route
    common = open(os.path.join(ROOT, "isle_amd", "csrc", "common.h")).read()
    assert re.search(r"int simdocs_table_form = 0;[^\n]*\n\s*int prevalence_tile_form = 0;", common)
