"""The rule of isle_hip_topic_top_docs without the library and without a GPU.  tests/topdocs_rule.py states it in numpy; here it is held to a
brute-force sort of Python tuples, every case of its table is shown to hit what it aims at, and isle_amd/csrc/topdocs_host.h — the host
statement and the emulation of the device's eight rounds over 1, 2 and 3 simulated ranks — is held to the rule through
isle_amd/host/topdocs_host_main.cpp, built here with the address and undefined-behaviour sanitizers (a stand-alone program, script on
stdin, lines out).  Every comparison is == on integers: documents, value bits, counts."""
import json
import os
import subprocess

import numpy as np
import pytest

import topdocs_rule as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def ord_py(b):
    return b ^ (M32 if b >> 31 else 0x80000000)


def brute(case):
    """per topic the (document, bits) pairs by (ord descending, document ascending), all of them"""
    per = [[] for _ in range(case.num_topics)]
    row = case.row_of_entry()
    for e in range(case.topic.size):
        per[int(case.topic[e])].append((-ord_py(int(case.bits[e])), case.doc_base + int(row[e]), int(case.bits[e])))
    return [sorted(p) for p in per]


@pytest.fixture(scope="module")
def brutes():
    return {c.name: brute(c) for c in tr.CASES}


@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c.name)
def test_the_numpy_rule_is_the_brute_force_sort(case, brutes):
    got = tr.rule(case)
    for t, p in enumerate(brutes[case.name]):
        m = min(case.n, len(p))
        assert int(got["counts"][t]) == m and int(got["topic_entries"][t]) == len(p)
        assert got["docs"][t, :m].tolist() == [x[1] for x in p[:m]]
        assert got["values"][t, :m].tolist() == [x[2] for x in p[:m]]
        assert (got["docs"][t, m:] == M32).all() and (got["values"][t, m:] == 0).all()


# ---- every case hits what it aims at ---------------------------------------------------------------------------------------------------------------
def aim_one(c, b):
    assert c.num_topics == 1 and c.topic.size == 1 and c.n in (1, 256)


def aim_no_rows(c, b):
    assert c.rows == 0


def aim_no_entries(c, b):
    assert c.rows == 5 and c.topic.size == 0


def aim_fewer(c, b):
    sizes = [len(p) for p in b]
    assert 0 in sizes and any(0 < s < c.n for s in sizes) and any(s > c.n for s in sizes)


def aim_bins(c, b):
    assert (c.num_topics * 256 * 4 <= 64 * 1024) == c.facts["lds"] and c.rows >= 3000
    longer = [p for p in b if len(p) > c.n]
    assert len(longer) == c.num_topics or c.n > 5
    assert c.n == 1 or not longer or any(p[c.n - 1][0] == p[c.n][0] for p in longer)  # bit-equal values meet across the n-th place


def aim_byte(c, b):
    k = c.facts["byte"]
    x = np.bitwise_xor.reduce(np.stack([c.bits, np.roll(c.bits, 1)]), axis=0)
    assert ((x & ~np.uint32(0xFF << (8 * k))) == 0).all() and len(set(c.bits.tolist())) == c.bits.size > c.n
    if k == 0:
        assert b[0][c.n - 1][2] - b[0][c.n][2] == 1  # one ulp apart across the n-th place
    v = c.values
    assert np.isfinite(v).all() and (v > 0).all()


def aim_tie(c, b):
    p = b[1]
    tied = [x for x in p if x[0] == p[min(c.n, len(p)) - 1][0]]
    assert len(tied) > 256 and len(tied) == 700  # the tie outlasts a whole low document byte
    docs = [x[1] for x in tied]
    for edge in c.facts["straddle"]:
        assert any(d // edge != docs[0] // edge for d in docs) and min(docs) % edge != 0
    if not c.facts["straddle"]:
        assert min(docs) >> 24 == 0xFF
    assert c.device == (c.n <= tr.MAX_N)


def aim_specials(c, b):
    have = set(c.bits.tolist())
    assert {0x80000000, 0, 0x7F800000, 0x7FC00000, 0x00000001, 0xBF800000} <= have
    v = [x[2] for x in b[1]]
    assert v.index(0x7FC00000) < v.index(0x7F800000) < v.index(0x3F800000) < v.index(0) < v.index(0x80000000) < v.index(0xBF800000) < v.index(0xFF800000)


def aim_tile(c, b):
    assert c.topic.size == c.facts["nnz"] and c.facts["nnz"] in (1023, 1024, 1025)


def aim_empty_run(c, b):
    lens = np.diff(c.off)
    filled = np.flatnonzero(lens)
    assert np.diff(filled).max() - 1 > tr.IT_WIN and c.topic.size < 1024  # within one tile


def aim_wide_row(c, b):
    assert np.diff(c.off).max() == 1500 == c.num_topics


AIMS = dict(one=aim_one, no_rows=aim_no_rows, no_entries=aim_no_entries, fewer=aim_fewer, bins=aim_bins, byte=aim_byte, tie=aim_tie, specials=aim_specials,
            tile=aim_tile, empty_run=aim_empty_run, wide_row=aim_wide_row)


@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c.name)
def test_every_case_hits_what_it_aims_at(case, brutes):
    AIMS[case.aim](case, brutes[case.name])


def test_the_table_covers_the_issue():
    aims = {c.aim for c in tr.CASES}
    assert aims == set(AIMS)
    assert {c.num_topics for c in tr.CASES if c.aim == "bins"} == {3, 64, 65, 257} and {c.n for c in tr.CASES if c.aim == "bins"} == {1, 5, 32, 256}
    assert {c.facts["byte"] for c in tr.CASES if c.aim == "byte"} == {0, 1, 2, 3}
    assert {c.n for c in tr.CASES if c.aim == "tie"} == {5, 256, 300}
    assert {r.name for r in tr.REFUSALS} == {"topic_is_num_topics", "repeated_topic", "descending_pair", "n_0", "n_257", "doc_base_too_large"}
    for name in tr.SHARDED:  # what the sharded test relies on
        assert tr.BY_NAME[name].device
    lead = [c for c in tr.CASES if c.aim in ("tie", "byte", "bins")]
    assert all(tr.cuts(c, 3)[1] == tr.cuts(c, 3)[2] >= 3 and c.off[tr.cuts(c, 3)[1]] == 0 for c in lead)  # a share with rows and no entries, one without rows
    for c in tr.CASES:
        if c.aim == "tie":  # the tied documents span the boundary of two shares
            assert 0 < tr.cuts(c, 2)[1] < c.rows and c.off[tr.cuts(c, 2)[1]] > 0


def test_the_cutter_keeps_every_entry():
    for c in tr.CASES:
        for W in (1, 2, 3):
            b = tr.cuts(c, W)
            parts = [tr.share(c, b, q) for q in range(W)]
            assert sum(p[1].size - 1 for p in parts) == c.rows
            assert np.array_equal(np.concatenate([p[2] for p in parts]), c.topic) and np.array_equal(np.concatenate([p[3] for p in parts]), c.bits)
            assert all(p[1][0] == 0 and p[1][-1] == p[2].size for p in parts)
            assert [p[0] for p in parts] == [c.doc_base + x for x in b[:-1]]


# ---- the header, through its stand-alone program ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("topdocs_host") / "topdocs_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "topdocs_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    text = "\n".join(" ".join(str(t) for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["cmd"] for o in out] == [line[0] for line in script]
    return out


def lst(a):
    a = np.asarray(a).reshape(-1)
    return [a.size] + a.tolist()


def triples(c):
    return [c.num_topics, c.n, c.doc_base] + lst(c.off) + lst(c.topic) + lst(c.bits)


@pytest.fixture(scope="module")
def answers(exe):
    """every case through the host statement and through the emulated rounds at W = 1, 2, 3: one run of the program"""
    script, keys = [], []
    for c in tr.CASES:
        script.append(["select"] + triples(c))
        keys.append((c.name, 0))
        for W in (1, 2, 3):
            script.append(["rounds"] + triples(c) + lst(tr.cuts(c, W)))
            keys.append((c.name, W))
    return dict(zip(keys, run(exe, script)))


@pytest.mark.parametrize("W", (0, 1, 2, 3), ids=lambda w: "statement" if w == 0 else "rounds_W%d" % w)
@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c.name)
def test_the_host_statement_and_the_emulated_rounds_equal_the_rule(case, W, answers):
    want, got = tr.rule(case), answers[(case.name, W)]
    assert got["counts"] == want["counts"].tolist() and got["entries"] == want["topic_entries"].tolist()
    assert got["docs"] == want["docs"].reshape(-1).tolist()
    assert got["values"] == want["values"].reshape(-1).tolist()


EDGE_BITS = [0, 1, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xBF800000, 0xFF7FFFFF,
             0xFF800000, 0xFFC00000, 0xFFFFFFFF]


def test_ord_and_the_key_round_trip_on_the_edge_patterns(exe):
    docs = [0, 1, 0xFF, 0x100, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000, 0xFFFFFFF0]
    script = [["ord"] + lst(EDGE_BITS)] + [["key", b, d] for b in EDGE_BITS for d in docs]
    out = run(exe, script)
    assert out[0]["ord"] == [ord_py(b) for b in EDGE_BITS] and out[0]["back"] == EDGE_BITS
    assert out[0]["ord"] == tr.ord_bits(EDGE_BITS).tolist()
    pairs = [(b, d) for b in EDGE_BITS for d in docs]
    for (b, d), o in zip(pairs, out[1:]):
        assert o["key"] == (ord_py(b) << 32 | (~d & M32)) and o["key"] != 0 and o["doc"] == d and o["bits"] == b
    # the order of ord is the numeric order where there is one (NaN patterns aside), -0.0 below +0.0
    finite = [b for b in EDGE_BITS if (b & 0x7F800000) != 0x7F800000 or (b & 0x007FFFFF) == 0]
    by_ord = sorted(finite, key=ord_py)
    as_float = np.array(by_ord, np.uint32).view(np.float32)
    assert (np.diff(as_float.astype(np.float64)) >= 0).all() and by_ord.index(0x80000000) + 1 == by_ord.index(0)


def test_the_argument_checks_and_the_bins_home(exe):
    script = [["args", 3, 4, 5, 1, 0, 10], ["args", 2, 0, 5, 1, 0, 10], ["args", 2, 4, 0, 1, 0, 10], ["args", 2, 4, 257, 1, 0, 10], ["args", 2, 4, 256, 33, 0, 10],
              ["args", 2, 4, 256, 32, 0, 10], ["args", 2, 4, 5, 1, 0xFFFFFFF1 - 10, 10], ["args", 2, 4, 5, 1, 0xFFFFFFF1 - 9, 10], ["args", 2, 4, 5, 1, 1 << 40, 0],
              ["lds", 1], ["lds", 64], ["lds", 65], ["fault", 3, 3, 1, 0], ["fault", 2, 3, 1, 0], ["fault", 2, 3, 0, 2], ["fault", 2, 3, 0, 3], ["fault", 2, 3, 0, 1]]
    out = run(exe, script)
    texts = [o["text"] for o in out[:9]]
    assert "unknown source 3" in texts[0] and "num_topics = 0 < 1" in texts[1] and "n = 0 not in [1, 256]" in texts[2] and "n = 257 not in [1, 256]" in texts[3]
    assert "33 ranks x n = 256 are more than 8192 keys" in texts[4] and texts[5] == "" and texts[6] == "" and "exceed 4294967281" in texts[7] and "exceed" in texts[8]
    assert [o["lds"] for o in out[9:12]] == [1, 1, 0]
    assert [o["what"] for o in out[12:]] == [1, 0, 2, 2, 0]
