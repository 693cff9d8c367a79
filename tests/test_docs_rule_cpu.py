"""The rule of isle_hip_prune_docs without the library and without a GPU.  tests/docs_rule.py states it in numpy; here it is held to a
brute-force statement on Python integers, the cases of its table are shown to hit what they aim at, and isle_amd/csrc/docs_host.h (the
hash, the argument checks, the lengths, the first-of-its-kind table, the rule and the plain loop that builds the pruned CSC) is held to the
rule on every case through isle_amd/host/docs_host_main.cpp, built here with the address and undefined-behaviour sanitizers (a
stand-alone program, script on stdin, lines out).  Every comparison is == on integers: ids, lengths, offsets, count bits, the refusals'
texts."""
import json
import os
import subprocess

import numpy as np
import pytest

import docs_rule as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dr.CASES + dr.SHARDED + [dr.SHARD_REFUSAL]


def brute(case):
    """the rule on Python integers -> (refused, words, tokens, first_of as reported, kept documents as lists of (row, count bits), dropped)"""
    D = case.offs.size - 1
    bits = case.counts.view(np.uint32)
    docs = [[(int(case.rows[e]), int(bits[e])) for e in range(int(case.offs[d]), int(case.offs[d + 1]))] for d in range(D)]
    words = [len(doc) for doc in docs]
    tokens = [sum(int(case.counts[e]) for e in range(int(case.offs[d]), int(case.offs[d + 1]))) for d in range(D)]
    if (case.max_words and case.min_words > case.max_words) or (case.max_tokens and case.min_tokens > case.max_tokens):
        return True, words, tokens, None, None, None
    first, kept, dropped = [], [], [0, 0, 0]
    for d, doc in enumerate(docs):
        tests = [words[d] < case.min_words, tokens[d] < case.min_tokens, bool(case.max_words) and words[d] > case.max_words,
                 bool(case.max_tokens) and tokens[d] > case.max_tokens]
        if any(tests):
            dropped[tests.index(True) // 2] += 1
            first.append(dr.DROPPED)
            continue
        rep = next(j for j in range(d + 1) if docs[j] == doc) if case.dups else d
        first.append(rep)
        if rep == d:
            kept.append(d)
        else:
            dropped[2] += 1
    return not kept, words, tokens, first, kept, dropped


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("docs_host") / "docs_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "docs_host_main.cpp")], capture_output=True, text=True, timeout=300)
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


@pytest.mark.parametrize("case", [c for c in ALL if c.offs.size <= 2500 and c.rows.size <= 30000], ids=lambda c: c.name)
def test_the_numpy_rule_is_the_brute_force_statement(case):
    refused, words, tokens, first, kept, dropped = brute(case)
    got = dr.rule(case, doc_offset=11)
    assert got["words"].tolist() == words and got["tokens"].tolist() == tokens and bool(got["text"]) == refused
    if first is None:
        return
    assert got["first_of"].tolist() == first and got["dropped"] == dropped and np.flatnonzero(got["keep"]).tolist() == kept
    if refused:
        return
    bits = case.counts.view(np.uint32)
    assert got["kept_docs"].tolist() == [11 + d for d in kept] and got["docs"] == len(kept)
    assert got["offs"].tolist() == [0] + np.cumsum([words[d] for d in kept]).tolist()
    assert got["rows"].tolist() == [int(case.rows[e]) for d in kept for e in range(int(case.offs[d]), int(case.offs[d + 1]))]
    assert got["counts"].tolist() == [int(bits[e]) for d in kept for e in range(int(case.offs[d]), int(case.offs[d + 1]))]


def test_every_case_hits_what_it_aims_at():
    by = dr.BY_NAME
    r = {n: dr.rule(by[n]) for n in by if by[n].aim in ("edge", "refusal", "equality")}
    assert r["bounds_equal_a_length"]["words"].tolist() == [0, 1, 2, 5, 1, 3, 4] and r["bounds_equal_a_length"]["tokens"].tolist() == [0, 3, 2, 5, 1000, 4, 4]
    assert np.flatnonzero(r["bounds_equal_a_length"]["keep"]).tolist() == [2, 5, 6] and r["bounds_equal_a_length"]["dropped"] == [3, 1, 0]
    assert np.flatnonzero(r["min_equals_max"]["keep"]).tolist() == [5]
    assert np.flatnonzero(r["max_zero_is_none"]["keep"]).tolist() == [1, 2, 3, 4, 5, 6]
    assert r["fails_a_minimum_and_a_maximum"]["dropped"] == [3, 0, 0]        # the document of one word and 1000 tokens is counted below
    assert r["tokens_min_before_words_max"]["dropped"] == [5, 1, 0] and np.flatnonzero(r["tokens_min_before_words_max"]["keep"]).tolist() == [4]
    assert np.flatnonzero(r["words_only"]["keep"]).tolist() == [0, 1, 4] and np.flatnonzero(r["tokens_only"]["keep"]).tolist() == [1, 3, 5, 6]
    assert np.flatnonzero(r["tokens_min_equals_max"]["keep"]).tolist() == [5, 6]
    assert {n: r[n]["text"] for n in r if by[n].aim == "refusal"} == {
        "refuse_min_words_above_max": "prune_docs: min_words = 5 > max_words = 4",
        "refuse_min_tokens_above_max": "prune_docs: min_tokens = 9 > max_tokens = 8",
        "refuse_nothing_kept": "prune_docs: no document kept (min_words = 6, max_words = 0, min_tokens = 0, max_tokens = 0, drop_duplicates = 0)",
        "refuse_nothing_kept_band": "prune_docs: no document kept (min_words = 0, max_words = 0, min_tokens = 6, max_tokens = 999, drop_duplicates = 0)"}
    e = r["equality"]
    assert e["first_of"].tolist() == [0, 0, 2, 3, 4, 5, 5, 7, 8, 4, 10, 11, 12, 4, 5, 15, 16, 2, 18, 19, 18, 19]
    assert e["dropped"] == [0, 0, 8] and e["n_duplicates"] == 8 and int(e["tokens"][19]) == 2 * 4294967040 > 2 ** 32
    bits = by["equality"].counts.view(np.uint32)
    assert bits[by["equality"].offs[8] + 1] - bits[by["equality"].offs[7] + 1] == 1   # the next float up
    m = r["equality_min_words_1"]
    assert m["dropped"] == [3, 0, 6] and m["first_of"][[5, 6, 14]].tolist() == [dr.DROPPED] * 3
    assert r["equality_not_asked"]["docs"] == 22 and r["equality_not_asked"]["first_of"].tolist() == list(range(22))
    assert r["equality_and_bounds"]["dropped"] == [3, 9, 4]
    # the alternating runs: every run of the narrow form holds 75 documents of three contents, X, Y, Z, X, Y, Z, ...
    a = by["alternating_runs"]
    keys = [dr.narrow_key(a.rows[a.offs[d]:a.offs[d + 1]]) for d in range(300)]
    assert keys == [d % 4 for d in range(300)]
    fo = dr.rule(a)["first_of"]
    assert fo.tolist() == [d % 12 for d in range(300)] and fo[24] == 0      # the third X of run 0 (document 24) finds the first
    assert sorted(c.offs.size - 1 for c in dr.CASES if c.aim == "tile")[:8] == [2047, 2048, 2049, 4095, 4096, 4097, 4097, 8193]
    assert by["nnz_0"].rows.size == 0 and dr.rule(by["nnz_0"])["docs"] == 1 and dr.rule(by["nnz_0_not_asked"])["docs"] == 5
    w = dr.rule(by["wave"])
    assert w["words"].tolist() == [63, 64, 65, 5000, 5000, 65, 64, 63, 5000, 5000] and w["first_of"].tolist() == [0, 1, 2, 3, 4, 2, 1, 0, 3, 9]
    assert dr.rule(by["wave_bounds"])["dropped"] == [2, 1, 3]
    lens = np.diff(by["empties"].offs)
    assert lens[0] == 0 and lens[-1] == 0 and (lens[4:2004] == 0).all()
    assert dr.rule(by["empties"])["docs"] == 6 and dr.rule(by["empties_min_words_1"])["dropped"] == [2002, 0, 0]
    c7 = dr.rule(by["copies_70000"])
    assert c7["docs"] == 1 and c7["dropped"] == [0, 0, 69999] and 69999 > 65535
    for n in ("identity", "identity_not_asked"):
        i = dr.rule(by[n])
        assert np.array_equal(i["offs"], by[n].offs) and np.array_equal(i["rows"], by[n].rows) and i["dropped"] == [0, 0, 0]
        assert np.array_equal(i["kept_docs"], np.arange(by[n].offs.size - 1))
    assert dr.rule(by["identity_not_asked"])["n_duplicates"] == 1     # (a duplicate is there, and stays: nobody asked)


def test_the_shard_cuts_are_what_the_sharded_test_is_about():
    a, b, c = dr.SHARDED
    ka, kb = dr.rule(a)["keep"], dr.rule(b)["keep"]
    cut3 = dr.cuts(a, 3)
    assert cut3[1] == cut3[2] == 2 and not ka[:2].any() and ka[2:].any()     # world 3: rank 0's documents are all dropped, rank 1 has none
    assert dr.rule_share(a, cut3, 2)[4] == 0                                   # ... so the documents of rank 2 start the corpus
    assert dr.cuts(b, 2)[1] == 5 and not kb[:5].any() and kb[5:].any()       # world 2: rank 0 is left with nothing
    assert dr.rule(b)["dropped"][1] == 5 and dr.rule(b)["dropped"][0] == 1
    rc = dr.rule(c)
    assert min(rc["dropped"][:2]) > 0 and 0 < rc["docs"] < 1500 and c.dups == 0
    assert dr.rule(dr.SHARD_REFUSAL)["text"] == "prune_docs: no document kept (min_words = 5, max_words = 0, min_tokens = 0, max_tokens = 0, drop_duplicates = 0)"
    for case in dr.SHARDED:   # the slices of the single-rank result put together are the single-rank result
        for world in (1, 2, 3):
            cut, want = dr.cuts(case, world), dr.rule(case)
            parts = [dr.rule_share(case, cut, q) for q in range(world)]
            assert np.array_equal(np.concatenate([p[1] for p in parts]), want["rows"]) and np.array_equal(np.concatenate([p[3] for p in parts]), want["kept_docs"])
            assert [p[4] for p in parts] == np.cumsum([0] + [p[3].size for p in parts[:-1]]).tolist()


def test_the_header_answers_as_the_rule_does(exe):
    script = [["consts"]]
    hashed = [([], []), ([3], [0x3F800000]), ([0, 5, 9], [0x3F800000, 0x40000000, 0x4F7FFFFF]), ([9, 5, 0], [0x4F7FFFFF, 0x40000000, 0x3F800000])]
    script += [["hash"] + lst(r) + lst(b) for r, b in hashed]
    tests = [(1, 1000, 2, 0, 0, 500), (5, 5, 0, 2, 5, 0), (4, 4, 0, 2, 5, 0), (3, 4, 3, 3, 4, 4), (3, 4, 3, 3, 4, 3), (0, 0, 0, 0, 0, 0)]
    script += [["fails"] + list(t) for t in tests]
    args = [("prune_docs", 0, 0, 0, 0, 0, 0, 1), ("prune_docs", 1, 5, 4, 0, 0, 0, 1), ("prune_docs", 1, 5, 0, 9, 8, 0, 1), ("prune_docs", 1, 5, 5, 8, 8, 1, 1),
            ("prune_docs", 1, 0, 0, 0, 0, 2, 1), ("prune_docs", 1, 0, 0, 0, 0, -1, 3), ("prune_docs", 1, 0, 0, 0, 0, 1, 3), ("doc_duplicates", 1, 0, 0, 0, 0, 1, 2),
            ("prune_docs", 1, 9, 8, 0, 0, 0, 3), ("doc_lengths", 0, 0, 0, 0, 0, 0, 1)]
    script += [["args"] + list(a) for a in args]
    n_head = len(script)
    for c in ALL:
        script.append(["prune", c.min_words, c.max_words, c.min_tokens, c.max_tokens, c.dups, 11] + lst(c.offs) + lst(c.rows) + lst(c.counts.view(np.uint32)))
    out = run(exe, script)
    assert out[0] == dict(dropped=dr.DROPPED, narrow_bits=dr.NARROW_BITS, forms=[0, 1, 2], key_bits=[64, dr.NARROW_BITS])
    for (r, b), o in zip(hashed, out[1:5]):
        assert o["hash"] == dr.doc_hash(r, b) and o["narrow"] == dr.doc_hash(r, b) % (1 << dr.NARROW_BITS)
    assert out[1]["hash"] == 0 and out[3]["hash"] == out[4]["hash"] != out[2]["hash"]          # a commutative sum
    assert [o["fails"] for o in out[5:5 + len(tests)]] == [1, 2, 1, 0, 2, 0]
    assert [o["text"] for o in out[5 + len(tests):n_head]] == [dr.check_args(*a[2:7], world=a[7], who=a[0], has_A=bool(a[1])) for a in args] == [
        "prune_docs: no count matrix", "prune_docs: min_words = 5 > max_words = 4", "prune_docs: min_tokens = 9 > max_tokens = 8", "",
        "prune_docs: drop_duplicates = 2, neither 0 nor 1", "prune_docs: drop_duplicates = -1, neither 0 nor 1",
        "prune_docs: duplicates with 3 ranks: equality across ranks needs the contents exchanged",
        "doc_duplicates: duplicates with 2 ranks: equality across ranks needs the contents exchanged", "prune_docs: min_words = 9 > max_words = 8",
        "doc_lengths: no count matrix"]
    for c, got in zip(ALL, out[n_head:]):
        want = dr.rule(c, doc_offset=11)
        assert got["text"] == want["text"], c.name
        assert got["words"] == want["words"].tolist() and got["tokens"] == want["tokens"].tolist(), c.name
        assert got["all_first_of"] == want["all_first_of"].tolist() and got["n_duplicates"] == want["n_duplicates"], c.name
        if "first_of" not in want:      # refused by its arguments
            assert got["first_of"] == [] and got["offs"] == []
            continue
        assert got["first_of"] == want["first_of"].tolist() and got["dropped"] == want["dropped"], c.name
        if want["text"]:
            assert got["kept_docs"] == [] and got["offs"] == []
            continue
        assert got["kept_docs"] == want["kept_docs"].tolist() and got["offs"] == want["offs"].tolist(), c.name
        assert got["rows"] == want["rows"].tolist() and got["counts"] == want["counts"].tolist(), c.name


def test_the_library_header_carries_the_same_forms():
    text = open(os.path.join(ROOT, "include", "isle_hip.h")).read()
    for name, value in (("ISLE_DOC_HASH_AUTO", 0), ("ISLE_DOC_HASH_FULL", 1), ("ISLE_DOC_HASH_NARROW", 2)):
        assert "#define %s %d" % (name, value) in text
    host = open(os.path.join(ROOT, "isle_amd", "csrc", "docs_host.h")).read()
    assert "DOC_HASH_AUTO = 0, DOC_HASH_FULL = 1, DOC_HASH_NARROW = 2" in host and "DOCS_NARROW_BITS = %d" % dr.NARROW_BITS in host
