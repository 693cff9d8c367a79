"""The rule of isle_hip_prune_vocab without the library and without a GPU.  tests/vocab_rule.py states it in numpy; here it is held to a
brute-force statement on Python integers, every case of its table is shown to hit what it aims at, and isle_amd/csrc/vocab_host.h (the
key, the argument checks, the rule on a table, the plain loop that builds the pruned CSC) is held to the rule on every case through
isle_amd/host/vocab_host_main.cpp, built here with the address and undefined-behaviour sanitizers (a stand-alone program, script on stdin,
lines out).  Every comparison is == on integers: ids, offsets, count bits, the refusals' texts."""
import json
import os
import subprocess

import numpy as np
import pytest

import vocab_rule as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = vr.CASES + vr.SHARDED + [vr.SHARD_REFUSAL]


def brute(case):
    """the rule on Python integers: (text, kept words, new documents as lists of (new id, count bits), emptied)"""
    D = case.offs.size - 1
    docs = [[(int(case.rows[e]), int(case.counts[e:e + 1].view(np.uint32)[0])) for e in range(int(case.offs[d]), int(case.offs[d + 1]))] for d in range(D)]
    df = [0] * case.V
    for doc in docs:
        for w, _ in doc:
            df[w] += 1
    top = case.max_df or D
    if case.min_df > top or case.keep_n >= 2 ** 32:
        return "refused", df, None, None, None
    passers = [w for w in range(case.V) if case.min_df <= df[w] <= top]
    if case.keep_n and len(passers) > case.keep_n:
        passers = sorted(sorted(passers, key=lambda w: (df[w] << 32) | (~w & 0xFFFFFFFF), reverse=True)[:case.keep_n])
    if not passers:
        return "refused", df, None, None, None
    new = {w: i for i, w in enumerate(passers)}
    out = [[(new[w], b) for w, b in doc if w in new] for doc in docs]
    return "", df, passers, out, sum(1 for a, b in zip(docs, out) if a and not b)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vocab_host") / "vocab_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "vocab_host_main.cpp")], capture_output=True, text=True, timeout=300)
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


@pytest.mark.parametrize("case", [c for c in ALL if c.rows.size <= 70000], ids=lambda c: c.name)
def test_the_numpy_rule_is_the_brute_force_statement(case):
    text, df, kept, docs, emptied = brute(case)
    got = vr.rule(case)
    assert got["df"].tolist() == df and bool(got["text"]) == bool(text)
    if text:
        return
    assert got["kept_words"].tolist() == kept and got["vocab"] == len(kept) and got["docs_emptied"] == emptied
    assert got["offs"].tolist() == [0] + np.cumsum([len(d) for d in docs]).tolist()
    assert got["rows"].tolist() == [w for d in docs for w, _ in d] and got["counts"].tolist() == [b for d in docs for _, b in d]
    for d in range(case.offs.size - 1):   # every column still ascends strictly
        r = got["rows"][got["offs"][d]:got["offs"][d + 1]]
        assert (np.diff(r.astype(np.int64)) > 0).all()


def test_every_case_hits_what_it_aims_at():
    by = vr.BY_NAME
    df = vr.df_of(8, by["ties_cut_inside"].rows).tolist()
    assert df == [5, 3, 3, 3, 1, 0, 2, 0]
    assert vr.rule(by["ties_cut_inside"])["kept_words"].tolist() == [0, 1]       # three words tie at df 3 across the cut: the smallest id
    assert vr.rule(by["ties_cut_inside_3"])["kept_words"].tolist() == [0, 1, 2]
    passers = sum(1 for x in df if x >= 1)
    assert [by[n].keep_n - passers for n in ("keep_n_equals_passers", "keep_n_one_below", "keep_n_above")] == [0, -1, 1]
    assert vr.rule(by["keep_n_one_below"])["kept_words"].tolist() == [0, 1, 2, 3, 6]
    assert vr.rule(by["keep_n_equals_passers"])["kept_words"].tolist() == vr.rule(by["keep_n_above"])["kept_words"].tolist() == [0, 1, 2, 3, 4, 6]
    assert vr.rule(by["keep_n_one"])["kept_words"].tolist() == [0]
    assert by["min_equals_max"].min_df == by["min_equals_max"].max_df and vr.rule(by["min_equals_max"])["kept_words"].tolist() == [1, 2, 3]
    r = vr.rule(by["min_zero_keeps_absent"])
    assert r["kept_words"].tolist() == list(range(8)) and 0 in df
    assert vr.rule(by["min_zero_max_small"])["kept_words"].tolist() == [4, 5, 7]
    assert vr.rule(by["max_df_none_is_doc_count"])["kept_words"].tolist() == [0]
    texts = {n: vr.rule(by[n])["text"] for n in by if by[n].aim == "refusal"}
    assert texts == {"refuse_min_above_max": "prune_vocab: min_df = 4 > max_df = 3",
                     "refuse_min_above_docs": "prune_vocab: min_df = 7 > max_df = 6 (the corpus's document count)",
                     "refuse_keep_n_2_32": "prune_vocab: keep_n = 4294967296, 2^32 or more",
                     "refuse_nothing_kept": "prune_vocab: no word kept (min_df = 4, max_df = 4, keep_n = 0)"}
    assert sorted(c.rows.size for c in vr.CASES if c.aim == "nnz") == [0, vr.SCAN_TILE - 1, vr.SCAN_TILE, vr.SCAN_TILE + 1, 2 * vr.SCAN_TILE + 1]
    assert by["nnz_0"].offs.size - 1 > 0
    assert sorted(c.V for c in vr.CASES if c.aim == "part") == [vr.PART - 1, vr.PART, vr.PART + 1, 2 * vr.PART + 3]
    for c in vr.CASES:
        if c.aim == "part":   # words either side of every part boundary occur, kept and dropped words on both sides, several workgroups' worth of entries
            d = vr.df_of(c.V, c.rows)
            assert all(d[w] > 0 for w in (0, vr.PART - 2, c.V - 1) if w < c.V) and all(d[w] > 0 for w in (vr.PART, 2 * vr.PART + 2) if w < c.V)
            k = vr.rule(c)["kept_words"]
            assert c.rows.size > 3 * 4096 and 0 < k.size < c.V and (c.V <= vr.PART or (k >= vr.PART).any())
    h = by["head_70000"]
    d = vr.df_of(h.V, h.rows)
    assert d[0] == 70000 > 65535 and d[1] == 69999 and vr.rule(h)["kept_words"][0] == 1
    docs = by["documents_lose"]
    lens, new = np.diff(docs.offs), np.diff(vr.rule(docs)["offs"])
    assert lens[0] == 0 and lens[-1] == 0 and (lens[4:2004] == 0).all() and vr.rule(docs)["docs_emptied"] == 1
    first = 2004
    assert [(int(lens[first + i]), int(new[first + i])) for i in range(3)] == [(3, 2), (3, 2), (2, 0)]   # loses its first, its last, all
    one = by["one_document_all_words"]
    assert np.diff(one.offs)[0] == one.V == 5000
    cn = by["counts"].counts
    assert (cn != np.floor(cn)).any() and (cn > 2 ** 24).any()
    ke = vr.rule(by["keeps_everything"])
    assert ke["vocab"] == 900 and np.array_equal(ke["rows"], by["keeps_everything"].rows) and np.array_equal(ke["offs"], by["keeps_everything"].offs)


def test_the_shard_cuts_are_what_the_sharded_test_is_about():
    c = vr.SHARDED[0]
    cut2, cut3 = vr.cuts(c, 2), vr.cuts(c, 3)
    local = [vr.df_of(c.V, vr.share(c, cut2, q)[1]) for q in range(2)]
    assert local[0][2] == 1 and local[1][2] == 1 and c.min_df == 2 and 2 in vr.rule(c)["kept_words"]   # w2 reaches min_df only summed
    assert cut3[1] == cut3[2] > 0 and c.offs[cut3[1]] == 0        # rank 0: documents and no entries; rank 1: no documents
    t = vr.SHARDED[1]
    d = vr.df_of(t.V, t.rows)
    assert vr.rule(t)["kept_words"].tolist() == [0, 3, 4] and d[0] == d[3] == 3 and t.keep_n == 3
    z = vr.SHARDED[2]
    b = vr.cuts(z, 3)
    assert b[1] == b[2] and 0 < vr.rule(z)["vocab"] < z.V
    assert vr.rule(vr.SHARD_REFUSAL)["text"] == "prune_vocab: no word kept (min_df = 5, max_df = 9, keep_n = 0)"


def test_the_header_answers_as_the_rule_does(exe):
    small = ALL
    script = [["parts", V] for V in (1, vr.PART - 1, vr.PART, vr.PART + 1, 2 * vr.PART + 3)]
    script += [["key", 5, 0], ["key", 3, 7], ["key", 0xFFFFFFF0, 0xFFFFFFEF]]
    script += [["args", 0, 1, 0, 0, 10], ["args", 1, 11, 0, 0, 10], ["args", 1, 10, 0, 0, 10], ["args", 1, 4, 3, 0, 10], ["args", 1, 1, 0, 2 ** 32, 10],
               ["args", 1, 1, 0, 2 ** 32 - 1, 10], ["args", 1, 1, 0, 0, 0], ["args", 1, 0, 0, 0, 0]]
    n_head = len(script)
    for c in small:
        D = c.offs.size - 1
        script.append(["prune", c.min_df, c.max_df, c.keep_n, D, c.V] + lst(c.offs) + lst(c.rows) + lst(c.counts.view(np.uint32)))
        script.append(["rule", c.min_df, c.max_df, c.keep_n, D] + lst(vr.df_of(c.V, c.rows)))
    out = run(exe, script)
    assert [o["parts"] for o in out[:5]] == [1, 1, 1, 2, 3] and all(o["part"] == vr.PART for o in out[:5])
    assert [o["key"] for o in out[5:8]] == [(5 << 32) | 0xFFFFFFFF, (3 << 32) | 0xFFFFFFF8, (0xFFFFFFF0 << 32) | 0x10]
    assert [o["text"] for o in out[8:n_head]] == ["prune_vocab: no count matrix", "prune_vocab: min_df = 11 > max_df = 10 (the corpus's document count)", "",
                                                 "prune_vocab: min_df = 4 > max_df = 3", "prune_vocab: keep_n = 4294967296, 2^32 or more", "",
                                                 "prune_vocab: min_df = 1 > max_df = 0 (the corpus's document count)", ""]
    for i, c in enumerate(small):
        got, tab, want = out[n_head + 2 * i], out[n_head + 2 * i + 1], vr.rule(c)
        assert got["text"] == tab["text"] == want["text"], c.name
        assert got["df"] == want["df"].tolist(), c.name
        if want["text"]:
            assert got["kept_words"] == [] and got["offs"] == [] and tab["kept_words"] == []
            continue
        assert got["kept_words"] == tab["kept_words"] == want["kept_words"].tolist(), c.name
        assert np.array_equal(np.array(tab["remap"], np.int64).astype(np.uint32), want["remap"]), c.name
        assert got["offs"] == want["offs"].tolist() and got["rows"] == want["rows"].tolist() and got["counts"] == want["counts"].tolist(), c.name
        assert got["docs_emptied"] == want["docs_emptied"], c.name


def test_the_python_layer_states_the_float_rule_once():
    import isle_amd.hot_path as hpm
    doc = hpm.HotPath.prune_vocab.__doc__
    assert doc.count("floor(max_df * docs_global)") == 1
