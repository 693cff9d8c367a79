"""The rule of isle_hip_prune_near_docs without the library and without a GPU.  tests/neardup_rule.py states it in numpy; here it is held to
a brute-force statement on Python sets and integers, the cases of its table are shown to hit what they aim at by the rule alone, the
properties P1 - P3 are checked in both forms of the key, a recall case is checked, and isle_amd/csrc/neardup_host.h (the hashes, the
argument checks, the signatures, the band keys, the set sizes, the resolution, the roots and the pruned CSC) is held to the rule on every
case through isle_amd/host/neardup_host_main.cpp, built here with the address and undefined-behaviour sanitizers (a stand-alone program,
script on stdin, lines out).  Every comparison is == on integers."""
import json
import os
import subprocess

import numpy as np
import pytest

import neardup_rule as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1


def py_mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


_SIGS = {}


def brute(case, form):
    """the rule on Python sets and integers -> (sig, keys, parent, first_of, pairs_tested, rounds)"""
    D, H = case.offs.size - 1, case.bands * case.rows_per_band
    sets = [set(int(w) for w in case.rows[case.offs[d]:case.offs[d + 1]]) for d in range(D)]
    if case.name not in _SIGS:      # (the signatures do not depend on the form)
        sig = [[min([py_mix(((i + 1) << 32) | w) for w in s], default=M) for i in range(H)] for s in sets]
        keys = []
        for b in range(case.bands):
            row = []
            for d in range(D):
                k = 0
                for j in range(case.rows_per_band):
                    k = py_mix(k ^ sig[d][b * case.rows_per_band + j])
                row.append(k)
            keys.append(row)
        _SIGS[case.name] = (sig, keys)
    sig, keys = _SIGS[case.name]
    parent, tested, rounds = list(range(D)), 0, 0
    for b in range(case.bands):
        groups = {}
        for d in range(D):
            if parent[d] == d:
                groups.setdefault(keys[b][d] & 3 if form == "narrow" else keys[b][d], []).append(d)
        most = 0
        for members in groups.values():
            leaders = []
            for d in members:
                for l in leaders:
                    tested += 1
                    inter = len(sets[d] & sets[l])
                    if inter * case.den >= case.num * len(sets[d] | sets[l]):
                        parent[d] = l
                        break
                else:
                    leaders.append(d)
            most = max(most, len(leaders))
        rounds += most
    first = []
    for d in range(D):
        x = d
        while parent[x] != x:
            x = parent[x]
        first.append(x)
    return sig, keys, parent, first, tested, rounds


BRUTE = [c for c in nr.CASES if c.rows.size * c.bands * c.rows_per_band <= 2000000 and c.offs.size <= 2040]


@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("case", BRUTE, ids=lambda c: c.name)
def test_the_numpy_rule_is_the_brute_force_statement(case, form):
    sig, keys, parent, first, tested, rounds = brute(case, form)
    got = nr.rule(case, form)
    assert got["sig"].tolist() == sig and got["keys"].tolist() == keys
    assert got["parent"].tolist() == parent and got["first_of"].tolist() == first
    assert (got["pairs_tested"], got["rounds"], got["n_dropped"]) == (tested, rounds, sum(f != d for d, f in enumerate(first)))
    a = [set(int(w) for w in case.rows[case.offs[x]:case.offs[x + 1]]) for x in case.pairs[:, 0]]
    b = [set(int(w) for w in case.rows[case.offs[x]:case.offs[x + 1]]) for x in case.pairs[:, 1]]
    assert got["inter"].tolist() == [len(x & y) for x, y in zip(a, b)] and got["uni"].tolist() == [len(x | y) for x, y in zip(a, b)]
    # the pruned matrix: the kept documents' columns in order
    kept = [d for d in range(len(first)) if first[d] == d]
    bits = case.counts.view(np.uint32)
    assert got["kept_docs"].tolist() == kept and got["docs"] == len(kept)
    assert got["offs"].tolist() == [0] + np.cumsum([case.offs[d + 1] - case.offs[d] for d in kept]).tolist()
    assert got["rows"].tolist() == [int(case.rows[e]) for d in kept for e in range(int(case.offs[d]), int(case.offs[d + 1]))]
    assert got["counts"].tolist() == [int(bits[e]) for d in kept for e in range(int(case.offs[d]), int(case.offs[d + 1]))]


def test_the_brute_force_covers_the_table_but_its_largest_cases():
    assert sorted(c.name for c in nr.CASES if c not in BRUTE) == ["D_2047", "D_2048", "D_2049", "D_4095", "D_4096", "D_4097", "D_8193", "copies_70000", "lengths_16x8"]


@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("case", nr.CASES, ids=lambda c: c.name)
def test_the_properties_hold_in_both_forms(case, form):
    r = nr.rule(case, form)
    D = case.offs.size - 1
    n = np.diff(case.offs)
    ids = np.arange(D)
    dropped = np.flatnonzero(r["first_of"] != ids)
    # (P1) a dropped document's parent is an earlier document it is similar to; a kept one is its own parent
    assert (r["parent"][dropped] < dropped).all() and np.array_equal(r["parent"][r["keep"]], ids[r["keep"]])
    for d in dropped[:: max(1, dropped.size // 300)]:
        p = int(r["parent"][d])
        inter = np.intersect1d(case.rows[case.offs[d]:case.offs[d + 1]], case.rows[case.offs[p]:case.offs[p + 1]], assume_unique=True).size
        assert nr.similar(inter, int(n[d]), int(n[p]), case.num, case.den)
    assert np.array_equal(r["first_of"][r["first_of"]], r["first_of"])                  # roots are roots
    # (P2) the same word set, the same first_of
    seen, smallest = {}, np.empty(D, np.int64)
    for d in range(D):
        smallest[d] = seen.setdefault(case.rows[case.offs[d]:case.offs[d + 1]].tobytes(), d)
    assert np.array_equal(r["first_of"][smallest], r["first_of"])
    # (P3) num == den: the partition is "equal word sets"
    if case.num == case.den:
        assert np.array_equal(r["first_of"], smallest)
    # the length filter changed no answer: every test it decided was a dissimilar pair
    for b, d, l, allowed, sim in r["trace"][:: max(1, len(r["trace"]) // 2000)]:
        if not allowed:
            inter = np.intersect1d(case.rows[case.offs[d]:case.offs[d + 1]], case.rows[case.offs[l]:case.offs[l + 1]], assume_unique=True).size
            assert not sim and not nr.similar(inter, int(n[d]), int(n[l]), case.num, case.den)


def test_every_case_hits_what_it_aims_at():
    by = nr.BY_NAME
    # ---- the lengths and the shapes of the signature
    ld = by["lengths_16x4"]
    lens = np.diff(ld.offs).tolist()
    assert lens[0] == 0 and lens[-1] == 0 and {0, 1, 63, 64, 65, 5000} <= set(lens) and lens[-3] == 0
    shapes = sorted((c.bands, c.rows_per_band) for c in nr.CASES if c.aim == "lengths")
    assert shapes == [(1, 1), (13, 5), (16, 4), (16, 8), (63, 1), (64, 1)]
    assert [b * r for b, r in shapes] == [1, 65, 64, 128, 63, 64] and 64 % 5 != 0 and 64 % 4 == 0
    for c in nr.CASES:
        if c.aim == "lengths":
            r = nr.rule(c, "full")
            assert (r["sig"][0] == nr.EMPTY_SIG).all() and (r["sig"][-1] == nr.EMPTY_SIG).all() and r["first_of"][-1] == 0   # empty documents are similar
    r = nr.rule(ld, "full")
    assert np.flatnonzero(np.diff(ld.offs) >= 4999).tolist() == [11, 12, 13, 14, 18] and r["first_of"][[11, 12, 13, 14, 18]].tolist() == [11, 11, 13, 11, 11]
    # ---- the threshold and the length filter, on and off their boundaries: (inter, uni) by the rule's own sizes, tested in the narrow form
    t, named = by["threshold_edges"], nr.THRESHOLD_DOCS
    r = nr.rule(t, "narrow")
    n = np.diff(t.offs)
    size = {(int(a), int(b)): (int(i), int(u)) for (a, b), i, u in zip(t.pairs, r["inter"], r["uni"])}
    met = {(d, l): (allowed, sim) for b, d, l, allowed, sim in r["trace"]}
    a, b = named["on_threshold"]
    assert size[(a, b)] == (4, 5) and 4 * t.den == t.num * 5 and met[(b, a)] == (True, True) and r["parent"][b] == a
    assert min(n[a], n[b]) * t.den == t.num * max(n[a], n[b])                              # ... and on the filter's boundary too: read
    a, b = named["below_threshold"]
    assert size[(a, b)] == (3999, 5000) and met[(b, a)] == (True, False) and r["parent"][b] == b
    a, b = named["above_threshold"]
    assert size[(a, b)] == (4000, 5000) and met[(b, a)] == (True, True) and r["parent"][b] == a
    a, b = named["filter_on"]
    assert (n[a], n[b]) == (5, 4) and size[(a, b)] == (3, 6) and met[(b, a)] == (True, False)
    a, b = named["filter_off"]
    assert (n[a], n[b]) == (6, 4) and 4 * t.den == t.num * 6 - 4 and size[(a, b)] == (4, 6) and met[(b, a)] == (False, False)
    a, b, c = named["filter_off_by_one"]
    assert (n[a], n[b], n[c]) == (10, 8, 7) and met[(b, a)] == (True, True) and met[(c, a)] == (False, False) and 7 * t.den == t.num * 10 - 5
    a, b, c = named["subset"]
    assert size[(a, b)] == (10, 20) and size[(a, c)] == (17, 20) and met[(b, a)] == (False, False) and met[(c, a)] == (True, True)
    a, b, c = named["disjoint"]
    assert size[(a, b)] == (0, 24) and size[(a, c)] == (6, 18) and met[(b, a)] == (True, False) and met[(c, a)] == (True, False) and met[(c, b)] == (True, False)
    # ---- num == den
    e = nr.rule(by["equal_sets_1x1"], "full")
    assert e["first_of"].tolist() == [0, 0, 2, 3, 4, 5, 0, 4, 5, 9, 10, 2] and by["equal_sets_13x5"].num == by["equal_sets_13x5"].den == 7
    assert by["equal_sets_pool"].den == nr.MAX_DEN
    # ---- the alternating groups: in the narrow form every group of band 0 holds 75 documents of three disjoint sets, X, Y, Z, X, Y, Z, ...
    alt = by["alternating_groups"]
    ra = nr.rule(alt, "narrow")
    assert nr.cut(ra["keys"][0], "narrow").tolist() == [int(nr.cut(ra["keys"][0], "narrow")[d % 4]) for d in range(300)]
    assert len(set(nr.cut(ra["keys"][0], "narrow")[:4].tolist())) == 4
    band0 = [x for x in ra["trace"] if x[0] == 0]
    leaders_of = {}
    for _, d, l, _, sim in band0:
        leaders_of.setdefault(d, []).append(l)
    assert max(len(v) for v in leaders_of.values()) == 3 and leaders_of[24] == [0] and leaders_of[32] == [0, 4, 8]    # the third kind finds its leader in round 3
    assert ra["first_of"].tolist() == [d % 12 for d in range(300)]
    # ---- the chain across bands (full form)
    depth, deep = nr.chain_depth(by["cross_band_chain"], "full")
    rc = nr.rule(by["cross_band_chain"], "full")
    assert depth >= 2 and deep and (rc["first_of"] != rc["parent"]).any() and nr.find_chain_seed() == nr.CHAIN_SEED
    # ---- one group of 70 000 copies: one round
    c7 = by["copies_70000"]
    for form in nr.FORMS:
        r7 = nr.rule(c7, form)
        assert (r7["rounds"], r7["pairs_tested"], r7["n_dropped"], r7["docs"]) == (1, 69999, 69999, 1) and 69999 > 65535
    # ---- the tiles, and the narrow form's budget: a few hundred rounds at the most
    assert sorted(c.offs.size - 1 for c in nr.CASES if c.aim == "tile") == [2047, 2048, 2049, 4095, 4096, 4097, 8193]
    assert max(nr.rule(c, "narrow")["rounds"] for c in nr.CASES) < 400
    le = np.diff(by["empties"].offs)
    assert le[0] == 0 and le[-1] == 0 and (le[4:2004] == 0).all() and nr.rule(by["empties"], "full")["docs"] == 5


def test_recall_of_planted_pairs():
    case = nr.recall_case()
    assert case.pairs.shape == (200, 2)
    inter, uni = nr.jaccard(case.offs, case.rows, case.pairs)
    assert (inter.astype(np.int64) * 10 >= 9 * uni.astype(np.int64)).all()                # every planted pair has Jaccard >= 0.9
    for form in nr.FORMS:
        r = nr.rule(case, form)
        assert np.array_equal(r["first_of"][case.pairs[:, 0]], r["first_of"][case.pairs[:, 1]]), form
    assert nr.rule(case, "full")["n_dropped"] == 200


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("neardup_host") / "neardup_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "neardup_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    text = "\n".join(" ".join(str(t) for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o.pop("cmd") for o in out] == [line[0] for line in script]
    return out


def lst(a):
    a = np.asarray(a).reshape(-1)
    return [a.size] + [int(x) for x in a]


def shown(c, form):
    """whether the program prints the case's signatures and keys too (they do not depend on the form; the largest tables stay inside)"""
    return form == "full" and (c.offs.size - 1) * c.bands * c.rows_per_band <= 300000


def test_the_header_answers_as_the_rule_does(exe):
    script = [["consts"]]
    hashed = [(0, 0), (0, 7), (63, 7), (64, 7), (127, 0xFFFFFFFF)]
    script += [["hash", i, w] for i, w in hashed]
    sims = [(4, 5, 4, 4, 5), (3999, 4500, 4499, 4, 5), (4000, 4500, 4500, 4, 5), (4, 6, 4, 4, 5), (0, 0, 0, 4, 5), (0, 0, 3, 1, 65535), (3, 3, 3, 7, 7), (2, 3, 3, 7, 7)]
    script += [["similar"] + list(s) for s in sims]
    args = [("doc_near_duplicates", 0, 4, 5, 16, 4, 1), ("prune_near_docs", 1, 4, 5, 16, 4, 2), ("doc_jaccard", 1, 1, 1, 1, 1, 3), ("prune_near_docs", 1, 0, 5, 16, 4, 1),
            ("prune_near_docs", 1, 6, 5, 16, 4, 1), ("doc_near_duplicates", 1, 1, 65536, 16, 4, 1), ("doc_near_duplicates", 1, 65535, 65535, 16, 4, 1),
            ("doc_signatures", 1, 1, 1, 0, 4, 1), ("doc_signatures", 1, 1, 1, 65, 1, 1), ("doc_signatures", 1, 1, 1, 16, 9, 1), ("doc_signatures", 1, 1, 1, 17, 8, 1),
            ("doc_signatures", 1, 1, 1, 64, 2, 1), ("doc_signatures", 1, 1, 1, -1, 4, 1)]
    script += [["args"] + list(a) for a in args]
    pairs = [(5, [0, 4, 5], [1, 2, 3]), (5, [0, 4], [1, 7]), (5, [], []), (0, [0], [0])]
    script += [["pairs", D] + lst(a) + lst(b) for D, a, b in pairs]
    n_head = len(script)
    runs = [(c, form) for c in nr.CASES for form in nr.FORMS]
    for c, form in runs:
        script.append(["rule", int(form == "narrow"), int(shown(c, form)), c.num, c.den, c.bands, c.rows_per_band, 11] + lst(c.offs) + lst(c.rows) + lst(c.counts.view(np.uint32))
                      + lst(c.pairs[:, 0]) + lst(c.pairs[:, 1]))
    out = run(exe, script)
    assert out[0] == dict(forms=[nr.KEY_AUTO, nr.KEY_FULL, nr.KEY_NARROW], limits=[nr.MAX_BANDS, nr.MAX_ROWS, nr.MAX_H, nr.MAX_DEN], empty_sig=nr.EMPTY_SIG,
                          narrow_bits=nr.dr.NARROW_BITS)
    assert [o["hash"] for o in out[1:6]] == [py_mix(((i + 1) << 32) | w) for i, w in hashed] == [int(nr.nd_hash(i, w)) for i, w in hashed]
    at = 6
    assert [(o["allow"], o["similar"]) for o in out[at:at + len(sims)]] == [(1, 1), (1, 0), (1, 1), (0, 0), (1, 1), (0, 0), (1, 1), (1, 0)]
    assert [(o["allow"], o["similar"]) for o in out[at:at + len(sims)]] == [(int(nr.lengths_allow(a, b, n, d)), int(nr.similar(i, a, b, n, d))) for i, a, b, n, d in sims]
    at += len(sims)
    assert [o["text"] for o in out[at:at + len(args)]] == [nr.check_args(a[0], bool(a[1]), *a[2:6], world=a[6]) for a in args] == [
        "doc_near_duplicates: no count matrix",
        "prune_near_docs: near duplicates with 2 ranks: similarity across ranks needs the contents exchanged: out of scope",
        "doc_jaccard: near duplicates with 3 ranks: similarity across ranks needs the contents exchanged: out of scope",
        "prune_near_docs: threshold 0/5, not 1 <= num <= den <= 65535", "prune_near_docs: threshold 6/5, not 1 <= num <= den <= 65535",
        "doc_near_duplicates: threshold 1/65536, not 1 <= num <= den <= 65535", "",
        "doc_signatures: bands = 0, rows_per_band = 4, not 1 <= bands <= 64, 1 <= rows_per_band <= 8, bands rows_per_band <= 128",
        "doc_signatures: bands = 65, rows_per_band = 1, not 1 <= bands <= 64, 1 <= rows_per_band <= 8, bands rows_per_band <= 128",
        "doc_signatures: bands = 16, rows_per_band = 9, not 1 <= bands <= 64, 1 <= rows_per_band <= 8, bands rows_per_band <= 128",
        "doc_signatures: bands = 17, rows_per_band = 8, not 1 <= bands <= 64, 1 <= rows_per_band <= 8, bands rows_per_band <= 128", "",
        "doc_signatures: bands = -1, rows_per_band = 4, not 1 <= bands <= 64, 1 <= rows_per_band <= 8, bands rows_per_band <= 128"]
    at += len(args)
    assert [(o["bad"], o["text"]) for o in out[at:n_head]] == [(2, nr.bad_pair(2, 5, 3, 5)), (1, nr.bad_pair(1, 4, 7, 5)), (0, ""), (0, nr.bad_pair(0, 0, 0, 0))]
    assert nr.bad_pair(2, 5, 3, 5) == "doc_jaccard: pair 2 names documents 5 and 3 of 5"
    for (c, form), got in zip(runs, out[n_head:]):
        want = nr.rule(c, form, doc_offset=11)
        name = c.name + " " + form
        assert got["text"] == want["text"] == "", name
        if shown(c, form):
            assert got["sig"] == want["sig"].reshape(-1).tolist() and got["keys"] == want["keys"].reshape(-1).tolist(), name
        assert got["inter"] == want["inter"].tolist() and got["uni"] == want["uni"].tolist(), name
        assert got["parent"] == want["parent"].tolist() and got["first_of"] == want["first_of"].tolist(), name
        assert (got["n_dropped"], got["pairs_tested"], got["rounds"]) == (want["n_dropped"], want["pairs_tested"], want["rounds"]), name
        assert got["kept_docs"] == want["kept_docs"].tolist() and got["offs"] == want["offs"].tolist(), name
        assert got["rows"] == want["rows"].tolist() and got["counts"] == want["counts"].tolist(), name


def test_the_library_header_carries_the_same_forms():
    text = open(os.path.join(ROOT, "include", "isle_hip.h")).read()
    for name, value in (("ISLE_NEARDUP_KEY_AUTO", 0), ("ISLE_NEARDUP_KEY_FULL", 1), ("ISLE_NEARDUP_KEY_NARROW", 2)):
        assert "#define %s %d" % (name, value) in text
    host = open(os.path.join(ROOT, "isle_amd", "csrc", "neardup_host.h")).read()
    assert "ND_KEY_AUTO = 0, ND_KEY_FULL = 1, ND_KEY_NARROW = 2" in host
    assert "#include <hip" not in host and "isle_ctx*" not in host                    # plain C++
    route = open(os.path.join(ROOT, "isle_amd", "csrc", "route_host.h")).read()
    assert route.rstrip().endswith("inline NdKey route_neardup_key(int asked) { return asked == 2 ? ND_FORM_NARROW : ND_FORM_FULL; }")
