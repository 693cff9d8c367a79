"""isle_amd/csrc/stage_host.h, the host rules of the stages either side of the hot path, without the library, without a GPU and without a
transport: stage_host_main is built here with the address and undefined-behaviour sanitizers (a stand-alone program) and answers a script
that this file sends on stdin.  A float crosses as its 32 bits, a double as its 64 bits, and every comparison is == on those bits.  Every
expected value is stated here (or in stages_certificate.py) in Python, from integers, sorts, sets and libm through the math module; nothing
here reads the header, so no case can pass by agreement of the code with itself."""
import json
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import stages_certificate as stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
M64 = (1 << 64) - 1
NAN64 = 0x7FF8000000000000  # std::nan("")


def f2b(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def d2b(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def fl(vals):
    """<n values> of floats, as bits"""
    return [len(vals)] + [f2b(v) for v in vals]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stage_host") / "stage_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "stage_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    """script: a list of token lists -> one dict per command"""
    text = "\n".join(" ".join(str(t) for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["cmd"] for o in out] == [line[0] for line in script]
    return out


# ---- the corpus average and its limit --------------------------------------------------------------------------------------------------------
def corpus(doc_sizes, first=None):
    """one entry per document of that many tokens (an empty document has none); first: the count of the first entry instead"""
    cnt = [s for s in doc_sizes if s]
    if first is not None:
        cnt[0] = first
    return np.array(cnt, F), np.concatenate([[0], np.cumsum([1 if s else 0 for s in doc_sizes])])


@pytest.mark.parametrize("cnt,offs", [
    corpus([3, 4, 5]), corpus([3, 0, 4, 4]), corpus([7]), corpus([1, 1, 9]),
    corpus([0, 0]),                # nz_docs = 0: divided by 1
    (np.zeros(0, F), np.array([0])),  # no document at all
    corpus([1, 1, 1], first=0),    # tokens = 2 < nz_docs = 3 (a zero count, which no ingest lets through): average 0
    corpus([65533]), corpus([65534]), corpus([65535, 65533]), corpus([65535, 65534, 65534]), corpus([2 ** 23, 1]),
])
def test_average_and_limit(exe, cnt, offs):
    avg, tokens, nz = stc.corpus_avg(cnt, offs)
    o = run(exe, [["avg", tokens, nz]])[0]
    assert o["avg"] == f2b(avg)
    assert o["ok"] == (int(avg) + 2 <= 65535)
    if o["ok"]:
        assert o["maxv"] == int(avg) + 2


def test_limit_boundary(exe):
    """avg = 65533 is the last average accepted"""
    a, b = run(exe, [["avg", 65533 * 4 + 3, 4], ["avg", 65534 * 4, 4]])
    assert (a["avg"], a["ok"], a["maxv"]) == (f2b(65533.0), True, 65535)
    assert (b["avg"], b["ok"]) == (f2b(65534.0), False)
    big = run(exe, [["maxv", f2b(3.0e9)], ["maxv", f2b(0.0)]])  # beyond 32 bits: refused, not wrapped
    assert not big[0]["ok"] and (big[1]["ok"], big[1]["maxv"]) == (True, 2)


# ---- count_gr, count_eq ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 30, 1000])
def test_threshold_counts(exe, k):
    nzs = [0, 1, 2 * k - 1, 2 * k, 2 * k + 1, 20 * k - 1, 20 * k, 20 * k + 1, 2 ** 24 + 1, 10 ** 7]
    nzs += [2 ** 25 + 2, 2 ** 24 + 5]  # as float32 2^25 and 2^24 + 4: at k = 1 count_gr loses one, count_eq stays on 838861
    for nz, o in zip(nzs, run(exe, [["counts", nz, k] for nz in nzs])):
        assert (o["gr"], o["eq"]) == stc.threshold_counts(nz, k), (nz, k)
    assert stc.threshold_counts(20 * k, k)[1] + 1 == stc.threshold_counts(20 * k + 1, k)[1]  # the step of count_eq is among the cases


# ---- the sampling key ------------------------------------------------------------------------------------------------------------------------
def key_py(seed, d, w):
    """splitmix64 of (seed, global document number) -> u in [0, 1) -> u^(1 / weight), in integers mod 2^64 and libm's pow"""
    z = (((seed + 1) * 0x9E3779B97F4A7C15) & M64) ^ ((d * 0xD1342543DE82EF95) & M64)
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    u = float(z >> 11) * (1.0 / 9007199254740992.0)
    return F(0.0) if w == 0 else F(math.pow(u, 1.0 / float(F(w))))


WEIGHTS = [0.0, 1.0, 95.0, 1900.0, 2.0 ** -3]
SEEDS = [0, 11, 2 ** 64 - 2]


@pytest.mark.parametrize("seed", SEEDS)
def test_sampling_key(exe, seed):
    docs = [0, 1, 2 ** 32, 2 ** 40 + 7]
    out = run(exe, [["keys", seed, d] + fl([w] * 2) for d in docs for w in WEIGHTS])
    want = [[f2b(key_py(seed, d, w)), f2b(key_py(seed, d + 1, w))] for d in docs for w in WEIGHTS]
    assert [o["keys"] for o in out] == want
    assert all(k == [0, 0] for k, (d, w) in zip(want, [(d, w) for d in docs for w in WEIGHTS]) if w == 0)
    ones = [k for k, w in zip(want, WEIGHTS * len(docs)) if w == 1.0]  # at weight 1 the key is u itself
    assert len({b for k in ones for b in k}) == len({d + i for d in docs for i in (0, 1)}), "the keys depend on the document"


@pytest.mark.parametrize("seed", SEEDS)
def test_a_shards_keys_are_that_slice_of_the_one_rank_keys(exe, seed):
    n = 23
    w = [WEIGHTS[i % 5] if i % 7 else 3.0 for i in range(n)]
    for base in (0, 2 ** 32 - 11):
        whole = run(exe, [["keys", seed, base] + fl(w)])[0]["keys"]
        assert whole == [f2b(key_py(seed, base + i, w[i])) for i in range(n)]
        for lo, hi in ((0, 0), (0, 9), (9, 10), (10, 23), (23, 23)):
            assert run(exe, [["keys", seed, base + lo] + fl(w[lo:hi])])[0]["keys"] == whole[lo:hi]


# ---- the pivot over all ranks and the drop mask ------------------------------------------------------------------------------------------------
# 1 - 2^-30 is a rate below 1 whose float32 is 1.0: the only way to nth = Dg, which the clamp takes back to Dg - 1 (0.999999 x Dg stays
# below Dg in float32 at every Dg)
RATES = [1e-9, 0.25, 0.5, 0.999999, 1.0 - 2.0 ** -30]


def keys_of(Dg):
    """half the keys 0, the rest drawn from seven values: whichever key is the pivot, a block of keys equals it"""
    rng = np.random.default_rng(Dg)
    vals = np.array([0.03125, 0.2, 0.4, 0.55, 0.7, 0.9, 0.99], F)
    k = np.where(np.arange(Dg) % 2 == 0, F(0), vals[rng.integers(0, 7, size=Dg)])
    return [F(v) for v in rng.permutation(k)]


def layouts(D):
    return [s for s in ([D], [0, D], [1, D - 1], [D, 0, 0]) if min(s) >= 0]


@pytest.mark.parametrize("Dg", [0, 1, 2, 1000])
def test_pivot_and_mask(exe, Dg):
    keys = keys_of(Dg)
    nths = set()
    for rate in RATES:
        if Dg:
            nth = min(int(F(rate) * F(Dg)), Dg - 1)  # float32 product
            nths.add(nth)
            pivot = sorted(keys, reverse=True)[nth]
        else:
            pivot = F(2.0)
        mask = [int(not (k >= pivot)) for k in keys]
        assert not any(m for k, m in zip(keys, mask) if k == pivot), "equal keys are kept"
        if Dg == 1000:
            assert sum(k == pivot for k in keys) > 1 and sum(mask) < Dg
        for sizes in layouts(Dg):
            cuts = np.concatenate([[0], np.cumsum(sizes)])
            shards = [keys[cuts[r]:cuts[r + 1]] for r in range(len(sizes))]
            dmax = max(sizes)
            padded = [list(s) + [F(-1.0)] * (max(dmax, 1) - len(s)) for s in shards]
            script = [["pad", dmax] + fl(s) for s in shards]
            script.append(["pivot", d2b(rate)] + fl([v for p in padded for v in p]))
            script += [["mask", f2b(pivot)] + fl(s) for s in shards]
            out = run(exe, script)
            R = len(sizes)
            assert [o["keys"] for o in out[:R]] == [[f2b(v) for v in p] for p in padded]
            assert out[R]["pivot"] == f2b(pivot), (rate, sizes)
            for r, o in enumerate(out[R + 1:]):
                assert o["n"] == sizes[r] and o["slots"] == max(sizes[r], 1)
                assert o["drop"][:sizes[r]] == mask[cuts[r]:cuts[r + 1]], (rate, sizes, r)
    if Dg == 1000:
        assert {0, Dg - 1} <= nths
        assert int(F(RATES[-1]) * F(Dg)) == Dg and int(F(0.999999) * F(Dg)) == Dg - 1


def test_pivot_of_distinct_keys(exe):
    """no padding, every key its own value: the pivot tells nth = 250 from 251 (0.251 x 1000 in float32 and in double)"""
    keys = [F(v) for v in np.random.default_rng(3).permutation(np.arange(1, 1001) / 1001.0)]
    assert int(F(0.251) * F(1000)) == 250 and int(0.251 * 1000) == 251
    for rate in RATES + [0.251]:
        o = run(exe, [["pivot", d2b(rate)] + fl(keys)])[0]
        assert o["pivot"] == f2b(sorted(keys, reverse=True)[min(int(F(rate) * F(1000)), 999)])


# ---- a shard's place in B's columns --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", [[5], [0, 5], [5, 0], [0, 0, 0], [3, 0, 4, 1]])
def test_placement(exe, kept):
    out = run(exe, [["place", r, len(kept)] + kept for r in range(len(kept))])
    assert [(o["b_off"], o["b_glob"]) for o in out] == [(sum(kept[:r]), sum(kept)) for r in range(len(kept))]


# ---- UMass coherence: the plan and the sums ------------------------------------------------------------------------------------------------------
def coherence_py(topics, vocab, eps, zero_word=None, seed=0):
    """-> (script line, expected answer): sets and sorts for the plan, the reference's loop order and math.log for the sums"""
    T, M = len(topics), len(topics[0])
    U = sorted({w for t in topics for w in t})
    loc = [[U.index(w) for w in t] for t in topics]
    pair = lambda a, b: (min(a, b), max(a, b))  # noqa: E731
    keys = [pair(l[i], l[j]) for l in loc for i in range(1, M) for j in range(i)]
    P = sorted(set(keys))
    part_off = [sum(1 for lo, _ in P if lo < u) for u in range(len(U) + 1)]
    rng = np.random.default_rng(seed)
    du = [0 if U[u] == zero_word else int(v) for u, v in enumerate(rng.integers(1, 60, size=len(U)))]
    dp = [int(rng.integers(0, min(du[lo], du[hi]) + 1)) for lo, hi in P]
    coh, df, cdf = [], [], []
    for l in loc:
        s, undefined = 0.0, False
        for i in range(1, M):
            for j in range(i):
                dij, dj = dp[P.index(pair(l[i], l[j]))], du[l[j]]
                cdf.append(dij)
                if dj == 0:
                    undefined = True  # log(0) = -inf there, an error here: the topic is NaN either way
                else:
                    s += math.log(float(dij) + eps) - math.log(float(dj))
        coh.append(NAN64 if undefined else d2b(s))
        df += [du[u] for u in l]
    line = ["coh", T, M, vocab] + [w for t in topics for w in t] + [d2b(eps), len(du) + len(dp)] + du + dp
    want = dict(U=U, loc=[u for l in loc for u in l], keys=[lo << 32 | hi for lo, hi in keys], P=[lo << 32 | hi for lo, hi in P],
                part_off=part_off, part_hi=[hi for _, hi in P], coherence=coh, doc_freq=df, co_doc_freq=cdf)
    return line, want


def check_coherence(exe, topics, vocab, eps=1.0, **kw):
    line, want = coherence_py(topics, vocab, eps, **kw)
    o = run(exe, [line])[0]
    assert o.pop("same_without_outputs") and o.pop("cmd") == "coh"
    assert o == want
    return want


def test_coherence_one_word_per_topic_has_no_pairs(exe):
    w = check_coherence(exe, [[4], [9], [4]], 10)
    assert w["coherence"] == [d2b(0.0)] * 3 and w["P"] == [] and w["part_off"] == [0, 0, 0] and w["co_doc_freq"] == []


@pytest.mark.parametrize("eps", [1.0, 1e-12])
def test_coherence_32_words(exe, eps):
    rng = np.random.default_rng(5)
    w = check_coherence(exe, [[int(v) for v in rng.permutation(5000)[:32]]], 5000, eps)
    assert len(w["P"]) == 32 * 31 // 2 and w["part_off"][-1] == len(w["P"])


def test_coherence_one_topic(exe):
    check_coherence(exe, [[7, 2, 11, 3]], 12)


def test_coherence_topics_sharing_words_and_a_pair(exe):
    w = check_coherence(exe, [[5, 9, 2], [9, 5, 7], [1, 0, 8]], 10)
    assert len(w["U"]) == 7 and len(w["keys"]) == 9 and len(w["P"]) == 8  # (5, 9) is counted once and read by two topics


def test_coherence_undefined_for_the_topic_with_an_absent_word_only(exe):
    w = check_coherence(exe, [[5, 9, 2], [9, 6, 7], [5, 2, 8]], 10, zero_word=6)
    assert [c == NAN64 for c in w["coherence"]] == [False, True, False]
    w = check_coherence(exe, [[5, 9, 2], [9, 7, 6]], 10, zero_word=6)  # as the last word it is never a dj
    assert NAN64 not in w["coherence"]


def test_coherence_refusals(exe):
    def refused(topics, vocab):
        return run(exe, [["coh", len(topics), len(topics[0]), vocab] + [w for t in topics for w in t] + [d2b(1.0), 0]])[0]
    assert refused([[1, 2, 3], [4, 12, 5]], 12) == dict(cmd="coh", refused="topic_coherence: word 12 of topic 1 >= vocab 12")
    assert refused([[1, 2, 3], [4, 11, 5]], 12).get("refused") is None
    assert refused([[3, 2, 3], [4, 11, 5]], 12) == dict(cmd="coh", refused="topic_coherence: word 3 repeats in topic 0")
    assert refused([[1, 2, 3], [4, 5, 5]], 12) == dict(cmd="coh", refused="topic_coherence: word 5 repeats in topic 1")
    assert refused([[1, 2, 3], [3, 2, 1]], 12).get("refused") is None  # across topics a word may repeat


# ---- the top-five count rule, the diversity average, the line of a byte -----------------------------------------------------------------------
def top_five_literal(runs, m):
    """The reference's loop (src/sparseMatrix.cpp:198-208) over sorted tuples, run r being runs[r] copies of r"""
    q = [r for r, n in enumerate(runs) for _ in range(n)]
    num = it = prev = 0
    while it != len(q):
        if q[it] != q[prev] and it - prev >= m:
            prev = it
            num += 1
        it += 1
    return num


@pytest.mark.parametrize("runs,m", [([], 2), ([5], 5), ([5], 2), ([1] * 9, 2), ([1] * 9, 3), ([5, 1], 5), ([4, 1], 5), ([2, 7, 1, 1, 3, 6, 1], 3),
                                    ([1, 1, 1, 1, 6, 1, 1], 5), ([3, 3, 3, 1], 3)])
def test_top_five_count(exe, runs, m):
    assert run(exe, [["top5", m, len(runs)] + runs])[0]["num"] == top_five_literal(runs, m)


def test_top_five_count_known(exe):
    assert top_five_literal([5, 1], 5) == 1 and top_five_literal([4, 1], 5) == 0 and top_five_literal([1] * 9, 2) == 4


@pytest.mark.parametrize("dist,kp", [([0.5, 0.25, 0.125], 3), ([0.1, 0.2, 0.3], 3), ([0.1, math.inf, 0.3, math.nan], 2), ([math.inf], 0), ([], 0),
                                     ([1e300, 1e300, -math.inf], 2)])
def test_diversity_average(exe, dist, kp):
    s = 0.0
    for v in dist:
        if math.isfinite(v):
            s += v
    want = d2b(s / float(kp)) if kp else NAN64
    assert run(exe, [["div", kp, len(dist)] + [d2b(v) for v in dist]])[0]["avg"] == want


@pytest.mark.parametrize("text", [b"", b"a", b"\n", b"ab\ncd\n", b"ab\ncd", b"\n\n\nx"])
def test_line_of_byte(exe, text):
    n = len(text)
    script = [["line", pos, text.hex() or "-"] for pos in list(range(n + 1)) + [n + 5]]
    for (_, pos, _), o in zip(script, run(exe, script)):
        upto = min(pos, n - 1 if n else 0)  # a position at the end of the text belongs to the last byte's line
        assert o["line"] == 1 + text[:upto].count(b"\n"), (text, pos)
