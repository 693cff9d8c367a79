"""The host rules of the distributed radix select (isle_amd/csrc/stage_host.h select_digit, select_mask, select_chunks / select_chunk;
route_host.h route_post_select) without the library and without a GPU: isle_amd/host/post_select_main.cpp is built here with the address
and undefined-behaviour sanitizers (a stand-alone program) and answers a script sent on stdin.  A float crosses as its 32 bits.  Every
expected value is stated here from sorting; nothing here reads the headers."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("post_select") / "post_select_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "post_select_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    text = "\n".join(" ".join(str(int(t)) if not isinstance(t, str) else t for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["cmd"] for o in out] == [line[0] for line in script]
    return out


def pick_by_sorting(bins, remaining):
    """the digit of the remaining-th largest of a multiset holding bins[d] copies of d, and its rank among the copies of that digit"""
    digits = np.repeat(np.arange(256), bins)[::-1]  # descending
    assert 1 <= remaining <= len(digits)
    d = int(digits[remaining - 1])
    return d, remaining - int((digits > d).sum())


def test_digit_pick_against_sorting(exe):
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(40):
        bins = rng.integers(0, 6, 256) * (rng.random(256) < rng.choice([0.02, 0.3, 1.0]))
        if bins.sum() == 0:
            bins[rng.integers(256)] = 1
        for rem in {1, int(bins.sum()), int(rng.integers(1, bins.sum() + 1))}:
            cases.append((bins.astype(np.int64), rem))
    one = lambda d, n: np.bincount([d], minlength=256) * n  # noqa: E731
    cases += [(one(0, 7), 1), (one(0, 7), 7), (one(255, 7), 1), (one(255, 7), 7)]
    # remaining equal to a cumulative count exactly: the last copy of a digit, and one past it the first copy of the next digit below
    steps = np.zeros(256, np.int64)
    steps[[250, 200, 3, 0]] = [4, 1, 5, 2]
    cases += [(steps, rem) for rem in (4, 5, 6, 10, 11, 12)]
    out = run(exe, [["pick", rem, 256] + list(bins) for bins, rem in cases])
    for (bins, rem), o in zip(cases, out):
        assert (o["digit"], o["remaining"]) == pick_by_sorting(bins, rem), (np.flatnonzero(bins), rem)
    big = run(exe, [["pick", 2 ** 32 - 1, 256] + list(one(0, 2 ** 32 - 1)), ["pick", 2 ** 32 - 1, 256] + list(one(255, 2 ** 32 - 1))])  # no overflow at the top
    assert [(o["digit"], o["remaining"]) for o in big] == [(0, 2 ** 32 - 1), (255, 2 ** 32 - 1)]
    assert [pick_by_sorting(steps, rem) for rem in (4, 5, 6, 10, 11, 12)] == [(250, 4), (200, 1), (3, 1), (3, 5), (0, 1), (0, 2)]


def _segments():
    rng = np.random.default_rng(9)
    segs = {
        "uniform": rng.random(300, dtype=F) + F(0.01),
        "equal": np.full(257, 0.5, F),
        "top16": (F(30000) / (F(60000) + (np.arange(257) * 37 % 101).astype(F))).astype(F),  # share sign, exponent and seven mantissa bits
        "wide": np.exp(rng.uniform(-80, 80, 256)).astype(F),                                # every exponent byte
        "two": np.array([1.5, 1.5000001], F),
        "tiny": np.array([1e-45, 2e-45, 1e-38, 1.0, 3e38], F),                              # denormals and the largest exponents
    }
    assert all((v > 0).all() for v in segs.values())
    return segs


@pytest.mark.parametrize("name", sorted(_segments()))
def test_four_passes_over_split_segments_against_sorting(exe, name):
    """the segment cut into 1 .. 4 parts at several places, empty parts included: the value is sorted(...)[r - 1] from the largest"""
    v = _segments()[name]
    n = len(v)
    bits = v.view(np.uint32)
    desc = np.sort(v)[::-1]
    rng = np.random.default_rng(len(name))
    splits = [[n], [n // 2, n - n // 2], [0, n], [1, n - 1], [n - 1, 0, 1], [n // 3, 0, n // 3, n - 2 * (n // 3)]]
    perm = rng.permutation(n)
    ranks = sorted({1, 2, n // 2, n - 1, n} - {0})
    script, want = [], []
    for sp in splits:
        assert sum(sp) == n
        parts = np.split(bits[perm], np.cumsum(sp)[:-1])
        for r in ranks:
            script.append(["select", r, len(parts)] + [t for p in parts for t in [len(p)] + list(p)])
            want.append(int(desc[r - 1:r].view(np.uint32)[0]))
    out = run(exe, script)
    assert [o["value"] for o in out] == want
    assert all(o["remaining"] >= 1 for o in out)


@pytest.mark.parametrize("chunk", [1, 7, 65536])
def test_chunk_plan_tiles_the_slots(exe, chunk):
    counts = sorted({0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk, 3 * chunk + 1} - {-1})
    out = run(exe, [["chunks", n, chunk] for n in counts])
    for n, o in zip(counts, out):
        ch = o["chunks"]
        assert o["n"] == len(ch) == -(-n // chunk)
        at = 0
        for first, count in ch:
            assert first == at and 1 <= count <= chunk
            at += count
        assert at == n
        assert all(count == chunk for _, count in ch[:-1])


def test_plan_constants_and_form(exe):
    """64 MiB of bins per all-reduce to begin with: 65 536 slots of 256 counters of four bytes; the histogram form with more than one rank"""
    out = run(exe, [["plan"]] + [["form", w] for w in (0, 1, 2, 8)])
    assert out[0]["bins_bytes"] == 64 << 20 and out[0]["chunk_slots"] == (64 << 20) // 1024 == 65536
    assert [o["histogram"] for o in out[1:]] == [0, 0, 1, 1]
