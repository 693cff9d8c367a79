"""The plain rules of tests/tdf_shard_rule.py (line ownership of a byte range, lines per document, bounds from counts, the window cut)
held to themselves and to the library's host rule, without a GPU: the ownership rule on every cut of small texts and on random ones;
plan_bound of isle_amd/csrc/stage_host.h, through a stand-alone program built here with the address and undefined-behaviour sanitizers,
against HotPath.plan_shards and the plain rule; and the certificates of the GPU tests fed arrays made by wrong rules, which they must
refuse."""
import os
import subprocess

import numpy as np
import pytest

import shard_cases as sc
import tdf_shard_rule as tr
from ingest_rule import ingest_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [b"", b"\n", b"1 1 1", b"1 1 1\n", b"\n\n\n", b"1 2 3\r\n\r\n 2  1\t7 \r\n12 10 345\n3 3 9", b"a\nbb\n\nccc", b"x" * 30, b"x" * 30 + b"\n"]


def restated_owned(text, b, e):
    """The rule as the pump walks it: with b > 0 and text[b - 1] != '\\n' skip through the first '\\n' at or after b (none: nothing); stop
    after the first '\\n' at a position >= e - 1, or at the end; b >= e owns nothing."""
    if b >= e:
        return b""
    s = b
    if b > 0 and text[b - 1:b] != b"\n":
        nl = text.find(b"\n", b)
        if nl < 0:
            return b""
        s = nl + 1
    if s >= e:
        return b""
    nl = text.find(b"\n", max(e - 1, s))
    return text[s:] if nl < 0 else text[s:nl + 1]


@pytest.mark.parametrize("text", SMALL)
def test_ownership_on_every_cut_of_small_texts(text):
    n = len(text)
    starts = [s for s, _ in tr.lines_with_starts(text)]
    for b in range(n + 2):
        for e in range(n + 2):
            assert tr.owned(text, b, e) == restated_owned(text, b, e), (b, e)
    for parts in range(1, n + 3):
        pieces = [tr.owned(text, *tr.rank_range(n, r, parts)) for r in range(parts)]
        assert b"".join(pieces) == text
        owners = [sum(1 for r in range(parts) if tr.rank_range(n, r, parts)[0] <= s < tr.rank_range(n, r, parts)[1]) for s in starts]
        assert all(o == 1 for o in owners)


def test_ownership_on_random_texts():
    rng = np.random.default_rng(12)
    for _ in range(300):
        n = int(rng.integers(0, 60))
        text = bytes(rng.choice(np.frombuffer(b"\n\n\r 123", np.uint8), size=n).tolist())
        parts = int(rng.integers(1, 9))
        assert b"".join(tr.owned(text, *tr.rank_range(n, r, parts)) for r in range(parts)) == text
        b, e = sorted(int(x) for x in rng.integers(0, n + 2, 2))
        assert tr.owned(text, b, e) == restated_owned(text, b, e)


# ---- plan_bound ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan_bound") / "plan_bound_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "plan_bound_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def plan_inputs():
    rng = np.random.default_rng(21)
    heavy = rng.integers(0, 5, 200)
    heavy[77] = 100000
    return {"random": rng.integers(0, 300, 500), "all-zero": np.zeros(37, np.int64), "parts-above-D": np.array([3, 1, 4]), "one-document": np.array([9]),
            "one-heavy-document": heavy, "trailing-empty": np.concatenate([rng.integers(1, 50, 40), np.zeros(60, np.int64)]),
            "leading-empty": np.concatenate([np.zeros(60, np.int64), rng.integers(1, 50, 40)]), "large-weights": rng.integers(2 ** 40, 2 ** 41, 64),
            "no-document": np.zeros(0, np.int64)}


def test_plan_bound_is_plan_shards_and_the_plain_rule(exe):
    from isle_amd import HotPath
    jobs = [(name, parts, w) for name, w in plan_inputs().items() for parts in (1, 2, 3, 8, 64)]
    script = "".join("%d %d %s\n" % (parts, len(w), " ".join(str(int(x)) for x in w)) for _, parts, w in jobs)
    r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(jobs)
    for (name, parts, w), line in zip(jobs, lines):
        got = np.array([int(x) for x in line.split()], np.int64)
        offs = np.concatenate([[0], np.cumsum(np.asarray(w, np.int64))]).astype(np.int64)
        assert np.array_equal(got, tr.bounds_from_counts(w, parts)), (name, parts, got)
        assert np.array_equal(got, HotPath.plan_shards(offs, parts).astype(np.int64)), (name, parts, got)
        assert np.array_equal(got, sc.plan_shards_py(offs, parts)), (name, parts, got)


# ---- the certificates refuse arrays made by a wrong rule ----------------------------------------------------------------------------------
CERT_CASES = ("spread-4", "trailing-empty-documents-3", "repeated-pair-across-ranges-2", "long-line-leading-zeros-3")


@pytest.mark.parametrize("case", list(tr.SHARDED))
def test_the_certificate_takes_the_rules_own_arrays(case):
    n, V, D, text = tr.SHARDED[case]
    res = ingest_rule(text, V, D)
    b = tr.certify_sharded(tr.reference_ranks(text, V, D, n), text, V, D, single=(res[1], res[2], res[3]))
    assert b[0] == 0 and b[-1] == D and np.all(np.diff(b) >= 0)


def test_a_window_cut_one_document_late_is_refused():
    n, V, D, text = tr.SHARDED["spread-4"]
    with pytest.raises(AssertionError):
        tr.certify_sharded(tr.reference_ranks(text, V, D, n, window_shift=1), text, V, D)
    res = ingest_rule(text, V, D)
    cnt, rows, offs = tr.window_cut(res, 11, 21)
    with pytest.raises(AssertionError):
        tr.certify_window(dict(cnt=cnt, rows=rows, offs=offs, entries_read=res[4], nnz=len(cnt)), res, 10, 20, D)
    cnt, rows, offs = tr.window_cut(res, 10, 20)
    with pytest.raises(AssertionError, match="offsets"):       # a cut whose offsets keep the whole matrix's numbering
        tr.certify_window(dict(cnt=cnt, rows=rows, offs=res[3][10:21], entries_read=res[4], nnz=len(cnt)), res, 10, 20, D)
    with pytest.raises(AssertionError, match="entries_read"):  # entries_read of the window, not of the text
        tr.certify_window(dict(cnt=cnt, rows=rows, offs=offs, entries_read=len(cnt), nnz=len(cnt)), res, 10, 20, D)


def test_bounds_from_counts_that_were_not_summed_are_refused():
    n, V, D, text = tr.SHARDED["spread-4"]
    with pytest.raises(AssertionError, match="bounds"):
        tr.certify_sharded(tr.reference_ranks(text, V, D, n, summed=False), text, V, D)


def test_a_line_counted_by_two_ranges_is_refused():
    n, V, D, text = tr.SHARDED["spread-4"]
    with pytest.raises(AssertionError):
        tr.certify_sharded(tr.reference_ranks(text, V, D, n, overlap=True), text, V, D)
    total = tr.doc_line_counts(text, V, D)
    twice = total.copy()
    twice[5] += 1
    with pytest.raises(AssertionError, match="doc_lines"):
        tr.certify_counts(dict(doc_lines=twice, lines_local=int(twice.sum()), lines_global=int(twice.sum()), bounds={}), text, V, D, ())


def test_the_counts_rule_on_a_text_with_blank_and_bad_lines():
    text = b"2 1 1\n\n2 x 1\n2 2 1\r\n9 9 9\n3 1 1\n2 1 5"
    assert tr.doc_line_counts(text, 5, 4).tolist() == [0, 3, 1, 0]            # the repeated pair (2, 1) counts twice; 9 9 9 is out of range
    assert tr.bounds_from_counts([0, 3, 1, 0], 2).tolist() == [0, 2, 4] and tr.bounds_from_counts([0, 0, 0], 4).tolist() == [0, 0, 0, 0, 3]
