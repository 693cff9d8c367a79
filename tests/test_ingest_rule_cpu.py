"""The plain rule of tests/ingest_rule.py against the generator's own matrix, against the earlier split()-based checker where that one is
valid, and against the host parser (isle_amd/host/prestage.h through `prestage_dump --A`) on every text of the case table that the GPU
module runs, the two large ones excepted.  No GPU.  Agreement with the host parser means: the same accept or reject, the same kind, the
same line, and on acceptance a bit-equal A."""
import os
import re
import subprocess

import numpy as np
import pytest

from ingest_cases import CASES, PASSES, SMALL_TEXT, key_bits
from ingest_rule import COUNT_MAX, KINDS, csc_from_entries, ingest_rule, text_from_entries
from test_cli_cpu import write_tdf
from tools.synth import Corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "isle_amd", "host", "prestage_dump")


def split_ingest(text, V, D):
    """The checker test_gpu_ingest.py used to hold: valid on well-formed texts only (split() and int() accept more than the parsers do)."""
    trip = np.array([[int(x) for x in ln.split()] for ln in text.decode().replace("\r", "").split("\n") if ln.strip()], np.int64).reshape(-1, 3)
    doc, word, cnt = trip[:, 0] - 1, trip[:, 1] - 1, trip[:, 2]
    order = np.lexsort((np.arange(len(doc)), word, doc))
    doc, word, cnt = doc[order], word[order], cnt[order]
    first = np.ones(len(doc), bool)
    first[1:] = (doc[1:] != doc[:-1]) | (word[1:] != word[:-1])
    doc, word, cnt = doc[first], word[first], cnt[first]
    offs = np.zeros(D + 1, np.int64)
    np.add.at(offs, doc + 1, 1)
    return cnt.astype(np.float32), word.astype(np.uint32), np.cumsum(offs), len(trip)


def assert_same_A(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)


# ---------------------------------------------------------------- the rule itself
def test_rule_rounds_counts_to_float32_nearest_even():
    got = ingest_rule(b"1 1 16777217\n1 2 4294967295\n1 3 16777219\n1 4 4294967167\n1 5 16777216\n", 9, 1)
    assert got[0] == "ok"
    # 2^24 + 1 is a tie and goes down to the even 2^24, 2^24 + 3 is a tie and goes up to 2^24 + 4; 2^32 - 1 goes up to 2^32, and
    # 2^32 - 129 lies one below the tie between 2^32 - 256 and 2^32: down
    assert [float(x) for x in got[1]] == [16777216.0, 4294967296.0, 16777220.0, 4294967040.0, 16777216.0]
    assert got[1].dtype == np.float32 and got[2].dtype == np.uint32 and got[3].dtype == np.int64
    assert ingest_rule(b"1 1 %d\n" % (COUNT_MAX + 1), 9, 1) == ("error", 6, 1)


def test_rule_reads_exact_integers_whatever_their_length():
    z = b"0" * 40
    got = ingest_rule(z + b"1 " + z + b"2 " + z + b"3\n", 5, 5)
    assert got[0] == "ok" and list(got[1]) == [3.0] and list(got[2]) == [1] and list(got[3]) == [0, 1, 1, 1, 1, 1]
    assert ingest_rule(b"18446744073709551617 1 3\n", 5, 5) == ("error", 4, 1)   # 1 modulo 2^64
    assert ingest_rule(b"1 18446744073709551617 3\n", 5, 5) == ("error", 4, 1)
    assert ingest_rule(b"1 1 18446744073709551616\n", 5, 5) == ("error", 6, 1)   # 0 modulo 2^64: too large, not zero
    assert ingest_rule(b"1 1 " + z + b"\n", 5, 5) == ("error", 5, 1)


def test_rule_keeps_the_first_of_repeated_pairs_and_counts_empty_documents():
    text = b"3 2 5\n\n1 4 1\n3 2 9\r\n  \n3 1 2\n7 7 7\n1 4 8\n6 1 3"
    tag, counts, rows, offs, nread = ingest_rule(text, 8, 9)
    assert tag == "ok" and nread == 7
    assert list(counts) == [1.0, 2.0, 5.0, 3.0, 7.0] and list(rows) == [3, 0, 1, 0, 6]
    assert list(offs) == [0, 1, 1, 3, 3, 3, 4, 5, 5, 5]


def test_rule_separators_lines_and_the_order_of_checks():
    for empty in (b"", b"\n", b"\n \r\n\t\n", b"  \t"):
        got = ingest_rule(empty, 5, 5)
        assert got[0] == "ok" and got[4] == 0 and len(got[1]) == 0 and len(got[2]) == 0 and list(got[3]) == [0] * 6
    assert ingest_rule(b"1\r2 3 4", 20, 20)[2][0] == 2 and ingest_rule(b"1\r2 3 4", 20, 20)[3][12] == 1      # '\r' is no separator: doc 12
    for bad in (b"\v", b"\f", b"-", b"+", b".", b"\0", b"\x80", b"\xff", b"x"):
        assert ingest_rule(b"1 1 1\n\n1" + bad + b"1 1\n", 5, 5) == ("error", 1, 3), bad
    assert ingest_rule(b"1 2 3 4\n", 5, 5) == ("error", 2, 1)
    assert ingest_rule(b"1 2\n", 5, 5) == ("error", 3, 1) and ingest_rule(b"1 1 1\n2", 5, 5) == ("error", 3, 2)
    assert ingest_rule(b"1 2 x 3 4\n", 5, 5) == ("error", 1, 1) and ingest_rule(b"1 2 3 4 x\n", 5, 5) == ("error", 2, 1)
    assert ingest_rule(b"9 1 0\n", 5, 5) == ("error", 4, 1) and ingest_rule(b"1 1 0\n0 0 0\n", 5, 5) == ("error", 5, 1)
    assert ingest_rule(b"1 1 1\n6 1 1\n1 x\n", 5, 5) == ("error", 4, 2)                                       # the lowest bad line


def test_text_from_entries_writes_what_percent_d_writes():
    rng = np.random.default_rng(0)
    doc = np.concatenate([[1, 9, 10, 99, 100, 4294967280, 1000000000], rng.integers(1, 2 ** 32, size=200)])
    word = np.concatenate([[4294967280, 1, 10, 7, 999999999, 1, 65536], rng.integers(1, 70000, size=200)])
    cnt = np.concatenate([[4294967295, 16777217, 1, 10, 2, 3, 100], rng.integers(1, 500, size=200)])
    assert text_from_entries(doc, word, cnt) == b"".join(b"%d %d %d\n" % t for t in zip(doc, word, cnt))
    eol, sep = [b"\n", b"\r\n", b"\n\n"], [b" ", b"\t", b"  ", b" \t "]
    want = b"".join(b"%d%s%d%s%d%s" % (d, sep[i % 4], w, sep[i % 4], c, eol[i % 3]) for i, (d, w, c) in enumerate(zip(doc, word, cnt)))
    assert text_from_entries(doc, word, cnt, eol=eol, sep=sep) == want
    assert text_from_entries(doc[:0], word[:0], cnt[:0]) == b""


# ---------------------------------------------------------------- the rule against the generator and the earlier checker
def test_rule_equals_the_generators_matrix_and_the_split_checker(tmp_path):
    V, D = 400, 1500
    c = Corpus(V, D, 6, seed=8)
    counts, rows, offs = c.A()
    for style, shuffle in (("plain", None), ("messy", 3), ("plain", 5)):
        path = str(tmp_path / "c.tdf")
        n = write_tdf(path, counts, rows, offs, shuffle_seed=shuffle, style=style)
        text = open(path, "rb").read()
        got = ingest_rule(text, V, D)
        assert got[0] == "ok" and got[4] == n
        assert_same_A(got[1:4], (counts, rows, offs))
        old = split_ingest(text, V, D)
        assert_same_A(got[1:4], old[:3])
        assert got[4] == old[3]


# ---------------------------------------------------------------- the case table
def test_case_table_covers_what_it_names():
    assert [key_bits(V, D) for _, _, V, D, _, _ in PASSES] == [b for _, b, _, _, _, _ in PASSES]
    assert [(b + 7) // 8 for _, b, _, _, _, _ in PASSES] == [1, 2, 3, 4, 5, 6, 7, 8]
    for c in CASES:
        if not (c.large or c.long_text):
            assert len(c.build()[0]) < SMALL_TEXT, c.id


SMALL = [c for c in CASES if not c.large]


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_host_parser_agrees_with_the_rule(case, tmp_path):
    text, arrays = case.build()
    want = case.expected(text, arrays)
    if arrays is not None:   # the array form of the rule's last step, which the large cases rely on, gives the rule's matrix
        assert want[0] == "ok" and want[4] == len(arrays[0])
        assert_same_A(csc_from_entries(*arrays, case.D), want[1:4])
    tdf, out = str(tmp_path / "t.tdf"), str(tmp_path / "A.bin")
    open(tdf, "wb").write(text)
    nread = want[4] if want[0] == "ok" else 0
    r = subprocess.run([DUMP, "--A", tdf, str(case.V), str(case.D), str(nread), out], capture_output=True, text=True)
    if want[0] == "error":
        assert r.returncode == 1, "the host parser accepts what the rule rejects (kind %d, line %d): %s" % (want[1], want[2], r.stderr)
        assert re.search(re.escape("%s on line %d" % (KINDS[want[1]], want[2])) + r"\s*$", r.stderr), r.stderr
        return
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    V, D, nnz = (int(x) for x in np.frombuffer(raw, np.uint64, 3))
    assert (V, D, nnz) == (case.V, case.D, len(want[1])) and len(raw) == 24 + 12 * nnz + 8 * (D + 1)
    counts = np.frombuffer(raw, np.float32, nnz, 24)
    rows = np.frombuffer(raw, np.uint64, nnz, 24 + 4 * nnz)
    offs = np.frombuffer(raw, np.int64, D + 1, 24 + 12 * nnz)
    assert int(rows.max(initial=0)) < V
    assert_same_A((counts, rows.astype(np.uint32), offs), want[1:4])


def test_prestage_dump_long_form_reports_the_same_kinds(tmp_path):
    tdf = str(tmp_path / "t.tdf")
    open(tdf, "wb").write(b"1 1 2\n1 2\n")
    r = subprocess.run([DUMP, tdf, "5", "2", "1", "1", "0", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "fewer than three fields on line 2" in r.stderr
