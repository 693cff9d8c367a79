"""The tdf text stream (isle_hip_tdf_begin / _acquire / _commit / _write / _finalize, HotPath.tdf_* and ingest_tdf_file) against the plain
rule of tests/ingest_rule.py on the whole text, whatever the cuts: every cut of small texts, the case table of tests/ingest_cases.py at
piece sizes from 1 byte to 4097, the error-order texts and the million-line text over many pieces, the library's own piece size through
both of its buffers more than once, the states of a stream, isle_amd/host/tdf_stream_main as a real process, and a whole-text ingest
between the parts of an open stream or feed, which share its kernels but none of its buffers.  Every comparison is exact:
counts, rows, offsets, entries_read, nnz; an error by its kind's wording and its 1-based line in the whole text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from feed_rule import BASE_D, BASE_V, base_corpus, feed_rule
from ingest_cases import CASES
from ingest_rule import KINDS, ingest_rule, text_from_entries
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "tdf_stream_main")

SEED_TEXT = b"3 2 8\n1 1 5\n"                       # the matrix a failed stream must leave as it was
NO_STREAM = "no open text stream"


def assert_exact(hp, info, want):
    _, counts, rows, offs, entries_read = want
    assert info["entries_read"] == entries_read and info["nnz"] == len(counts)
    gc, gr, go = hp.get_A()
    np.testing.assert_array_equal(go, offs)
    np.testing.assert_array_equal(gr, rows)
    np.testing.assert_array_equal(gc, counts)


def stream(hp, parts, V, D, piece=0, max_entries=0):
    hp.tdf_begin(V, D, _piece_bytes=piece)
    for part in parts:
        hp.tdf_write(part)
    return hp.tdf_finalize(max_entries)


def assert_stream_rejected(hp, parts, V, D, piece, kind, line):
    """The first bad line of the whole text, from whichever call learns of it; the matrix held before stays, the stream is gone."""
    hp.ingest_tdf(SEED_TEXT, 4, 3)
    before = hp.get_A()
    with pytest.raises(IsleHipError, match=re.escape("%s on line %d" % (KINDS[kind], line)) + r"\b"):
        stream(hp, parts, V, D, piece)
    for got, want in zip(hp.get_A(), before):
        np.testing.assert_array_equal(got, want)
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_finalize()


def check(hp, parts, V, D, piece, want):
    if want[0] == "error":
        assert_stream_rejected(hp, parts, V, D, piece, want[1], want[2])
    else:
        assert_exact(hp, stream(hp, parts, V, D, piece, max_entries=want[4]), want)


# ---------------------------------------------------------------- 1. every cut of small texts
SMALL = [
    b"1 2 3\r\n\r\n 2  1\t7 \r\n12 10 345\n3 3 9",              # '\r\n', a blank line, blanks around, multi-digit fields, no last newline
    b"\n\n  \t\n4 4 4\n4 4 5\n  1 1 1  \n\r\n2 12 4294967295",
    b"1 1 1\n2 2 x\n3 3\n",                                       # two bad lines: the first one, wherever the cut falls
    b"12 12 12",
]


@pytest.mark.parametrize("text", SMALL, ids=["crlf-blank-padded", "blanks-first-repeat", "two-bad-lines", "one-line-no-newline"])
def test_every_single_cut_and_every_byte_alone(hp, text):
    assert len(text) <= 64
    want = ingest_rule(text, 12, 12)
    for cut in range(len(text) + 1):
        check(hp, [text[:cut], text[cut:]], 12, 12, 64, want)
    check(hp, [text[i:i + 1] for i in range(len(text))], 12, 12, 64, want)


# ---------------------------------------------------------------- 2. the case table
TABLE = [c for c in CASES if not c.large and not c.long_text]


def _pieces_of(case):
    return (4097, 1000, 1, 7, 16) if len(case.build()[0]) <= 512 else (4097, 1000)


@pytest.mark.parametrize("case,piece", [(c, p) for c in TABLE for p in _pieces_of(c)], ids=["%s-piece%d" % (c.id, p) for c in TABLE for p in _pieces_of(c)])
def test_the_case_table_in_pieces(hp, case, piece):
    text, arrays = case.build()
    want = case.expected(text, arrays)
    check(hp, [text], case.V, case.D, piece, want)
    if not len(text.strip()):
        assert hp.get_A()[2].shape == (case.D + 1,) and not hp.get_A()[2].any()


# ---------------------------------------------------------------- 3. the first of several bad lines, pieces apart
LONG = [c for c in CASES if c.long_text]


@pytest.mark.parametrize("case", LONG, ids=[c.id for c in LONG])
def test_the_first_bad_line_wins_over_pieces(hp, case):
    text, arrays = case.build()
    assert len(LONG) == 4 and len(text) == 420000
    want = case.expected(text, arrays)
    assert want[0] == "error" and want[2] == (69300 if "late-blocks" in case.id else 3)
    assert_stream_rejected(hp, [text], case.V, case.D, 65536, want[1], want[2])


# ---------------------------------------------------------------- 4. a million lines: the line base over pieces
def test_a_million_lines_in_pieces_of_a_mebibyte(hp):
    case = next(c for c in CASES if c.id == "lines-million")
    text, arrays = case.build()
    assert_exact(hp, stream(hp, [text], case.V, case.D, 1 << 20), case.expected(text, arrays))


# ---------------------------------------------------------------- 5. the library's own piece size: both buffers more than once
def own_piece_size(hp):
    hp.tdf_begin(1, 1)
    buf, cap = C.c_void_p(), C.c_uint64()
    hp._chk(hp._lib.isle_hip_tdf_acquire(hp._h, C.byref(buf), C.byref(cap)))
    hp._chk(hp._lib.isle_hip_tdf_commit(hp._h, 0))
    hp.tdf_finalize()
    return int(cap.value)


def test_own_piece_size_one_write_and_from_a_file(hp, tmp_path):
    piece = own_piece_size(hp)
    V, D = 3000, 5000
    n = (3 * piece + piece // 3) // 11                  # a line is at least "dddd www c\n": more than three pieces and a ragged tail
    j = np.arange(n, dtype=np.int64)
    pair = (j * 7919) % (V * D)
    text = text_from_entries(pair // V + 1, pair % V + 1, j % 1000 + 1, eol=[b"\n", b"\r\n", b"\n\n"], sep=[b" ", b"\t"])
    assert 3 * piece < len(text) and len(text) % piece
    info = hp.ingest_tdf(text, V, D)
    want = hp.get_A()
    path = tmp_path / "own.tdf"
    path.write_bytes(text)
    for run in (lambda: stream(hp, [text], V, D), lambda: hp.ingest_tdf_file(str(path), V, D)):
        assert run() == info
        for got, ref in zip(hp.get_A(), want):
            np.testing.assert_array_equal(got, ref)
        hp.ingest_tdf(SEED_TEXT, 4, 3)                  # (so that the second comparison cannot pass on the first one's matrix)


# ---------------------------------------------------------------- 6. states
GOOD = b"2 3 4\n1 1 9\n2 3 5\n\n4 4 1"


def close_any_stream(hp):
    hp.tdf_begin(1, 1)
    hp.tdf_finalize()


def test_no_stream_open_is_refused(hp):
    close_any_stream(hp)
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_write(b"1 1 1\n")
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_finalize()


def test_a_text_stream_and_a_feed_exclude_each_other(hp):
    hp.tdf_begin(5, 5)
    with pytest.raises(IsleHipError, match="no open feed"):
        hp.feed([0], [0], [1])
    with pytest.raises(IsleHipError, match="no open feed"):
        hp.feed_finalize()
    hp.tdf_write(GOOD)
    assert_exact(hp, hp.tdf_finalize(), ingest_rule(GOOD, 5, 5))        # the refusals took nothing from the stream
    hp.feed_begin(5, 5)
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_write(GOOD)
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_finalize()
    hp.feed([4], [4], [7])
    assert hp.feed_finalize() == (1, 1)


def test_begin_discards_what_is_open(hp):
    hp.feed_begin(5, 5)
    hp.feed([0, 1], [0, 1], [9, 9])
    hp.tdf_begin(5, 5)                                  # the feed's two entries are gone
    hp.tdf_write(GOOD)
    assert_exact(hp, hp.tdf_finalize(), ingest_rule(GOOD, 5, 5))
    hp.tdf_begin(5, 5)
    hp.tdf_write(b"5 5 5\n")
    hp.tdf_begin(5, 5)                                  # ... and so is an open stream's line
    hp.tdf_write(bytearray(GOOD[:5]))
    hp.tdf_write(memoryview(GOOD)[5:9])
    hp.tdf_write(np.frombuffer(GOOD[9:], np.uint8))
    assert_exact(hp, hp.tdf_finalize(), ingest_rule(GOOD, 5, 5))
    hp.tdf_begin(5, 5)
    hp.feed_begin(5, 5)                                 # feed_begin discards an open stream
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_finalize()
    hp.feed_finalize()


def test_one_buffer_at_a_time(hp):
    lib, h = hp._lib, hp._h
    buf, cap, buf2, cap2 = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    hp.tdf_begin(5, 5, _piece_bytes=8)
    assert lib.isle_hip_tdf_commit(h, 0) != 0 and b"no buffer acquired" in lib.isle_hip_last_error(h)
    assert lib.isle_hip_tdf_acquire(h, C.byref(buf), C.byref(cap)) == 0 and cap.value == 8 and buf.value
    assert lib.isle_hip_tdf_acquire(h, C.byref(buf2), C.byref(cap2)) != 0
    assert lib.isle_hip_tdf_commit(h, 9) != 0 and b"9 bytes in a buffer of 8" in lib.isle_hip_last_error(h)
    C.memmove(buf.value, b"2 3 4\n1 ", 8)               # the refusals left the buffer with the caller
    assert lib.isle_hip_tdf_commit(h, 8) == 0
    assert lib.isle_hip_tdf_commit(h, 0) != 0
    assert lib.isle_hip_tdf_acquire(h, C.byref(buf2), C.byref(cap2)) == 0 and buf2.value != buf.value
    assert lib.isle_hip_tdf_commit(h, 0) == 0           # given back empty
    hp.tdf_write(GOOD[8:])
    assert_exact(hp, hp.tdf_finalize(), ingest_rule(GOOD, 5, 5))
    own = own_piece_size(hp)
    hp.tdf_begin(5, 5, _piece_bytes=own + 1)            # more than the library's own: its own
    assert lib.isle_hip_tdf_acquire(h, C.byref(buf), C.byref(cap)) == 0 and cap.value == own
    close_any_stream(hp)


def test_a_failed_stream_leaves_the_matrix_and_the_next_one_is_exact(hp):
    assert_stream_rejected(hp, [b"1 1 1\n2 2 0\n", GOOD], 5, 5, 4, 5, 2)
    assert_exact(hp, stream(hp, [GOOD], 5, 5, 4, max_entries=4), ingest_rule(GOOD, 5, 5))


def test_max_entries_is_checked_at_finalize_with_the_whole_text_wording(hp):
    hp.ingest_tdf(SEED_TEXT, 4, 3)
    before = hp.get_A()
    hp.tdf_begin(5, 5, _piece_bytes=7)
    hp.tdf_write(GOOD)
    with pytest.raises(IsleHipError, match=re.escape("file has 4 entries, <max_entries> says 5")):
        hp.tdf_finalize(max_entries=5)
    for got, want in zip(hp.get_A(), before):
        np.testing.assert_array_equal(got, want)
    with pytest.raises(IsleHipError, match=NO_STREAM):
        hp.tdf_finalize()


def test_a_missing_file_opens_no_stream_and_other_dtypes_are_refused(hp, tmp_path):
    close_any_stream(hp)
    hp.feed_begin(5, 5)
    with pytest.raises(OSError):
        hp.ingest_tdf_file(str(tmp_path / "none.tdf"), 5, 5)
    hp.feed([4], [4], [7])                              # the feed that was open still is
    assert hp.feed_finalize() == (1, 1)
    hp.tdf_begin(5, 5)
    with pytest.raises(ValueError):
        hp.tdf_write(np.array([49, 32, 49, 32, 49, 10], np.int64))
    hp.tdf_write(np.array([49, 32, 49, 32, 49, 10], np.uint8))
    assert hp.tdf_finalize() == dict(entries_read=1, nnz=1)


def test_an_empty_stream_gives_empty_columns(hp):
    info = stream(hp, [], 7, 9)
    assert info == dict(entries_read=0, nnz=0)
    counts, rows, offs = hp.get_A()
    assert len(counts) == 0 and len(rows) == 0 and offs.shape == (10,) and not offs.any()
    assert stream(hp, [b"", b"\n", b""], 7, 9) == dict(entries_read=0, nnz=0)


# ---------------------------------------------------------------- 7. the C++ driver, a process of its own
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    case = next(c for c in CASES if c.id == "passes-4")                  # 4400 lines
    d = tmp_path_factory.mktemp("tdf_stream")
    good, bad = d / "good.tdf", d / "bad.tdf"
    text = case.build()[0]
    good.write_bytes(text)
    bad.write_bytes(text[:30000] + b"7 x 7\n" + text[30000:])
    return case, str(good), str(bad), ingest_rule(text[:30000] + b"7 x 7\n" + text[30000:], case.V, case.D)


@pytest.mark.parametrize("piece", [1000, 0])
def test_the_driver_finds_stream_and_whole_text_identical(files, piece):
    case, good, _, _ = files
    assert os.path.exists(EXE), "build with make -C isle_amd/csrc"
    r = subprocess.run([EXE, good, str(case.V), str(case.D), str(piece)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"identical: 4400 entries read, nnz \d+", r.stdout.strip())


def test_the_driver_finds_the_two_refusals_equal(files):
    case, _, bad, want = files
    assert want[0] == "error" and want[1] == 1
    r = subprocess.run([EXE, bad, str(case.V), str(case.D), "1000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "both refuse: %s on line %d" % (KINDS[1], want[2])


# ---------------------------------------------------------------- 8. a whole-text ingest between the parts of a stream, or of a feed
def _between():
    """The stream's text and its cut, inside a line; another text of more lines than one 4096-byte tile holds and of more entries than the
    stream has taken by the cut, with its own V and D."""
    ours, other = (next(c for c in CASES if c.id == i) for i in ("passes-2", "passes-4"))
    text, cut = ours.build()[0], 10001
    assert b"\n" not in text[cut - 2:cut + 2] and text[:cut].count(b"\n") < 4400 < other.build()[0].count(b"\n") + 1
    return ours, text, cut, other, other.build()[0]


@pytest.mark.parametrize("refused", [False, True], ids=["taken", "refused"])
def test_a_whole_text_ingest_inside_an_open_stream_disturbs_neither(hp, refused):
    ours, text, cut, other, text2 = _between()
    hp.tdf_begin(ours.V, ours.D, _piece_bytes=1000)
    hp.tdf_write(text[:cut])
    if refused:
        with pytest.raises(IsleHipError, match=re.escape("%s on line 4401" % KINDS[5]) + r"\b"):
            hp.ingest_tdf(text2 + b"1 1 0\n", other.V, other.D)
    else:
        assert_exact(hp, hp.ingest_tdf(text2, other.V, other.D), ingest_rule(text2, other.V, other.D))
    hp.tdf_write(text[cut:])
    assert_exact(hp, hp.tdf_finalize(), ingest_rule(text, ours.V, ours.D))


def test_a_whole_text_ingest_inside_an_open_feed_disturbs_neither(hp):
    _, _, _, other, text2 = _between()
    d, w, c = base_corpus()
    hp.feed_begin(BASE_V, BASE_D)
    hp.feed(d[:1000], w[:1000], c[:1000])
    assert_exact(hp, hp.ingest_tdf(text2, other.V, other.D), ingest_rule(text2, other.V, other.D))
    hp.feed(d[1000:], w[1000:], c[1000:])
    assert hp.feed_finalize() == (int(np.count_nonzero(c)), len(feed_rule(d, w, c, BASE_D)[0]))
    for got, want in zip(hp.get_A(), feed_rule(d, w, c, BASE_D)):
        np.testing.assert_array_equal(got, want)
