"""The windowed text stream (isle_hip_tdf_begin_window, HotPath.tdf_begin_window) on one rank against the cut of the plain rule
(tests/tdf_shard_rule.py window_cut of tests/ingest_rule.py): A is the columns [doc_begin, doc_end) of what ingest_tdf gives, offsets
rebased, bit for bit, entries_read is the whole text's, and a text is refused where and how ingest_tdf refuses it, whichever documents
the window holds."""
import re

import numpy as np
import pytest

import tdf_shard_rule as tr
from ingest_cases import CASES
from ingest_rule import KINDS, ingest_rule
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu

TABLE = [c for c in CASES if not c.large and not c.long_text]


def window(hp, text, V, D, d0, d1, piece=0, max_entries=0):
    hp.tdf_begin_window(V, D, d0, d1, _piece_bytes=piece)
    hp.tdf_write(text)
    info = hp.tdf_finalize(max_entries)
    cnt, rows, offs = hp.get_A()
    return dict(info, cnt=cnt, rows=rows, offs=offs)


def windows_of(res, D):
    """the whole range, [0, 1), [D - 1, D), an empty window, an interior window, and a window whose documents have no line (if there is one)"""
    w = [(0, D), (0, 1), (D - 1, D), (D // 2, D // 2), (D // 3, (2 * D + 2) // 3)]
    empty = np.flatnonzero(np.diff(res[3]) == 0)
    if empty.size:
        d = e = int(empty[0])
        while e < D and res[3][e + 1] == res[3][e]:
            e += 1
        w.append((d, e))
    return w


@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_every_small_case_in_windows(hp, case):
    """A text the rule takes: every window is the cut of the rule's matrix.  A text the rule refuses: the same kind and the same line as
    ingest_tdf, from windows that hold no document at all, the first alone and the last alone (the bad line's document, where it names
    one within range, lies outside two of them at least)."""
    text, res = case.build()[0], ingest_rule(case.build()[0], case.V, case.D)
    if res[0] == "ok":
        for d0, d1 in windows_of(res, case.D):
            got = window(hp, text, case.V, case.D, d0, d1, piece=4097, max_entries=res[4])
            tr.certify_window(got, res, d0, d1, case.D)
            assert hp._a_shape == (case.V, d1 - d0, got["nnz"])
        return
    _, kind, line = res
    with pytest.raises(IsleHipError) as whole:
        hp.ingest_tdf(text, case.V, case.D)
    assert "%s on line %d" % (KINDS[kind], line) in str(whole.value)
    for d0, d1 in ((0, 0), (0, 1), (case.D - 1, case.D)):
        with pytest.raises(IsleHipError, match=re.escape("%s on line %d" % (KINDS[kind], line)) + r"\b"):
            window(hp, text, case.V, case.D, d0, d1, piece=7)
        with pytest.raises(IsleHipError, match="no open text stream"):
            hp.tdf_finalize()


def test_max_entries_counts_every_line_of_the_text(hp):
    text = b"1 1 1\n2 2 2\n3 3 3\n\n4 4 4\n"
    res = ingest_rule(text, 5, 5)
    tr.certify_window(window(hp, text, 5, 5, 1, 2, max_entries=4), res, 1, 2, 5)
    with pytest.raises(IsleHipError, match=r"file has 4 entries, <max_entries> says 1\b"):
        window(hp, text, 5, 5, 1, 2, max_entries=1)          # the window holds one entry: that is not what is counted


def _edge_text(nlines, mode, d0, d1, D):
    """nlines lines; mode "alt": documents inside and outside [d0, d1) in turn; "in" / "out": all inside / all outside"""
    inside = [d0, d1 - 1]
    outside = [d for d in (d0 - 1, d1) if 0 <= d < D]
    out = []
    for i in range(nlines):
        pool = inside if mode == "in" or (mode == "alt" and i % 2 == 0) else outside
        out.append(b"%d %d %d\n" % (pool[(i // 2) % len(pool)] + 1, i % 50 + 1, i % 9 + 1))
    return b"".join(out)


@pytest.mark.parametrize("nlines", (255, 256, 257, 4095, 4096, 4097))
@pytest.mark.parametrize("mode", ("alt", "in", "out"))
def test_filter_and_scan_edges(hp, nlines, mode):
    """block and tile edges of the filter and of the scan behind it, with the documents doc_begin - 1, doc_begin, doc_end - 1, doc_end"""
    V, D, d0, d1 = 50, 12, 4, 7
    text = _edge_text(nlines, mode, d0, d1, D)
    res = ingest_rule(text, V, D)
    got = window(hp, text, V, D, d0, d1, piece=1 << 20, max_entries=nlines)      # one piece: nlines lines in one launch
    tr.certify_window(got, res, d0, d1, D)
    assert (got["nnz"] == 0) == (mode == "out")


@pytest.mark.parametrize("piece", (1, 7, 4096))
def test_pieces_cut_anywhere(hp, piece):
    V, D, d0, d1 = 50, 12, 4, 7
    text = _edge_text(300 if piece == 1 else 1500, "alt", d0, d1, D)[:-1] + b"\r"      # the last line ends without '\n'
    res = ingest_rule(text, V, D)
    tr.certify_window(window(hp, text, V, D, d0, d1, piece=piece), res, d0, d1, D)


def test_window_arguments_and_stream_states(hp):
    with pytest.raises(IsleHipError, match=r"tdf_begin_window: documents \[3, 2\) of 5"):
        hp.tdf_begin_window(5, 5, 3, 2)
    with pytest.raises(IsleHipError, match=r"tdf_begin_window: documents \[0, 6\) of 5"):
        hp.tdf_begin_window(5, 5, 0, 6)
    text = b"1 1 1\n5 5 5\n"
    got = window(hp, text, 5, 5, 5, 5)                                            # doc_begin == doc_end == D: zero columns
    assert got["nnz"] == 0 and got["entries_read"] == 2 and len(got["offs"]) == 1 and got["offs"][0] == 0
    res = ingest_rule(text, 5, 5)                                                 # an ordinary stream behind a windowed one is whole again
    hp.tdf_begin(5, 5)
    hp.tdf_write(text)
    info = hp.tdf_finalize(2)
    cnt, rows, offs = hp.get_A()
    tr.certify_window(dict(info, cnt=cnt, rows=rows, offs=offs), res, 0, 5, 5)
