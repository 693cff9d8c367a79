"""The counting text stream (isle_hip_tdf_begin_counts / _finalize_counts, HotPath.tdf_begin_counts / tdf_finalize_counts) on one rank
against the plain rules of tests/tdf_shard_rule.py: the lines per document, lines_local, and the bounds for 1, 2, 3 and 8 parts.  The
texts aim at tdf_doc_count_k: it works one line per lane and adds once per run of equal documents within a wave of 64 lanes, in
workgroups of 256 lines."""

import numpy as np
import pytest

import tdf_shard_rule as tr
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu

V, D = 40, 23
PARTS = (1, 2, 3, 8)


def counts(hp, parts_of_text, piece=0):
    """one counting stream per number of parts (the stream ends with its plan) -> what certify_counts takes"""
    got = dict(bounds={})
    for parts in PARTS:
        hp.tdf_begin_counts(V, D, _piece_bytes=piece)
        for p in parts_of_text:
            hp.tdf_write(p)
        r = hp.tdf_finalize_counts(parts, fetch_doc_lines=True)
        got["bounds"][parts] = r["bounds"]
        if "doc_lines" in got:
            assert np.array_equal(got["doc_lines"], r["doc_lines"]) and got["lines_local"] == r["lines_local"]
        got.update(doc_lines=r["doc_lines"], lines_local=r["lines_local"], lines_global=r["lines_global"])
    return got


def run_text(lengths, first_doc=1):
    """runs of the given lengths, one document after another"""
    out, i = [], 0
    for j, n in enumerate(lengths):
        d = (first_doc - 1 + j) % D + 1
        for _ in range(n):
            out.append(b"%d %d %d\n" % (d, i % V + 1, i % 7 + 1))
            i += 1
    return b"".join(out)


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257, 2049))
def test_runs_of_one_document(hp, n):
    """a run of n lines of one document between two short runs: it begins at lane 3, spans whole waves and workgroups, and ends mid-wave"""
    text = run_text([3, n, 5], first_doc=7)
    tr.certify_counts(counts(hp, [text], piece=1 << 20), text, V, D, PARTS)


def test_a_run_across_a_piece_cut(hp):
    text = run_text([10, 300, 10])
    cut = len(text) // 2
    tr.certify_counts(counts(hp, [text[:cut], text[cut:]], piece=4096), text, V, D, PARTS)
    tr.certify_counts(counts(hp, [text], piece=7), text, V, D, PARTS)


def test_runs_of_length_one(hp):
    text = b"".join(b"%d %d 1\n" % (i % 2 * 5 + 3, i % V + 1) for i in range(700))    # documents 3 and 8 in turn
    tr.certify_counts(counts(hp, [text], piece=1 << 20), text, V, D, PARTS)


def test_blank_and_bad_lines_inside_a_run_neither_split_nor_lengthen_it(hp):
    """every fifth line blank, every seventh bad (of every kind the parser knows); nothing is refused, none of them is counted"""
    bad = [b"4 x 1\n", b"4 1 2 3\n", b"4 1\n", b"99 1 1\n", b"4 1 0\n", b"4 1 4294967296\n"]
    out = []
    for i in range(600):
        if i % 5 == 4:
            out.append(b" \t\r\n" if i % 2 else b"\n")
        elif i % 7 == 6:
            out.append(bad[(i // 7) % len(bad)])
        else:
            out.append(b"%d %d 2\n" % (4 if i < 400 else 5, i % V + 1))
    text = b"".join(out) + b"5 1 1"                                                    # and a last line without '\n'
    want = tr.doc_line_counts(text, V, D)
    assert want[3] > 64 and want[4] > 64 and want.sum() < 601 - 120
    tr.certify_counts(counts(hp, [text], piece=1 << 20), text, V, D, PARTS)
    tr.certify_counts(counts(hp, [text], piece=100), text, V, D, PARTS)


def test_a_byte_range_that_starts_and_ends_mid_line(hp, tmp_path):
    """the range reader of HotPath (the rule of tdf_pump::file_range): what the stream counts is what the range owns"""
    text = run_text([40, 40, 40, 40])
    path = str(tmp_path / "range.tdf")
    with open(path, "wb") as f:
        f.write(text)
    nl = [i for i, ch in enumerate(text) if ch == 10]
    for b, e in ((nl[10] - 2, nl[100] - 2), (nl[10] + 1, nl[100] + 1), (nl[10], nl[100]), (0, 3), (len(text) - 3, len(text)), (nl[5] + 2, nl[5] + 4), (7, 7)):
        mine = tr.owned(text, b, e)
        got = dict(bounds={})
        for parts in PARTS:
            hp.tdf_begin_counts(V, D, _piece_bytes=64)
            with open(path, "rb", buffering=0) as f:
                assert hp._pump(f, b, e) == len(mine), (b, e)
            r = hp.tdf_finalize_counts(parts, fetch_doc_lines=True)
            got["bounds"][parts] = r["bounds"]
            got.update(doc_lines=r["doc_lines"], lines_local=r["lines_local"], lines_global=r["lines_global"])
        tr.certify_counts(got, text, V, D, PARTS, owned_text=mine)


def test_one_process_plans_and_ingests_every_part(hp, tmp_path):
    """ingest_tdf_file_sharded without a communicator: parts and part given, pass 1 over the whole file"""
    from ingest_rule import ingest_rule
    text = run_text([30, 1, 0, 64, 5, 100, 2])
    path = str(tmp_path / "parts.tdf")
    with open(path, "wb") as f:
        f.write(text)
    res = ingest_rule(text, V, D)
    want_b = tr.bounds_from_counts(tr.doc_line_counts(text, V, D), 3)
    for part in range(3):
        info = hp.ingest_tdf_file_sharded(path, V, D, max_entries=res[4], parts=3, part=part, _piece_bytes=50)
        assert np.array_equal(info["bounds"], want_b) and info["lines_local"] == info["lines_global"] == res[4]
        cnt, rows, offs = hp.get_A()
        tr.certify_window(dict(info, cnt=cnt, rows=rows, offs=offs), res, int(want_b[part]), int(want_b[part + 1]), D)


def test_stream_states(hp):
    hp.tdf_begin_counts(V, D)
    with pytest.raises(IsleHipError, match="tdf_finalize: the open stream counts lines"):
        hp.tdf_finalize()
    hp.tdf_finalize_counts(2)                                                          # still open behind the refusal: an empty text
    with pytest.raises(IsleHipError, match="no open counting stream"):
        hp.tdf_finalize_counts(2)
    hp.tdf_begin(V, D)
    with pytest.raises(IsleHipError, match="no open counting stream"):
        hp.tdf_finalize_counts(2)
    hp.tdf_finalize()
