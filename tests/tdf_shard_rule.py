"""The plain rules of ingesting one tdf file onto document shards, the case table of its tests and the certificates.  No GPU, no torch.

  ownership   a line is a maximal run of bytes that ends in '\\n' or at the end of the file.  The byte range [b, e) owns the lines whose first
              byte s has b <= s < e.  Rank r of N takes [size * r // N, size * (r + 1) // N): every line is owned once, and the owned bytes
              of the ranks side by side are the file.
  counts      a line counts for its document if ingest_rule takes it as an entry; a blank or a bad line counts for nothing.  Repeated
              (doc, word) pairs count every time: the balance is by lines.
  bounds      from the counts summed over all ranges: bound p (0 < p < parts) is the first document d with
              lines(documents before d) >= lines_total * p // parts, at most D, at least bound p - 1; bound 0 is 0, bound parts is D.
  window      the shard [d0, d1) of ingest_rule's matrix: the entries of those columns, their offsets rebased to begin at 0.  The first
              bad line, its kind and entries_read are the whole text's.

The rules are stated here with list operations and exact integers; they call ingest_rule for what an entry is and share nothing with
isle_amd/hot_path.py or the library.  The certificates take arrays; tests/test_tdf_shard_rule_cpu.py feeds them arrays made by these rules
and by wrong ones."""
import numpy as np

from ingest_rule import ingest_rule


# ---------------------------------------------------------------------------------------------------------------------------------
# rules
# ---------------------------------------------------------------------------------------------------------------------------------
def lines_with_starts(text):
    """-> [(first byte position, the line's bytes with its '\\n' if it has one)]"""
    text, out, s = bytes(text), [], 0
    while s < len(text):
        nl = text.find(b"\n", s)
        e = len(text) if nl < 0 else nl + 1
        out.append((s, text[s:e]))
        s = e
    return out


def owned(text, b, e):
    """the bytes of the lines that [b, e) owns"""
    return b"".join(line for s, line in lines_with_starts(text) if b <= s < e)


def rank_range(size, r, n):
    return size * r // n, size * (r + 1) // n


def entry_of_line(line, V, D):
    """-> (doc, word) 0-based of a line that is an entry, else None (blank or bad: the counting pass tells them not apart)"""
    res = ingest_rule(line, V, D)
    if res[0] != "ok" or res[4] == 0:
        return None
    return int(np.flatnonzero(np.diff(res[3]))[0]), int(res[2][0])


def doc_line_counts(text, V, D):
    """valid lines per document, int64[D]"""
    cnt = np.zeros(D, np.int64)
    for _, line in lines_with_starts(text):
        en = entry_of_line(line, V, D)
        if en is not None:
            cnt[en[0]] += 1
    return cnt


def bounds_from_counts(counts, parts):
    counts = [int(x) for x in counts]
    D, total = len(counts), sum(counts)
    before = [0]
    for x in counts:
        before.append(before[-1] + x)
    b = [0]
    for p in range(1, parts):
        target = total * p // parts
        d = next((d for d in range(D + 1) if before[d] >= target), D)
        b.append(max(min(d, D), b[-1]))
    b.append(D)
    return np.asarray(b, np.int64)


def window_cut(res, d0, d1):
    """res: ingest_rule's ("ok", counts, rows, offs, entries_read) -> (counts, rows, offs) of the columns [d0, d1), offsets from 0"""
    _, cnt, rows, offs, _ = res
    o0, o1 = int(offs[d0]), int(offs[d1])
    return cnt[o0:o1], rows[o0:o1], (offs[d0:d1 + 1] - o0).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# certificates
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    assert a.tobytes() == b.tobytes(), "%s differs, first at %s" % (what, np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))[:1])


def certify_window(got, res, d0, d1, D):
    """got: dict(cnt float32, rows uint32, offs int64, entries_read, nnz) of a windowed stream over [d0, d1); res: ingest_rule of the whole text."""
    assert res[0] == "ok"
    cnt, rows, offs = window_cut(res, d0, d1)
    assert len(got["offs"]) == d1 - d0 + 1, "window [%d, %d): %d offsets" % (d0, d1, len(got["offs"]))
    _same_bits(np.asarray(got["offs"], np.int64), offs, "offsets")
    _same_bits(np.asarray(got["rows"], np.uint32), rows, "rows")
    _same_bits(np.asarray(got["cnt"], np.float32), cnt, "counts")
    assert got["entries_read"] == res[4], "entries_read %d, the whole text has %d" % (got["entries_read"], res[4])
    assert got["nnz"] == len(cnt)


def certify_counts(got, text, V, D, parts_list, owned_text=None):
    """got: dict(doc_lines, lines_local, lines_global, bounds {parts: array}) of a one-rank counting stream over owned_text (default: text)"""
    want = doc_line_counts(text if owned_text is None else owned_text, V, D)
    assert np.array_equal(np.asarray(got["doc_lines"], np.int64), want), "doc_lines differ at documents %s" % np.flatnonzero(np.asarray(got["doc_lines"], np.int64) != want)[:10]
    assert got["lines_local"] == got["lines_global"] == int(want.sum())
    for parts in parts_list:
        b = bounds_from_counts(want, parts)
        assert np.array_equal(np.asarray(got["bounds"][parts], np.int64), b), "parts %d: bounds %s, the rule gives %s" % (parts, got["bounds"][parts], b)


def certify_sharded(ranks, text, V, D, single=None):
    """ranks: per rank dict(bounds, cnt, rows, offs, entries_read, nnz, lines_local, lines_global).  The bounds are the rule's on every
    rank, the line counts are those of the ranks' byte ranges, and the shards side by side are ingest_rule's matrix; single (cnt, rows,
    offs of a single-rank ingest of the file): the same against it.  -> the bounds"""
    n, size = len(ranks), len(text)
    res = ingest_rule(text, V, D)
    assert res[0] == "ok"
    per_rank = [doc_line_counts(owned(text, *rank_range(size, r, n)), V, D) for r in range(n)]
    total = np.sum(per_rank, axis=0)
    want_b = bounds_from_counts(total, n)
    for r, q in enumerate(ranks):
        assert np.array_equal(np.asarray(q["bounds"], np.int64), want_b), "rank %d: bounds %s, the rule gives %s" % (r, q["bounds"], want_b)
        assert int(q["lines_local"]) == int(per_rank[r].sum()), "rank %d counted %d lines, its range owns %d" % (r, q["lines_local"], per_rank[r].sum())
        assert int(q["lines_global"]) == int(total.sum()) == res[4], "rank %d: lines_global %d" % (r, q["lines_global"])
        assert int(q["entries_read"]) == res[4], "rank %d: entries_read %d of %d" % (r, q["entries_read"], res[4])
        certify_window(dict(cnt=q["cnt"], rows=q["rows"], offs=q["offs"], entries_read=int(q["entries_read"]), nnz=int(q["nnz"])), res, int(want_b[r]), int(want_b[r + 1]), D)
    if single is not None:
        lens = np.concatenate([np.diff(np.asarray(q["offs"], np.int64)) for q in ranks])
        _same_bits(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(single[2], np.int64), "offsets side by side")
        _same_bits(np.concatenate([np.asarray(q["rows"], np.uint32) for q in ranks]), np.asarray(single[1], np.uint32), "rows side by side")
        _same_bits(np.concatenate([np.asarray(q["cnt"], np.float32) for q in ranks]), np.asarray(single[0], np.float32), "counts side by side")
    return want_b


def reference_ranks(text, V, D, n, summed=True, window_shift=0, overlap=False):
    """What n ranks must hold, from the rules alone.  Wrong rules: summed=False, every rank plans from its own range's counts;
    window_shift, the windows are cut that many documents late; overlap, a range also takes the line that its first byte lies inside,
    so that line is counted by two ranges."""
    size = len(text)
    res = ingest_rule(text, V, D)
    per_rank = []
    for r in range(n):
        b, e = rank_range(size, r, n)
        mine = owned(text, b, e)
        if overlap and b < e:
            mine = b"".join(line for s, line in lines_with_starts(text) if s < b < s + len(line)) + mine
        per_rank.append(doc_line_counts(mine, V, D))
    total = np.sum(per_rank, axis=0)
    out = []
    for r in range(n):
        b = bounds_from_counts(total if summed else per_rank[r], n)
        d0, d1 = min(int(b[r]) + window_shift, D), min(int(b[r + 1]) + window_shift, D)
        cnt, rows, offs = window_cut(res, d0, d1)
        out.append(dict(bounds=b, cnt=cnt, rows=rows, offs=offs, entries_read=res[4], nnz=len(cnt), lines_local=int(per_rank[r].sum()),
                        lines_global=int(total.sum())))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the texts of the multi-rank test (tests/test_gpu_tdf_sharded.py): id -> (ranks, V, D, text)
# ---------------------------------------------------------------------------------------------------------------------------------
def _spread(nlines, docs_used, V, seed):
    """document-major lines, like a corpus file, over documents 1 .. docs_used; counts 1 .. 5; some (doc, word) pairs repeat"""
    rng = np.random.default_rng(seed)
    doc = np.sort(rng.integers(1, docs_used + 1, nlines))
    return b"".join(b"%d %d %d\n" % (d, rng.integers(1, V + 1), i % 5 + 1) for i, d in enumerate(doc))


SHARDED = {
    "one-line-no-newline-4": (4, 9, 5, b"3 2 7"),                                                   # three ranks own no line
    "long-line-leading-zeros-3": (3, 9, 5, b"1 1 1\n" + b"0" * 200 + b"2 3 4\n5 5 5\n2 1 2\n"),     # bytes 6 .. 211 are one line: rank 1, [74, 149), owns nothing
    "crlf-cut-2": (2, 9, 5, b"1 1 1\r\n2 2 2"),                                                     # 12 bytes: rank 1 begins at byte 6, the '\n' behind the '\r' at byte 5
    "one-document-4": (4, 50, 6, b"".join(b"4 %d %d\n" % (w + 1, w + 1) for w in range(40))),       # every entry in document 4: empty windows
    "repeated-pair-across-ranges-2": (2, 9, 5, b"2 3 11\n1 1 1\n4 4 4\n5 1 2\n2 3 99\n"),          # the first in the file wins
    "trailing-empty-documents-3": (3, 20, 40, _spread(60, 9, 20, 5)),
    "spread-4": (4, 30, 50, _spread(300, 50, 30, 6)),
    "spread-3-to-threshold": (3, 30, 50, _spread(300, 50, 30, 7)),
}
AGREE_WORLD = 4                 # one more run on four ranks: every rank passes another agree_tag
THRESHOLD_CASE, THRESHOLD_K = "spread-3-to-threshold", 3
