"""The per-document topic files formatted on the device (isle_hip_infer_text; HotPath.infer_text, write_infer_text, infer_text_size;
isle_amd/csrc/infer_text.hip; ISLEInfer's top_topics_* files).

Every comparison is byte equality of whole texts.  The expected text is the numpy restatement of tests/test_doc_text_cpu.py (held there
to a transcription of the reference's writer and to the library's host formatter) applied to what the same infer_resident call
returned: offs / topic / weight for ISLE_DOCTEXT_ENTRIES, top_topic / top_weight for ISLE_DOCTEXT_TOP.  tests/test_gpu_infer_resident.py
holds those arrays to the certified path.  A tile is 1024 lines, a piece at most CHUNK = 16 MiB."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import infer_certificate as ic
from isle_amd import HotPath, IsleHipError
from test_doc_text_cpu import NUM_END, doc_lines_text, entries_text, top_text
from test_model_text_cpu import _const, _uint_field

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")
CHUNK = 16 << 20
TILE = 1024


def load(hp, case):
    hp.upload_counts(case["M"].shape[0], case["counts"], case["rows"], case["offs"])
    return case["offs"].shape[0] - 1


def expected(got, what, base=1, rows=None):
    if what == "entries":
        return entries_text(got["offs"], got["topic"], got["weight"], base, rows)
    return top_text(got["top_topic"], got["top_weight"], base, rows)


def pieces_of(hp, what, rows=None, base=1):
    got = []
    n = hp._infer_text_call(what, rows, base, lambda mv: got.append(bytes(mv)))
    return got, n


# ---- 1. both kinds across k ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_weight", (None, 0.0), ids=("rule", "all"))
@pytest.mark.parametrize("k", (1, 7, 257, 1024))
def test_both_kinds(hp, k, min_weight):
    case = ic.make_case(k)
    D = load(hp, case)
    got = hp.infer_resident(case["M"], min_weight=min_weight)
    conv, length = got["llh"][:, 0] != 0, np.diff(case["offs"])
    # an empty document, one with words that did not converge, and a converged one: skipped rows are part of the case
    assert (length == 0).any() and (~conv & (length > 0)).any() and conv.any()
    assert (np.diff(got["offs"])[~conv] == 0).all() and (got["top_topic"][~conv] < 0).all()
    for what in ("entries", "top"):
        want = expected(got, what)
        text = hp.infer_text(what)
        assert len(text) == len(want) and text == want, (k, min_weight, what)
        assert hp.infer_text_size(what) == (len(want), want.count(b"\n"))
        assert hp.infer_text(what, rows=(0, D)) == want                          # a second call: the same bytes
    lines = hp.infer_text("entries")
    assert lines.count(b"\n") == got["nentries"]
    if k == 1 and min_weight is None:
        assert lines == b"" and hp.infer_text("top") == b""                      # nothing is heavier than 1 / 1
    if k == 1 and min_weight == 0.0:
        assert lines == b"".join(b"%d\t1\t1.000000\n" % (d + 1) for d in np.flatnonzero(conv)) != b""


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------------
def test_tile_edges_of_the_entries(hp):
    """ENTRIES texts of 0, 1, 1023, 1024, 1025 and 2049 lines at k = 1024.  With min_weight = 0 every converged document of the case holds
    exactly 1024 entries (all weights are positive), so whole rows give multiples of the tile only and no document can lie across a tile
    boundary.  Those ranges are run as they are; the other counts come from the same documents with min_weight set to the (n + 1)-th
    largest weight of the rows, which leaves exactly n entries spread over the documents, one of them across the boundary."""
    case = ic.make_case(1024)
    D = load(hp, case)
    every = hp.infer_resident(case["M"], min_weight=0.0)
    offs = every["offs"]
    full = np.flatnonzero(np.diff(offs) == 1024)
    assert full.size >= 3 and set(np.diff(offs).tolist()) == {0, 1024} and offs[1] == 0          # row 0 is empty
    b = int(full[0])
    for r, n in (((0, 1), 0), ((0, b + 1), 1024), ((b, b + 1), 1024), ((b, b + 2), 2048), ((0, D), int(offs[D])), ((b + 1, D), int(offs[D] - offs[b + 1]))):
        want = expected(every, "entries", base=3, rows=r)
        assert want.count(b"\n") == n
        assert hp.infer_text("entries", rows=r, base=3) == want and hp.infer_text_size("entries", rows=r, base=3) == (len(want), n)
    for r in ((0, 0), (5, 5), (D, D)):                                            # row_begin == row_end
        assert pieces_of(hp, "entries", r) == ([], (0, 0)) and pieces_of(hp, "top", r) == ([], (0, 0))
    spans = 0
    for lo in (0, b + 1):                                                          # the whole case, and a range starting inside it
        desc = np.sort(every["weight"][offs[lo]:])[::-1]
        for n in (0, 1, 1023, 1024, 1025, 2049):
            assert desc[n] < desc[n - 1] or n == 0                                 # no tie at the threshold
            got = hp.infer_resident(case["M"], min_weight=float(desc[n]))
            o = got["offs"]
            assert o[D] - o[lo] == n
            want = expected(got, "entries", base=3, rows=(lo, D))
            assert want.count(b"\n") == n and (n == 0) == (want == b"")
            assert pieces_of(hp, "entries", (lo, D), 3) == ([want] if n else [], (len(want), n)), (lo, n)
            inner = o[lo:] - o[lo]
            spans += int(n > TILE and ((inner[:-1] < TILE) & (inner[1:] > TILE)).any())   # a document across the first tile boundary
    assert spans >= 2


def test_tile_edges_of_the_top_topics(hp):
    # five candidate lines per row: 204, 205 and 206 rows are 1020, 1025 and 1030 candidates around the tile of 1024
    V, k, D = 64, 7, 260
    rng = np.random.default_rng(4)
    M = ((rng.random((V, k)) ** 2 + 0.01) / V).astype(np.float32)
    lens = rng.integers(0, 30, size=D)
    lens[[0, 100, 204, 205]] = 0
    offs = np.zeros(D + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    rows = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lens]).astype(np.uint32)
    hp.upload_counts(V, rng.integers(1, 6, size=rows.size).astype(np.float32), rows, offs)
    got = hp.infer_resident(M)
    held = (got["top_topic"] >= 0).sum(axis=1)
    assert set(held.tolist()) >= {0, 1, 2, 3} and held.max() <= 5                 # rows with no, some and many slots
    for n in (204, 205, 206):
        for lo in (0, 3, 54):
            want = expected(got, "top", base=11, rows=(lo, lo + n))
            assert hp.infer_text("top", rows=(lo, lo + n), base=11) == want and want
            assert hp.infer_text_size("top", rows=(lo, lo + n), base=11) == (len(want), int(held[lo:lo + n].sum()))
    for r in ((0, D), (2, D), (205, 206), (204, 206)):
        assert hp.infer_text("top", rows=r) == expected(got, "top", rows=r)
        assert hp.infer_text("entries", rows=r) == expected(got, "entries", rows=r)


# ---- 3. runs of empty documents: the offsets window and its fallback -----------------------------------------------------------------
def test_empty_runs(hp):
    V, k, gap = 64, 7, 5000
    rng = np.random.default_rng(3)
    M = ((rng.random((V, k)) + 0.25) / V).astype(np.float32)
    words = [np.sort(rng.choice(V, size=n, replace=False)).astype(np.uint32) for n in (5, 9, 1, 30)]
    lens = np.concatenate([[5], np.zeros(gap, int), [9, 1, 30], np.zeros(gap, int)])
    offs = np.zeros(lens.size + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    rows = np.concatenate(words)
    counts = rng.integers(1, 6, size=rows.size).astype(np.float32)
    hp.upload_counts(V, counts, rows, offs)
    D = lens.size
    got = hp.infer_resident(M, min_weight=0.0)
    assert got["nconverged"] == 4 and got["nentries"] == 4 * k and got["offs"][1] == got["offs"][gap + 1] == k   # the run between two documents
    assert got["offs"][gap + 4] == got["offs"][D] == 4 * k                                                      # ... and the run at the end
    for what in ("entries", "top"):
        assert hp.infer_text(what) == expected(got, what) != b""
        for r in ((1, D), (17, gap + 2), (gap, D), (gap + 4, D), (3, gap), (0, 1), (gap + 1, gap + 4)):
            assert hp.infer_text(what, rows=r, base=5) == expected(got, what, base=5, rows=r), (what, r)
    assert hp.infer_text("entries", rows=(3, gap)) == b"" and hp.infer_text("top", rows=(gap + 4, D)) == b""


# ---- 4. digit edges of the numbers ---------------------------------------------------------------------------------------------
def test_digit_edges_and_the_largest_number(hp):
    case = ic.make_case(7)
    load(hp, case)
    got = hp.infer_resident(case["M"])
    D = got["offs"].size - 1
    has = np.flatnonzero(np.diff(got["offs"]) > 0)
    j = 1 + int(np.argmin(np.diff(has)))
    prev, m = int(has[j - 1]), int(has[j])                                        # two rows with lines, no row with lines between them
    assert m - prev < 10 and got["nentries"] < TILE                               # all in one tile
    part = hp.infer_resident(case["M"], docs=(prev, D))                           # row 0 is document prev, row m - prev the next with lines
    for edge in (10, 10 ** 4, 10 ** 9):
        base = edge - (m - prev)                                                   # row m - prev prints as `edge`, row 0 with a digit less
        for what in ("entries", "top"):
            text = hp.infer_text(what, base=base)
            assert text == expected(part, what, base=base)
            assert text.startswith(b"%d\t" % base) and (b"\n%d\t" % edge) in text
    got = hp.infer_resident(case["M"])
    rows = int(has[-1]) + 1                                                        # the last row of the range prints lines
    base = NUM_END - 1 - (rows - 1)
    for what in ("entries", "top"):
        text = hp.infer_text(what, rows=(0, rows), base=base)
        assert text == expected(got, what, base=base, rows=(0, rows)) and b"\n2147483646\t" in text
        seen = []
        with pytest.raises(IsleHipError) as e:
            hp._infer_text_call(what, (0, rows), base + 1, lambda mv: seen.append(bytes(mv)))
        assert seen == [] and "error -1" in str(e.value) and "row %d " % (rows - 1) in str(e.value), str(e.value)
        with pytest.raises(IsleHipError):
            hp.infer_text_size(what, rows=(0, rows), base=base + 1)
        assert hp.infer_text(what, rows=(0, rows), base=base) == text              # the context is usable, the bytes are right
        assert hp.infer_text(what, rows=(0, rows - 1), base=base + 1) == expected(got, what, base=base + 1, rows=(0, rows - 1))
    with pytest.raises(IsleHipError):
        hp.infer_text("entries", base=2 ** 40)


# ---- 5. pieces -----------------------------------------------------------------------------------------------------------------
def big_result(hp):
    V, k, D, n = 1403, 1024, 2000, 60
    rng = np.random.default_rng(8)
    M = ((rng.random((V, k), np.float32) + np.float32(0.25)) / np.float32(V)).astype(np.float32)
    rows = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for _ in range(D)]).astype(np.uint32)
    offs = np.arange(D + 1, dtype=np.int64) * n
    hp.upload_counts(V, rng.integers(1, 4, size=rows.size).astype(np.float32), rows, offs)
    return hp.infer_resident(M, min_weight=0.0)


def test_pieces(hp):
    got = big_result(hp)
    want = expected(got, "entries")
    assert len(want) > 2 * CHUNK
    me, threads = threading.get_ident(), []
    parts = []

    def consume(mv):
        threads.append(threading.get_ident())
        parts.append(bytes(mv))

    nbytes, nlines = hp._infer_text_call("entries", None, 1, consume)
    assert len(parts) >= 3 and all(0 < len(p) <= CHUNK for p in parts) and all(p.endswith(b"\n") for p in parts)
    assert set(threads) == {me}
    text = b"".join(parts)
    assert len(text) == len(want) and text == want                                # in order: the concatenation is the file
    assert (nbytes, nlines) == (len(want), got["nentries"]) == hp.infer_text_size("entries")
    assert hp.infer_text("entries") == text                                       # a second call: the same bytes
    assert hp.infer_text("top") == expected(got, "top")

    seen = []

    def refusing(ptr, n, user):
        seen.append(C.string_at(ptr, n))
        return 1 if len(seen) == 2 else 0

    from isle_amd.hot_path import _TEXT_SINK
    cb = _TEXT_SINK(refusing)
    nb = C.c_uint64()
    rc = hp._lib.isle_hip_infer_text(hp._h, 0, 0, 2000, 1, C.cast(cb, C.c_void_p), None, C.byref(nb), None)
    assert rc == -1 and len(seen) == 2 and b"".join(seen) == want[:len(seen[0]) + len(seen[1])] and nb.value == len(want)
    with pytest.raises(IsleHipError):
        hp._chk(rc)
    assert hp.infer_text("entries") == want                                       # a following full call is correct


def test_write_infer_text_streams_into_a_file(hp, tmp_path):
    case = ic.make_case(257)
    load(hp, case)
    got = hp.infer_resident(case["M"])
    for what in ("entries", "top"):
        path = str(tmp_path / what)
        want = expected(got, what, base=1000)
        assert hp.write_infer_text(path, what, base=1000) == (len(want), want.count(b"\n")) and open(path, "rb").read() == want


# ---- 6. validity ---------------------------------------------------------------------------------------------------------------
def test_validity():
    case = ic.make_case(7)
    h = HotPath(0)
    try:
        for what in ("entries", "top"):
            with pytest.raises(IsleHipError):
                h.infer_text(what, rows=(0, 0))                                     # before any infer_resident
        D = load(h, case)
        with pytest.raises(IsleHipError):
            h.infer_text("entries", rows=(0, 0))
        got = h.infer_resident(case["M"], docs=(2, D))
        before = h.infer_entries(D - 2, got["nentries"])
        assert h.infer_text("entries") == expected(got, "entries") and h.infer_text("top", base=2) == expected(got, "top", base=2)
        after = h.infer_entries(D - 2, got["nentries"])
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        for bad in (dict(rows=(3, 2)), dict(rows=(0, D - 1)), dict(what=2), dict(what=-1)):   # row_end beyond the resident rows; unknown kinds
            seen = []
            with pytest.raises(IsleHipError):
                h._infer_text_call(bad.get("what", "entries"), bad.get("rows"), 1, lambda mv: seen.append(bytes(mv)))
            assert seen == []
        assert h.infer_text("entries", rows=(0, D - 2)) == expected(got, "entries")
        load(h, case)                                                              # a new A voids the result
        for what in ("entries", "top"):
            with pytest.raises(IsleHipError):
                h.infer_text(what)
    finally:
        h.close()


# ---- 7. the C++ yardstick ------------------------------------------------------------------------------------------------------
def test_device_text_equals_the_cpp_host_loops(hp, tmp_path):
    case = ic.make_case(257)
    D = load(hp, case)
    got = hp.infer_resident(case["M"])
    dumps = {"entries": [got["offs"].astype(np.int64), got["topic"].astype(np.uint32), got["weight"].astype(np.float32)],
             "top": [got["top_topic"].astype(np.int32), got["top_weight"].astype(np.float32)]}
    for what, arrays in dumps.items():
        src, out = str(tmp_path / (what + ".bin")), str(tmp_path / (what + ".txt"))
        with open(src, "wb") as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        r = subprocess.run([os.path.join(HOST, "infer_text_main"), what, src, str(D), "7", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        host = open(out, "rb").read()
        dev = hp.infer_text(what, base=7)
        assert len(dev) == len(host) and dev == host and host == expected(got, what, base=7) and host


# ---- 8. ISLEInfer over a range that spans two output files ---------------------------------------------------------------------------
def test_isleinfer_writes_two_files(hp, tmp_path):
    V, k, D, first = 50, 3, 1_000_001, 5
    rng = np.random.default_rng(12)
    M = rng.random((V, k)) ** 3
    M[::7] = 0                                                                   # words no topic holds: their documents do not converge
    M = np.floor(M / M.sum(axis=0) * 1e6) / 1e6
    model = "".join("%d\t%d\t%.6f\n" % (t + 1, w + 1, M[w, t]) for t in range(k) for w in range(V) if M[w, t] > 1e-8)
    model_file = str(tmp_path / "M_hat_catch_sparse")
    open(model_file, "w").write(model)
    word = rng.integers(0, V, size=D).astype(np.int64)
    word[D - 1] = 1                                                              # the one document of the second file converges
    count = rng.integers(1, 4, size=D).astype(np.int64)
    doc = np.arange(D, dtype=np.int64) + first
    parts = [_uint_field(doc, 10), _const(D, " "), _uint_field(word + 1, 10), _const(D, " "), _uint_field(count, 10), _const(D, "\n")]
    tdf = str(tmp_path / "docs.tdf")
    with open(tdf, "wb") as f:
        f.write(np.hstack([p[0] for p in parts])[np.hstack([p[1] for p in parts])].tobytes())
    out = str(tmp_path / "out")
    os.mkdir(out)
    args = [os.path.join(HOST, "ISLEInfer"), model_file, tdf, out, str(k), str(V), str(first), str(first + D), str(D), str(model.count("\n")), "0", "0"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = ["top_topics_iters_15_Lf_10.000000_doc_%d_to_%d" % (first + a, first + b) for a, b in ((0, 1_000_000), (1_000_000, D))]
    assert sorted(os.listdir(out)) == sorted(names)
    hp.load_model_text(model.encode(), V, k)
    hp.upload_counts(V, count.astype(np.float32), word.astype(np.uint32), np.arange(D + 1, dtype=np.int64))
    got = hp.infer_resident("loaded")
    assert 0 < got["nconverged"] < D and got["top_topic"][D - 1, 0] >= 0          # the second file is not empty
    assert "Number of docs for which inference converged: %d (of %d)" % (got["nconverged"], D) in r.stdout
    for name, rows in zip(names, ((0, 1_000_000), (1_000_000, D))):
        want = expected(got, "top", base=first, rows=rows)
        text = open(os.path.join(out, name), "rb").read()
        assert len(text) == len(want) and text == want and want
        assert hp.infer_text("top", rows=rows, base=first) == want
