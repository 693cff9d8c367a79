"""Model files formatted on the device (isle_hip_model_text / isle_hip_edge_topics_text; HotPath.model_text, write_model,
model_text_size, edge_topics_text; isle_amd/csrc/model_text.hip).

Yardsticks: the vectorised numpy restatement of the two layouts in tests/test_model_text_cpu.py (tied there to the Python restatement
of the C++ writer and to the library's host formatter) and, through isle_amd/host/model_text_main, the bytes of the C++ host writers
themselves (trainer_detail::write_dense_as_sparse / write_dense).  Every comparison is byte equality of the whole text.

The text leaves the library in pieces of at most CHUNK = 16 MiB (ISLE_TEXT_CHUNK_BYTES, isle_amd/csrc/common.h): whole columns, a
longer column split between tiles of 1024 rows.  The (2 500 003, 1) shapes put more than that into one column (a split inside a
column), (5000, 1031) puts several whole columns into each of several pieces, the edge test formats several pieces as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from isle_amd import IsleHipError
from isle_amd.hot_path import catchword_rank, model_rank_threshold
from test_model_text_cpu import TINY, dense_text_np, random_domain_floats, sparse_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "model_text_main")
CHUNK = 16 << 20
RESTATE = {"sparse": sparse_text, "dense": dense_text_np}
SHAPES = [(1, 1), (1, 7), (4097, 3), (1_000_003, 2), (5000, 1031), (2_500_003, 1)]


def simplex(V, cols, seed):
    """random columns on the simplex, like a real model, a third of the entries exactly zero"""
    rng = np.random.default_rng(seed)
    M = rng.random((V, cols), np.float32) ** 4
    M[rng.random((V, cols), np.float32) < 0.33] = 0
    M /= np.maximum(M.sum(axis=0, keepdims=True), np.float32(1e-30))
    return np.asfortranarray(M, np.float32)


def torture(V, cols, seed):
    """uniform random bits over the writer's domain (NaN included) mixed with zeros, -0, and values around 1e-8f; one all-zero column"""
    rng = np.random.default_rng(seed)
    M = random_domain_floats(V * cols, seed).reshape(V, cols).copy()
    r = rng.random((V, cols))
    M[r < 0.15] = 0
    M[(r >= 0.15) & (r < 0.2)] = -0.0
    near = (r >= 0.2) & (r < 0.3)
    tb = int(TINY.view(np.uint32))
    M[near] = (tb + rng.integers(-3, 4, size=int(near.sum()))).astype(np.uint32).view(np.float32)
    if cols >= 3:
        M[:, cols // 2] = 0
    return np.asfortranarray(M, np.float32)


def pieces_of(hp, which, fmt):
    got = []
    n = hp._model_text_call(which, fmt, lambda mv: got.append(bytes(mv)))
    return got, n


@pytest.mark.parametrize("content", ["simplex", "torture"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_model_both_formats(hp, shape, content):
    V, cols = shape
    M = simplex(V, cols, seed=V + cols) if content == "simplex" else torture(V, cols, seed=V + 3 * cols)
    for fmt in ("sparse", "dense"):
        want = RESTATE[fmt](M)
        got, (nbytes, nentries) = pieces_of(hp, M, fmt)
        assert all(len(p) > 0 for p in got) and all(len(p) <= CHUNK for p in got)
        text = b"".join(got)
        assert len(text) == len(want) and text == want, (shape, content, fmt)
        assert len(got) == (len(want) > 0) if len(want) <= CHUNK else len(got) >= 2   # no call for no bytes, one piece up to the bound
        with np.errstate(invalid="ignore"):
            entries = int((M > TINY).sum()) if fmt == "sparse" else M.size   # the dense writer emits every entry
        assert (nbytes, nentries) == (len(want), entries)
        assert hp.model_text_size(M, fmt) == (nbytes, nentries)          # the size query alone
        assert hp.model_text(M, fmt) == text                             # a second call: the same bytes
    if shape == (2_500_003, 1):
        assert len(dense_text_np(M)) > CHUNK                             # one column longer than a piece: split between tiles
    if shape == (5000, 1031):
        assert len(dense_text_np(M)) > 2 * CHUNK                         # several whole-column pieces


def one_row_columns():
    """a 1 x 64 dense model of exact zeros, NaN and weights of one to seven whole digits: every column is one tile of 5 or 10 to 15 bytes"""
    vals = np.array([0.0, np.nan, 0.5, 12.25, 345.125, 6789.5, 12345.75, 999999.9, 1000001.5], np.float32)
    return np.asfortranarray(vals[np.random.default_rng(3).integers(0, vals.size, size=64)][None, :])


def test_every_store_alignment_of_the_smallest_tiles(hp):
    """The store path out of LDS (mt_store_tile, isle_amd/csrc/text_format.h) at every alignment of a tile's first byte modulo 16, and
    for a tile that owns no whole 16-byte line and shares its only one with both neighbours."""
    M = one_row_columns()
    want = dense_text_np(M)
    ends = np.flatnonzero(np.frombuffer(want, np.uint8) == ord("\n")) + 1   # V = 1: a column is a tile is a line
    starts = np.concatenate([[0], ends[:-1]])
    assert len(ends) == 64 and set(ends - starts) <= {5, 10, 11, 12, 13, 14, 15}
    assert set(int(x) % 16 for x in starts) == set(range(16))
    inside = (starts // 16 == (ends - 1) // 16) & (starts % 16 != 0) & (ends % 16 != 0)
    assert inside[1:-1].any()
    assert hp.model_text(M, "dense") == want


@pytest.mark.parametrize("fmt", ["sparse", "dense"])
def test_a_second_tile_of_one_row_in_every_column(hp, fmt):
    M = torture(1025, 3, seed=11)
    assert hp.model_text(M, fmt) == RESTATE[fmt](M)


def test_all_skipped_model_gives_no_bytes_and_no_sink_call(hp):
    M = np.asfortranarray(np.full((3000, 5), 1e-9, np.float32))
    M[::3] = 0
    M[1::7] = np.nan
    got, n = pieces_of(hp, M, "sparse")
    assert got == [] and n == (0, 0)
    assert hp.model_text(np.zeros((17, 0), np.float32, order="F"), "dense") == b""
    assert hp.model_text(M, "dense") == dense_text_np(M)


def test_pieces_are_consecutive_and_the_text_does_not_depend_on_the_split(hp, tmp_path):
    M = torture(5000, 1031, seed=77)
    got, (nbytes, _) = pieces_of(hp, M, "dense")
    assert len(got) >= 3 and sum(map(len, got)) == nbytes
    want = dense_text_np(M)
    at = 0
    for p in got:                                                          # each piece is the next stretch of the file
        assert p == want[at:at + len(p)]
        at += len(p)
    # the columns formatted on their own, in groups that split the text elsewhere, concatenate to the same sparse file only after
    # renumbering — so compare group texts with the restatement's, which pins the piece boundaries as irrelevant
    for lo, hi in ((0, 100), (100, 1031)):
        assert hp.model_text(M[:, lo:hi], "dense") == dense_text_np(M[:, lo:hi])
    path = str(tmp_path / "model.dense")
    assert hp.write_model(path, M, "dense")[0] == nbytes and open(path, "rb").read() == want


@pytest.mark.parametrize("content", ["simplex", "torture"])
def test_device_text_equals_the_cpp_host_writer(tmp_path, content):
    for V, cols in [(1, 1), (4097, 3), (1_000_003, 2), (5000, 1031), (2_500_003, 1)]:
        M = simplex(V, cols, seed=5) if content == "simplex" else torture(V, cols, seed=6)
        src, base = str(tmp_path / "m.f32"), str(tmp_path / "m")
        M.reshape(-1, order="F").tofile(src)
        r = subprocess.run([EXE, src, str(V), str(cols), base], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        for fmt in ("sparse", "dense"):
            dev, host = open(base + ".dev." + fmt, "rb").read(), open(base + ".host." + fmt, "rb").read()
            assert len(dev) == len(host) and dev == host, (V, cols, fmt)
            assert host == RESTATE[fmt](M)                                  # and the restatement is the C++ writer's text


def resident(hp, V=3000, D=6000, k=12, seed=4):
    from tools.synth import Corpus
    c = Corpus(V, D, k, seed)
    cnt, rows, offs = c.A()
    hp.upload_counts(V, cnt, rows, offs)
    hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    assign = (c.planted()[oc] % (k - 1)).astype(np.uint32)                 # topic k - 1 stays empty: a NaN column in the average model
    hp.find_catchwords(k, max(catchword_rank(D, k), 1), assign=assign, fetch_thresholds=False)
    catch = hp.construct_topic_model(k, max(model_rank_threshold(D, k), 1), D, fetch_sums=False)["model"]
    avg = hp.avg_topic_model(k)
    return catch, avg


def test_resident_models_and_edge_topics(hp, tmp_path):
    k = 12
    catch, avg = resident(hp, k=k)
    assert np.isnan(avg[:, k - 1]).all() and not np.isnan(avg[:, :k - 1]).any()
    assert hp.model_text("catch", "sparse") == sparse_text(catch)
    assert hp.model_text("catch", "dense") == dense_text_np(catch)
    assert hp.model_text("avg", "dense") == dense_text_np(avg)
    assert b"nan\tnan\t" in hp.model_text("avg", "dense")
    assert hp.model_text("avg", "sparse") == sparse_text(avg)
    assert hp.model_text_size("catch", "sparse") == (len(sparse_text(catch)), int((catch > TINY).sum()))

    rng = np.random.default_rng(9)
    pairs = rng.integers(0, k, size=(2500, 2)).astype(np.int64)
    E = hp.edge_topics(pairs, 0.7)
    for fmt in ("sparse", "dense"):
        want = RESTATE[fmt](E)
        got = []
        n = hp._text_call(lambda sink, nb, ne: hp._lib.isle_hip_edge_topics_text(hp._h, pairs.ctypes.data_as(C.c_void_p), pairs.shape[0], 0.7,
                                                                                 {"sparse": 0, "dense": 1}[fmt], sink, None, nb, ne),
                          lambda mv: got.append(bytes(mv)))
        assert len(want) > CHUNK and len(got) >= 2, "the edge text must span several pieces"
        assert b"".join(got) == want and n[0] == len(want)
        assert hp.edge_topics_text(pairs, 0.7, fmt) == want
    path = str(tmp_path / "EdgeModel_sparse")
    nb, ne = hp.edge_topics_text(pairs, 0.7, "sparse", path=path)
    assert open(path, "rb").read() == sparse_text(E) and nb == os.path.getsize(path) and ne == int((E > TINY).sum())
    assert hp.edge_topics_text(pairs[:0], 0.7) == b""
    assert hp.edge_topics_text(pairs[:3], 0.25, "sparse") == sparse_text(hp.edge_topics(pairs[:3], 0.25))


def load_sparse_model(path, num_topics, vocab_size):
    """read_sparse_model of isle_amd/host/ISLEInfer.cpp (base 1): three blank-separated fields per line, topic, word, weight; the weight's
    digits before and after the point accumulated one at a time in float, combined as (float)(before + after * 0.1^places).
    -> model_by_word (vocab, topics) and the (word, topic) positions in file order."""
    M = np.zeros((vocab_size, num_topics), np.float32)
    pos = []
    for ln in open(path, "rb").read().split(b"\n"):
        if not ln:
            continue
        t, w, x = ln.split()
        before, after = x.split(b".")
        vb = va = np.float32(0)
        for ch in before:
            vb = np.float32(vb * np.float32(10) + np.float32(ch - 48))
        for ch in after:
            va = np.float32(va * np.float32(10) + np.float32(ch - 48))
        assert 1 <= int(t) <= num_topics and 1 <= int(w) <= vocab_size
        M[int(w) - 1, int(t) - 1] = np.float32(float(vb) + float(va) * 0.1 ** len(after))
        pos.append((int(w) - 1, int(t) - 1))
    return M, pos


def test_sparse_file_round_trip_through_the_inference_loader(hp, tmp_path):
    k = 12
    catch, _ = resident(hp, k=k)
    V = catch.shape[0]
    path = str(tmp_path / "M_hat_catch_sparse")
    nbytes, nentries = hp.write_model(path, "catch", "sparse")
    assert os.path.getsize(path) == nbytes
    loaded, pos = load_sparse_model(path, k, V)
    with np.errstate(invalid="ignore"):
        emitted = catch > TINY
    assert len(pos) == nentries == int(emitted.sum()) and len(set(pos)) == len(pos)
    at = np.zeros((V, k), bool)
    at[tuple(np.array(pos).T)] = True
    assert np.array_equal(at, emitted)                                     # the file's (topic, word) positions are exactly the emitted ones
    want = np.zeros((V, k), np.float32)
    for ln in open(path).read().split("\n")[:-1]:
        t, w, x = ln.split("\t")
        whole, frac = x.split(".")
        assert len(frac) == 6
        want[int(w) - 1, int(t) - 1] = np.float32(int(whole) + int(frac) * 0.1 ** 6)
    assert np.array_equal(loaded, want)
    # a non-zero of the loaded model sits at an emitted position, and every emitted position whose text is not all zeros is one
    assert not (loaded != 0)[~emitted].any() and np.array_equal(loaded != 0, emitted & (want != 0))
    assert np.abs(loaded - np.where(emitted, catch, 0)).max() <= 1.01e-6   # six truncated decimals


def test_errors_deliver_nothing(hp):
    k = 12
    resident(hp, k=k)
    M = simplex(2000, 4, seed=1)

    def refused(call):
        got = []
        with pytest.raises(IsleHipError) as e:
            call(lambda mv: got.append(bytes(mv)))
        assert got == [] and "error -1" in str(e.value), str(e.value)       # ISLE_E_ARG
        return str(e.value)

    neg = M.copy()
    neg[1234, 2] = -0.25
    assert "column 2, row 1234" in refused(lambda sink: hp._model_text_call(neg, "dense", sink))
    assert hp.model_text(neg, "sparse") == sparse_text(np.where(neg < 0, 0, neg))   # the sparse writer skips a negative entry
    inf = M.copy()
    inf[7, 3] = np.inf
    inf[1999, 3] = np.inf
    for fmt in ("sparse", "dense"):
        assert "column 3, row 7 " in refused(lambda sink: hp._model_text_call(inf, fmt, sink))
    big = M.copy()
    big[0, 0] = 2.0 ** 31
    refused(lambda sink: hp._model_text_call(big, "sparse", sink))
    refused(lambda sink: hp._model_text_call(M, 2, sink))                   # unknown format
    refused(lambda sink: hp._text_call(lambda s, nb, ne: hp._lib.isle_hip_model_text(hp._h, 3, None, 3000, k, 0, s, None, nb, ne), sink))  # unknown model
    refused(lambda sink: hp._text_call(lambda s, nb, ne: hp._lib.isle_hip_model_text(hp._h, 0, None, 3000, k + 1, 0, s, None, nb, ne), sink))
    refused(lambda sink: hp._text_call(lambda s, nb, ne: hp._lib.isle_hip_model_text(hp._h, 0, None, 2999, k, 0, s, None, nb, ne), sink))
    from isle_amd import HotPath
    fresh = HotPath(0)
    try:
        for which in ("catch", "avg"):
            got = []
            with pytest.raises(IsleHipError):
                fresh._model_text_call(which, "sparse", lambda mv: got.append(bytes(mv)))   # a resident model that does not exist
            assert got == []
    finally:
        fresh.close()


def test_a_refusing_sink_stops_the_delivery_and_the_context_stays_usable(hp):
    M = torture(5000, 1031, seed=78)
    want = dense_text_np(M)
    assert len(want) > 2 * CHUNK                                           # at least three pieces
    seen = []

    def sink(ptr, n, user):
        seen.append(C.string_at(ptr, n))
        return 1 if len(seen) == 2 else 0

    from isle_amd.hot_path import _TEXT_SINK
    cb = _TEXT_SINK(sink)
    host = np.asfortranarray(M)
    nb = C.c_uint64()
    rc = hp._lib.isle_hip_model_text(hp._h, 2, host.ctypes.data_as(C.c_void_p), 5000, 1031, 1, C.cast(cb, C.c_void_p), None, C.byref(nb), None)
    assert rc == -1 and len(seen) == 2 and b"".join(seen) == want[:len(seen[0]) + len(seen[1])]
    assert nb.value == len(want)

    class Boom(Exception):
        pass

    def raising(mv):
        raise Boom()

    with pytest.raises(Boom):
        hp._model_text_call(M, "dense", raising)
    assert hp.model_text(M, "dense") == want                               # the context still works
