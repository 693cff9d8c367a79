"""The triple feed (isle_hip_feed_begin / _entries / _finalize, HotPath.feed_begin / feed / feed_finalize / upload_coo) against the plain
rule of tests/feed_rule.py.  Every comparison is exact: counts (by their bits), rows, offsets, entries_fed, nnz.  Batch sizes sit at the
edges of the workgroup (256) and of the radix tile (2048); the shapes move wbits + dbits across 16 and 24, where the number of radix
passes changes."""
import re

import numpy as np
import pytest

from feed_rule import BASE_D, BASE_V, base_corpus, feed_rule
from ingest_rule import text_from_entries
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    d, w, c = base_corpus()
    return dict(d=d, w=w, c=c, want=feed_rule(d, w, c, BASE_D))


def batches_of(d, w, c, size):
    size = len(d) if size is None else size
    return [(d[a:a + size], w[a:a + size], c[a:a + size]) for a in range(0, len(d), max(size, 1))]


def feed_all(hp, V, D, batches, reserve=0, **fin):
    hp.feed_begin(V, D, reserve)
    for b in batches:
        hp.feed(*b)
    return hp.feed_finalize(**fin)


def assert_exact(hp, got, want, entries_fed):
    counts, rows, offs = want
    assert got == (entries_fed, len(counts))
    gc, gr, go = hp.get_A()
    np.testing.assert_array_equal(go, offs)
    np.testing.assert_array_equal(gr, rows)
    np.testing.assert_array_equal(gc.view(np.uint32), counts.view(np.uint32))


def check(hp, V, D, d, w, c, size=None, reserve=0):
    d, w, c = (np.asarray(x) for x in (d, w, c))
    got = feed_all(hp, V, D, batches_of(d, w, c, size), reserve)
    assert_exact(hp, got, feed_rule(d, w, c, D), int(np.count_nonzero(c)))


# ---- batching ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [255, 256, 257, 2047, 2048, 2049, None])
def test_any_batching_gives_the_same_bytes(hp, base, size):
    got = feed_all(hp, BASE_V, BASE_D, batches_of(base["d"], base["w"], base["c"], size))
    assert_exact(hp, got, base["want"], int(np.count_nonzero(base["c"])))


def test_batches_of_one(hp, base):
    check(hp, BASE_V, BASE_D, base["d"][:300], base["w"][:300], base["c"][:300], size=1)


def test_an_empty_batch_between_two_others(hp, base):
    d, w, c = base["d"], base["w"], base["c"]
    e = np.zeros(0, np.uint32)
    got = feed_all(hp, BASE_V, BASE_D, [(d[:1000], w[:1000], c[:1000]), (e, e, e), ([], [], []), (d[1000:], w[1000:], c[1000:])])
    assert_exact(hp, got, base["want"], int(np.count_nonzero(c)))


@pytest.mark.parametrize("first,second", [(11, 22), (22, 11)])
def test_of_a_pair_split_across_batches_the_earlier_batch_wins(hp, first, second):
    got = feed_all(hp, 10, 10, [([3, 1], [7, 2], [first, 5]), ([0, 3], [0, 7], [4, second])])
    assert got == (4, 3)
    counts, rows, offs = hp.get_A()
    assert counts.tolist() == [4.0, 5.0, float(first)] and rows.tolist() == [0, 2, 7]
    assert offs.tolist() == [0, 1, 2, 2, 3, 3, 3, 3, 3, 3, 3]


@pytest.mark.parametrize("reserve", [0, 16])
def test_the_store_grows_and_keeps_what_it_held(hp, base, reserve):
    got = feed_all(hp, BASE_V, BASE_D, batches_of(base["d"], base["w"], base["c"], 700), reserve)
    assert_exact(hp, got, base["want"], int(np.count_nonzero(base["c"])))


# ---- shape edges ------------------------------------------------------------------------------
def edge_entries(V, D, seed, n=300):
    rng = np.random.default_rng(seed)
    d, w = rng.integers(0, D, n), rng.integers(0, V, n)
    d[:4], w[:4] = [0, D - 1, 0, D - 1], [0, V - 1, V - 1, 0]
    d[4:12], w[4:12] = np.tile(d[:4], 2), np.tile(w[:4], 2)        # the corners twice more, under other counts
    c = rng.integers(1, 1000, n)
    c[20:26] = 0
    return d, w, c


def test_one_word(hp):
    check(hp, 1, 50, *edge_entries(1, 50, 1), size=64)


def test_one_document(hp):
    check(hp, 50, 1, *edge_entries(50, 1, 2), size=64)


@pytest.mark.parametrize("V", [256, 257])
@pytest.mark.parametrize("D", [255, 256, 257, 65536, 65537])
def test_key_widths_around_16_and_24_bits(hp, V, D):
    check(hp, V, D, *edge_entries(V, D, V + D), size=128)


def test_empty_documents_at_the_front_in_the_middle_and_at_the_end(hp):
    rng = np.random.default_rng(5)
    d = np.concatenate([rng.integers(5, 11, 60), rng.integers(20, 26, 60)])
    check(hp, 30, 40, d, rng.integers(0, 30, 120), rng.integers(1, 9, 120), size=50)
    offs = hp.get_A()[2]
    assert not offs[:6].any() and offs[11] == offs[20] and offs[26] == offs[40] == offs[-1]


def test_no_entries_at_all(hp):
    hp.feed_begin(7, 9)
    assert hp.feed_finalize() == (0, 0)
    counts, rows, offs = hp.get_A()
    assert len(counts) == 0 and len(rows) == 0 and len(offs) == 10 and not offs.any()


def test_a_batch_of_zero_counts_only(hp):
    got = feed_all(hp, 7, 9, [([1, 2], [3, 4], [5, 6]), ([1, 2, 8], [3, 4, 6], [0, 0, 0]), ([8], [6], [2])])
    assert_exact(hp, got, feed_rule([1, 2, 8], [3, 4, 6], [5, 6, 2], 9), 3)
    hp.feed_begin(7, 9)
    hp.feed([1, 2, 8], [3, 4, 6], [0, 0, 0])
    assert hp.feed_finalize() == (0, 0) and not hp.get_A()[2].any()


def test_the_largest_count(hp):
    got = feed_all(hp, 5, 3, [([1, 0], [2, 4], np.array([4294967295, 16777217], np.uint64))])
    assert got == (2, 2)
    assert hp.get_A()[0].tolist() == [16777216.0, 4294967296.0]


# ---- rejection --------------------------------------------------------------------------------
def rejected(hp, kind, ordinal, d, w, c):
    with pytest.raises(IsleHipError, match=re.escape("%s id out of range at entry %d " % (kind, ordinal))):
        hp.feed(d, w, c)


def test_ids_out_of_range_are_refused_with_kind_and_ordinal(hp):
    V, D = 6, 4
    hp.feed_begin(V, D)
    rejected(hp, "word", 1, [0, 1], [5, V], [1, 1])
    rejected(hp, "document", 0, [D], [0], [1])
    rejected(hp, "word", 2, [0, 1, 2, 3, D], [0, 1, V, 3, 0], [1, 1, 1, 1, 1])      # two bad entries: the lower ordinal
    rejected(hp, "document", 1, [0, D, 2, 3], [0, 1, V, 3], [1, 0, 1, 1])          # ... of either kind, under a zero count too
    assert hp.feed_finalize() == (0, 0)


def test_a_bad_entry_in_the_third_batch_counts_the_first_two_and_leaves_them_fed(hp, base):
    d, w, c = (x[:900].copy() for x in (base["d"], base["w"], base["c"]))
    assert (c[:600] == 0).any()                                                    # skipped entries count in the ordinal
    hp.feed_begin(BASE_V, BASE_D)
    hp.feed(d[:257], w[:257], c[:257])
    hp.feed(d[257:600], w[257:600], c[257:600])
    bad_w = w[600:].copy()
    bad_w[123] = BASE_V
    rejected(hp, "word", 600 + 123, d[600:], bad_w, c[600:])
    bad_d = d[600:].copy()
    bad_d[[7, 250]] = BASE_D, BASE_D + 5
    rejected(hp, "document", 600 + 7, bad_d, w[600:], c[600:])                     # the refused batch did not move the ordinal
    got = hp.feed_finalize()
    assert_exact(hp, got, feed_rule(d[:600], w[:600], c[:600], BASE_D), int(np.count_nonzero(c[:600])))


# ---- a batch cut into pieces inside the library (isle_hip_feed_entries_pieces) -------------------
@pytest.mark.parametrize("piece", [1, 255, 256, 257, 2048, 5000, 10 ** 9])
def test_the_pieces_a_batch_is_cut_into_do_not_show(hp, base, piece):
    d, w, c = (base[x][:3000] if piece == 1 else base[x] for x in "dwc")
    hp.feed_begin(BASE_V, BASE_D)
    hp.feed(d[:700], w[:700], c[:700], _piece_entries=piece)
    hp.feed(d[700:], w[700:], c[700:], _piece_entries=piece)
    assert_exact(hp, hp.feed_finalize(), feed_rule(d, w, c, BASE_D), int(np.count_nonzero(c)))


def test_a_bad_entry_in_a_later_piece_refuses_the_whole_batch(hp, base):
    d, w, c = (base[x][:2000].copy() for x in "dwc")
    hp.feed_begin(BASE_V, BASE_D)
    hp.feed(d[:300], w[:300], c[:300], _piece_entries=128)
    bad_d, bad_w = d[300:].copy(), w[300:].copy()
    bad_d[1500], bad_w[900], bad_w[901] = BASE_D, BASE_V, BASE_V + 1                # pieces 11 and 7 of the batch: the lower ordinal
    for piece in (128, 257, 900, 901, 1700):                                     # ... found in the 8th, 4th, 2nd, 1st, 1st piece
        with pytest.raises(IsleHipError, match=re.escape("word id out of range at entry %d " % (300 + 900))):
            hp.feed(bad_d, bad_w, c[300:], _piece_entries=piece)                 # the pieces before it were taken back
    bad_w[900:902] = 0
    with pytest.raises(IsleHipError, match=re.escape("document id out of range at entry %d " % (300 + 1500))):
        hp.feed(bad_d, bad_w, c[300:], _piece_entries=128)
    hp.feed(d[300:], w[300:], c[300:], _piece_entries=128)
    assert_exact(hp, hp.feed_finalize(), feed_rule(d, w, c, BASE_D), int(np.count_nonzero(c)))


# ---- state ------------------------------------------------------------------------------------
def test_calls_without_an_open_feed_fail_and_a_second_begin_starts_over(hp):
    feed_all(hp, 4, 4, [([1], [1], [1])])
    for _ in range(2):                                                             # after a finalize ... and after that failure
        with pytest.raises(IsleHipError, match="no open feed"):
            hp.feed([0], [0], [1])
        with pytest.raises(IsleHipError, match="no open feed"):
            hp.feed_finalize()
    from isle_amd import HotPath
    fresh = HotPath(0)
    try:                                                                           # ... and on a context that never had one
        with pytest.raises(IsleHipError, match="no open feed"):
            fresh.feed([0], [0], [1])
        with pytest.raises(IsleHipError, match="no open feed"):
            fresh.feed_finalize()
    finally:
        fresh.close()
    hp.feed_begin(4, 4)
    hp.feed([0, 1], [2, 3], [9, 9])
    hp.feed_begin(5, 3)
    hp.feed([2], [4], [6])
    assert_exact(hp, hp.feed_finalize(), feed_rule([2], [4], [6], 3), 1)
    with pytest.raises(IsleHipError, match="out of range"):
        hp.feed_begin(0, 3)
    with pytest.raises(IsleHipError, match="out of range"):
        hp.feed_begin(3, 0xfffffff1)


def test_the_current_matrix_stays_fetchable_while_a_feed_is_open(hp):
    counts, rows, offs = np.array([2, 3, 4], np.float32), np.array([0, 2, 1], np.uint32), np.array([0, 2, 2, 3], np.int64)
    hp.upload_counts(3, counts, rows, offs)
    hp.feed_begin(9, 9)
    hp.feed([8, 0], [8, 0], [1, 1])
    gc, gr, go = hp.get_A()
    assert gc.tolist() == counts.tolist() and gr.tolist() == rows.tolist() and go.tolist() == offs.tolist()
    assert_exact(hp, hp.feed_finalize(), feed_rule([8, 0], [8, 0], [1, 1], 9), 2)


# ---- equivalences -----------------------------------------------------------------------------
def test_tdf_ingest_of_the_same_triples_gives_the_same_matrix(hp, base):
    keep = base["c"] != 0
    d, w, c = (base[x][keep].astype(np.uint64) for x in "dwc")
    info = hp.ingest_tdf(text_from_entries(d + np.uint64(1), w + np.uint64(1), c), BASE_V, BASE_D)
    assert info == dict(entries_read=len(d), nnz=len(base["want"][0]))
    assert_exact(hp, (len(d), info["nnz"]), base["want"], len(d))


def test_thresholding_after_the_feed_equals_thresholding_after_upload_counts(hp, base):
    k = 5
    outs = []
    for how in ("feed", "upload"):
        if how == "feed":
            feed_all(hp, BASE_V, BASE_D, batches_of(base["d"], base["w"], base["c"], 1000))
        else:
            hp.upload_counts(BASE_V, *base["want"])
        info = hp.threshold(k)
        outs.append((info, hp.get_B()))
    (ia, a), (ib, b) = outs
    assert ia == ib and a["D"] == b["D"] > 0 and a["nnz"] == b["nnz"] > 0
    for name in ("vals", "rows", "offs", "original_cols", "zetas"):
        assert a[name].tobytes() == b[name].tobytes(), name


def test_doc_offset_and_docs_global_act_as_in_upload_counts(hp, base):
    k = 5
    outs = []
    for how in ("feed", "upload"):
        if how == "feed":
            feed_all(hp, BASE_V, BASE_D, batches_of(base["d"], base["w"], base["c"], None), doc_offset=5, docs_global=BASE_D + 9)
        else:
            hp.upload_counts(BASE_V, *base["want"], doc_offset=5, docs_global=BASE_D + 9)
        hp.threshold(k)
        outs.append((hp.shape(), hp.get_B()["original_cols"]))
    assert outs[0][0] == outs[1][0] and outs[0][0][0] == BASE_V
    assert np.array_equal(outs[0][1], outs[1][1]) and int(outs[0][1].min()) >= 5


# ---- upload_coo -------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1000, None])
def test_upload_coo(hp, base, batch):
    got = hp.upload_coo(BASE_V, BASE_D, base["d"].astype(np.int64), base["w"].tolist(), base["c"].astype(np.float64), batch=batch)
    assert_exact(hp, got, base["want"], int(np.count_nonzero(base["c"])))


def test_values_that_do_not_fit_32_unsigned_bits_raise_and_nothing_wraps(hp):
    for bad in ([1, -1], np.array([0, 2 ** 32], np.int64), np.array([-3], np.int32), [0.5], [2 ** 70], [float("nan")]):
        for slot in range(3):
            args = [[0, 0][:len(bad)], [0, 0][:len(bad)], [1, 1][:len(bad)]]
            args[slot] = bad
            with pytest.raises(ValueError):
                hp.upload_coo(4, 4, *args)
            hp.feed_begin(4, 4)
            with pytest.raises(ValueError):
                hp.feed(*args)
            assert hp.feed_finalize() == (0, 0)
    with pytest.raises(ValueError):
        hp.upload_coo(4, 4, [0, 1], [0], [1, 1])
