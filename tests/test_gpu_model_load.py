"""Model files read on the device into the resident model ISLE_MODEL_LOADED (isle_hip_load_model_text / isle_hip_get_loaded_model;
HotPath.load_model_text, load_model, loaded_model; isle_amd/csrc/model_load.hip).

Yardstick: tests/model_read_rule.py, the independent Python restatement of the rule in include/isle_hip.h (tied to the library's host
copy of the weight rule and to the C++ host parser in tests/test_model_read_cpu.py).  Every comparison of a model is equality of the
float bits.  V = 700 and k = 9 throughout: a sparse text of a few thousand lines spans many of the loader's 4096-byte tiles, a dense
line (about 6 KB) spans two."""
import numpy as np
import pytest

import model_read_rule as rule
from isle_amd import HotPath, IsleHipError

pytestmark = pytest.mark.gpu
V, K, TILE = 700, 9, 4096
_RULE = {}


def by_rule(text, fmt, base=1, vocab=V, cols=K):
    """the rule's parse of a text, computed once per text"""
    key = (bytes(text), fmt, base, vocab, cols)
    if key not in _RULE:
        _RULE[key] = rule.parse_sparse(text, vocab, cols, base) if fmt == "sparse" else rule.parse_dense(text, vocab, cols)
    return _RULE[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def load_and_compare(hp, text, fmt, base=1):
    want, n = by_rule(text, fmt, base)
    assert hp.load_model_text(text, V, K, fmt, base) == n
    got = hp.loaded_model()
    assert same_bits(got, want), (fmt, base, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    return got


def random_model(seed, nan_column=None):
    rng = np.random.default_rng(seed)
    M = (rng.random((V, K)) * 10.0 ** rng.integers(-7, 4, (V, K))).astype(np.float32)
    M[rng.random((V, K)) < 0.5] = 0
    if nan_column is not None:
        M[:, nan_column] = np.nan
    return np.asfortranarray(M)


@pytest.mark.parametrize("fmt", ["sparse", "dense"])
def test_writer_text_reads_back_by_the_rule(hp, fmt):
    M = random_model(1, nan_column=4 if fmt == "dense" else None)
    text = hp.model_text(M, fmt)
    assert len(text) > 8 * TILE
    got = load_and_compare(hp, text, fmt)
    if fmt == "sparse":
        assert by_rule(text, fmt)[1] == text.count(b"\n") == int((M > np.float32(1e-8)).sum())
    else:
        assert by_rule(text, fmt)[1] == V * K and (got.view(np.uint32)[:, 4] == 0x7fc00000).all() and not np.isnan(np.delete(got, 4, 1)).any()
        assert max(map(len, text.split(b"\n"))) > TILE                    # a line spans tiles


def digits(rng, n):
    return "".join(map(str, rng.integers(0, 10, n)))


def hand_made_lines(seed, n=1500):
    """lines valid under base 0 and base 1, with every liberty the format allows; weights of 8-14 digits on either side of the point"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w = digits(rng, int(rng.integers(8, 15))) + "." + digits(rng, int(rng.integers(0, 3))) if i % 2 else \
            digits(rng, int(rng.integers(0, 2))) + "." + digits(rng, int(rng.integers(8, 15)))
        sep = [" ", "\t", "  \t ", "\t\t", " \r "]
        ln = ["", "  ", "\t"][i % 3] + str(rng.integers(1, K)) + sep[i % 5] + str(rng.integers(1, V)) + sep[(i // 5) % 5] + w + ["", " ", " \t"][i % 3]
        out.append(ln.encode() + (b"\r" if i % 4 == 0 else b""))
        if i % 97 == 0:
            out.append([b"", b"  \t", b"\r"][i % 3])                          # blank lines
    return out


def test_hand_made_sparse_text(hp):
    lines = hand_made_lines(2)
    text = b"\n".join(lines)
    assert not text.endswith(b"\n") and len(text) > 8 * TILE
    for base in (0, 1):
        load_and_compare(hp, text, "sparse", base)
    assert not same_bits(by_rule(text, "sparse", 0)[0], by_rule(text, "sparse", 1)[0])
    # the same lines padded with blank lines to a whole number of tiles: the last tile is full, with and without a final newline
    half = len(lines) // 2
    for tail in (b"\n", b""):
        head, rest = b"\n".join(lines[:half]) + b"\n", b"\n".join(lines[half:]) + tail
        padded = head + b"\n" * (-(len(head) + len(rest)) % TILE) + rest
        assert len(padded) % TILE == 0 and padded.endswith(b"\n") == bool(tail)
        got = load_and_compare(hp, padded, "sparse", 1)
        assert same_bits(got, by_rule(text, "sparse", 1)[0])


def test_the_last_line_naming_a_cell_wins(hp):
    rng = np.random.default_rng(3)
    cells = rng.permutation(V * K)[:6000]
    lines = [b"%d\t%d\t%d.%06d" % (c // V + 1, c % V + 1, rng.integers(0, 50), rng.integers(0, 10 ** 6)) for c in cells]
    t, w = cells[10] // V + 1, cells[10] % V + 1                              # named again twice, far away, next to each other
    lines[5000:5000] = [b"%d %d 111.5" % (t, w), b"%d %d 222.25" % (t, w)]
    text = b"\n".join(lines) + b"\n"
    start = [0] + list(np.cumsum([len(x) + 1 for x in lines]))
    assert start[10] // TILE != start[5000] // TILE and start[5000] // TILE == start[5001] // TILE and len(lines) - 10 > 5000
    first = load_and_compare(hp, text, "sparse")
    assert first[w - 1, t - 1] == np.float32(222.25)
    assert hp.load_model_text(text, V, K, "sparse") == len(lines) and same_bits(hp.loaded_model(), first)
    # ... and the earlier line wins nothing by coming later in another order of the same lines
    lines[5000], lines[5001] = lines[5001], lines[5000]
    assert load_and_compare(hp, b"\n".join(lines), "sparse")[w - 1, t - 1] == np.float32(111.5)


def valid_sparse_lines(n=700):
    rng = np.random.default_rng(4)
    return [b"%d\t%d\t0.%06d" % (rng.integers(1, K + 1), rng.integers(1, V + 1), rng.integers(1, 10 ** 6)) for _ in range(n)]


def valid_dense_lines():
    return [b"\t".join(b"0.%06d" % x for x in np.random.default_rng(5 + t).integers(0, 10 ** 6, V)) + b"\t" for t in range(K)]


SPARSE_ERRORS = {
    "bad character": b"3 17 0.5x",
    "too many fields": b"3 17 0.5 1",
    "too few fields": b"3 17",
    "id zero or out of range": b"0 17 0.5",
    "token too long": b"3 17 0." + b"1" * 63,
}


def error_texts():
    """(format, text, line, kind): every kind of error on two lines that lie in different tiles; the earlier one is to be named"""
    out = []
    for kind, bad in SPARSE_ERRORS.items():
        lines = valid_sparse_lines()
        lines[200], lines[600] = bad, (b"1 %d 0.5" % (V + 1) if kind.startswith("id") else bad)
        out.append(("sparse", b"\n".join(lines) + b"\n", 201, kind))
    for kind, edit in (("wrong token count", lambda ln: ln[:-9]), ("wrong token count", lambda ln: ln + b"0.5\t"),
                       ("bad character", lambda ln: ln.replace(b"\t0.", b"\t0,", 3)), ("token too long", lambda ln: b"0." + b"7" * 63 + b"\t" + ln[9:])):
        lines = valid_dense_lines()
        lines[2], lines[6] = edit(lines[2]), edit(lines[6])
        out.append(("dense", b"\n".join(lines) + b"\n", 3, kind))
    lines = valid_sparse_lines()                                              # the limits that keep the parser's walks short
    lines[200], lines[600] = b" " * 4090 + lines[200], b"\t" * 5000
    out.append(("sparse", b"\n".join(lines) + b"\n", 201, "bad character"))
    lines = valid_dense_lines()
    lines[2], lines[6] = lines[2][:3000] + b"\r" * 65 + lines[2][3000:], lines[6] + b"\r" * 200
    out.append(("dense", b"\n".join(lines) + b"\n", 3, "bad character"))
    out.append(("dense", b"\n".join(valid_dense_lines()[:-1]) + b"\n", K - 1, "wrong line count"))
    out.append(("dense", b"\n".join(valid_dense_lines() + valid_dense_lines()[:1]), K + 1, "wrong line count"))
    return out


def test_nothing_is_loaded_before_the_first_load():
    hp = HotPath(0)
    try:
        hp.upload_counts(V, np.ones(2, np.float32), np.array([0, 1], np.uint32), np.array([0, 2], np.int64))
        with pytest.raises(IsleHipError):
            hp.loaded_model()
        for call in (lambda: hp.model_top_words(1, "loaded"), lambda: hp.topic_diversity(1, "loaded"), lambda: hp.model_text("loaded", "sparse"),
                     lambda: hp.infer_resident("loaded")):
            with pytest.raises(IsleHipError, match="no loaded model"):
                call()
    finally:
        hp.close()


def test_errors_name_the_first_offending_line_and_leave_the_loaded_model(hp):
    good = b"\n".join(valid_sparse_lines()) + b"\n"
    kept = load_and_compare(hp, good, "sparse")
    for fmt, text, line, kind in error_texts():
        with pytest.raises(rule.ModelReadError) as want:
            by_rule(text, fmt)
        assert (want.value.line, want.value.kind) == (line, kind), (fmt, kind, str(want.value))
        if fmt == "sparse":
            at = [i for i, ln in enumerate(text.split(b"\n")) if ln in (SPARSE_ERRORS[kind], b"1 %d 0.5" % (V + 1)) or len(ln) > 4096]
            first, second = (len(b"\n".join(text.split(b"\n")[:i])) for i in at)
            assert first // TILE != second // TILE
        with pytest.raises(IsleHipError, match="line %d: %s" % (line, kind)):
            hp.load_model_text(text, V, K, fmt)
        assert same_bits(hp.loaded_model(), kept)
    for bad_call in (lambda: hp.load_model_text(good, 0, K), lambda: hp.load_model_text(good, V, 0), lambda: hp.load_model_text(good, V, K, base=2),
                     lambda: hp.load_model_text(good, V, K, format=2)):
        with pytest.raises(IsleHipError):
            bad_call()
    assert same_bits(hp.loaded_model(), kept)
    load_and_compare(hp, b"\n".join(valid_dense_lines()), "dense")            # the context is usable: a valid load succeeds


def test_consumers_take_the_loaded_model(hp):
    from test_gpu_avg_model import check_diversity
    from test_gpu_infer import make_case
    D = 300
    M0, offs, rows, counts = make_case(V, K, D, 9)
    hp.upload_counts(V, counts, rows, offs)
    text = hp.model_text(M0, "sparse")
    M = load_and_compare(hp, text, "sparse")
    for chunk in (0, 64):
        got, want = hp.infer_resident("loaded", chunk_docs=chunk), hp.infer_resident(M, chunk_docs=chunk)
        assert got["nconverged"] == want["nconverged"] > 0 and got["nentries"] == want["nentries"] > 0
        for name in ("top_topic", "top_weight", "llh", "offs", "topic", "weight"):
            assert got[name].tobytes() == want[name].tobytes(), (chunk, name)
    for n in (1, 10):
        ids, w = hp.model_top_words(n, "loaded", with_weights=True)
        ids2, w2 = hp.model_top_words(n, M, with_weights=True)
        assert np.array_equal(ids, ids2) and same_bits(w, w2)
    for fmt in ("sparse", "dense"):
        assert hp.model_text("loaded", fmt) == hp.model_text(M, fmt)
        assert hp.model_text_size("loaded", fmt) == hp.model_text_size(M, fmt)
    check_diversity(M, hp.topic_diversity(K, "loaded"))
    with pytest.raises(IsleHipError):
        hp.topic_diversity(K + 1, "loaded")                                   # not the loaded model's columns
    hp.load_model_text(b"1 1 0.5\n", V + 1, K)
    with pytest.raises(IsleHipError):
        hp.infer_resident("loaded")                                           # not A's vocabulary


def test_the_loaded_model_is_independent_of_the_other_resident_state(hp, tmp_path):
    from test_gpu_model_text import resident
    resident(hp, k=12)
    before = hp.model_text("catch", "sparse")
    text = hp.model_text(random_model(6), "dense")
    kept = load_and_compare(hp, text, "dense")
    assert hp.model_text("catch", "sparse") == before and hp.model_text("loaded", "dense") == hp.model_text(kept, "dense")
    hp.ingest_tdf(b"1 1 2\n2 3 1\n", 3, 2)                                    # a new count matrix
    assert same_bits(hp.loaded_model(), kept)
    path = str(tmp_path / "model.dense")
    open(path, "wb").write(text)
    assert hp.load_model(path, V, K, "dense") == V * K and same_bits(hp.loaded_model(), kept)


def test_empty_input(hp):
    assert hp.load_model_text(b"", V, K, "sparse") == 0
    got = hp.loaded_model()
    assert got.shape == (V, K) and not got.view(np.uint32).any()
    assert hp.load_model_text(b"\n \r\n\t\n", V, K, "sparse") == 0
    with pytest.raises(IsleHipError, match="line 1: wrong line count"):
        hp.load_model_text(b"", V, K, "dense")
    assert not hp.loaded_model().view(np.uint32).any()
