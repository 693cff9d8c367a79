"""The lines of the per-document topic files (include/isle_hip.h, isle_hip_infer_text): "<doc>\\t<topic>\\t<weight>\\n" as ISLEInfer's
top_topics_* files and ISLETrainer::output_doc_topic_weights' DocTopicWeights.tsv hold them.

doc_lines_text below is the vectorised numpy restatement the GPU tests (tests/test_gpu_infer_text.py) take as their yardstick.  It is
built from the fields of tests/test_model_text_cpu.py and held here, byte for byte, to
  - a plain Python transcription of the reference's MMappedOutput::concat_int + concat_float (include/utils.h:383-478), and
  - the library's host formatter isle_hip_doc_line_text (isle_amd.hot_path.doc_line_text), compiled from the functions the kernels of
    isle_amd/csrc/infer_text.hip compile.
No GPU."""
import numpy as np
import pytest

from isle_amd.hot_path import doc_line_text
from test_gpu_infer_resident import KS
from test_model_text_cpu import TWO31, _const, _uint_field, _weight_field

NUM_END = 0x7fffffff   # concat_int: assert(num < 0x7fffffff)


# ---- the vectorised restatement ------------------------------------------------------------------------------------------------
def doc_lines_text(doc_numbers, topic_numbers, weights, block=1 << 20):
    """The lines of (doc_numbers[i], topic_numbers[i], weights[i]), the numbers as printed -> bytes.  Raises ValueError where the
    reference's writers are undefined: a number >= 0x7fffffff, a weight that is negative, NaN, infinite or >= 2^31."""
    d = np.asarray(doc_numbers, np.int64).reshape(-1)
    t = np.asarray(topic_numbers, np.int64).reshape(-1)
    w = np.asarray(weights, np.float32).reshape(-1)
    assert d.shape == t.shape == w.shape
    if ((d < 0) | (d >= NUM_END) | (t < 0) | (t >= NUM_END)).any():
        raise ValueError("a printed number is >= 0x7fffffff")
    with np.errstate(invalid="ignore"):
        if not ((w >= 0) & (w < TWO31)).all():
            raise ValueError("a printed weight is negative, NaN, infinite or >= 2^31")
    out = []
    for s in range(0, w.size, block):
        n = w[s:s + block].size
        parts = [_uint_field(d[s:s + block], 10), _const(n, "\t"), _uint_field(t[s:s + block], 10), _const(n, "\t"), _weight_field(w[s:s + block]),
                 _const(n, "\n")]
        out.append(np.hstack([p[0] for p in parts])[np.hstack([p[1] for p in parts])].tobytes())
    return b"".join(out)


def entries_text(offs, topic, weight, base=1, rows=None):
    """ISLE_DOCTEXT_ENTRIES for the arrays infer_resident returned: rows (begin, end) of the CSR, row r printed as r + base."""
    offs = np.asarray(offs, np.int64)
    b, e = (0, offs.size - 1) if rows is None else rows
    doc = np.repeat(np.arange(b, e, dtype=np.int64), np.diff(offs[b:e + 1]))
    return doc_lines_text(doc + base, np.asarray(topic[offs[b]:offs[e]], np.int64) + 1, weight[offs[b]:offs[e]])


def top_text(top_topic, top_weight, base=1, rows=None):
    """ISLE_DOCTEXT_TOP: for every row the slots 0..4 in order while top_topic[row, i] >= 0."""
    tt = np.asarray(top_topic, np.int64).reshape(-1, 5)
    tw = np.asarray(top_weight, np.float32).reshape(-1, 5)
    b, e = (0, tt.shape[0]) if rows is None else rows
    tt, tw = tt[b:e], tw[b:e]
    keep = np.cumprod(tt >= 0, axis=1).astype(bool)
    doc = np.broadcast_to(np.arange(b, e, dtype=np.int64)[:, None], tt.shape)
    return doc_lines_text(doc[keep] + base, tt[keep] + 1, tw[keep])


# ---- a plain transcription of the reference's writer ---------------------------------------------------------------------------
def itoa_mv(num):
    """include/utils.h:383-410 (without the terminal)"""
    if num == 0:
        return "0"
    s, neg = [], num < 0
    num = abs(num)
    while num != 0:
        s.append(chr(num % 10 + ord("0")))
        num //= 10
    if neg:
        s.append("-")
    return "".join(reversed(s))


def concat_int(num):
    assert num < 0x7fffffff   # :416
    return itoa_mv(int(num))


def concat_float(num):
    """ftoa_mv<float> (include/utils.h:421-466) as concat_float calls it: before_dec = 6, after_dec = 6, every operation in fp32."""
    num = np.float32(num)
    if num == 0.0:
        return "0.0"
    s, neg = [], bool(num < 0.0)
    if neg:
        num = -num
    num_int = int(num)   # (unsigned int)num
    if num_int == 0:
        s.append("0")
    else:
        d = 0
        while d < 6 and num_int > 0:
            s.append(chr(num_int % 10 + ord("0")))
            num_int //= 10
            d += 1
        assert num_int == 0   # :450
    if neg:
        s.append("-")
    s.reverse()
    s.append(".")
    frac = np.float32(num - np.float32(int(num)))
    for _ in range(6):
        frac = np.float32(frac * np.float32(10))
        assert int(frac) <= 9
        s.append(chr(ord("0") + int(frac)))
        frac = np.float32(frac - np.float32(int(frac)))
    return "".join(s)


def reference_line(doc_number, topic_number, w):
    return (concat_int(doc_number) + "\t" + concat_int(topic_number) + "\t" + concat_float(w) + "\n").encode("ascii")


# ---- inputs ------------------------------------------------------------------------------------------------------------------
NUMBERS = sorted({10 ** e - 1 for e in range(1, 10)} | {10 ** e for e in range(0, 10)} | {0x7ffffffe})   # 1, 9, 10, 99, ..., 10^9, 0x7ffffffe
TOPICS = [1, 9, 10, 99, 100, 999, 1000, 1024]


def special_weights():
    out = [np.float32(1.0), np.float32(2.0 ** -126)]   # 1.0f; the smallest positive normal
    for k in KS:
        x = np.float32(1) / np.float32(k)
        out += [x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(2))]
    return np.array(out, np.float32)


def random_weights(n=100_000, seed=21):
    """uniform random bit patterns in (0, 1]"""
    bits = np.random.default_rng(seed).integers(1, 0x3f800000 + 1, size=n, dtype=np.uint32)
    return bits.view(np.float32)


def cases():
    """(numbers, topics, weights): the full product of the digit edges with the special weights, then the random weights with the
    edges cycling beside them."""
    sw = special_weights()
    d, t, w = np.meshgrid(np.array(NUMBERS, np.int64), np.array(TOPICS, np.int64), sw, indexing="ij")
    rw = random_weights()
    i = np.arange(rw.size)
    d = np.concatenate([d.reshape(-1), np.array(NUMBERS, np.int64)[i % len(NUMBERS)]])
    t = np.concatenate([t.reshape(-1), np.array(TOPICS, np.int64)[(i // len(NUMBERS)) % len(TOPICS)]])
    w = np.concatenate([w.reshape(-1), rw])
    return d, t, w


@pytest.fixture(scope="module")
def restated():
    d, t, w = cases()
    text = doc_lines_text(d, t, w, block=50_000)
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) == w.size + 1
    return d, t, w, [ln + b"\n" for ln in lines[:-1]]


def test_inputs_are_what_they_should_be():
    assert NUMBERS[:5] == [1, 9, 10, 99, 100] and NUMBERS[-3:] == [999_999_999, 10 ** 9, 0x7ffffffe] and len(NUMBERS) == 20
    rw = random_weights()
    assert rw.size == 100_000 and (rw > 0).all() and (rw <= 1).all()
    sw = special_weights()
    assert sw[0] == 1 and sw[1] == np.finfo(np.float32).tiny and sw.size == 2 + 3 * len(KS)


def test_restatement_equals_the_transcription_of_the_reference_writer(restated):
    d, t, w, lines = restated
    want = [reference_line(int(a), int(b), c) for a, b, c in zip(d, t, w)]
    assert lines == want


def test_restatement_equals_the_library_formatter(restated):
    d, t, w, lines = restated
    got = [doc_line_text(int(a), int(b), c) for a, b, c in zip(d, t, w)]
    assert got == lines


def test_known_lines():
    assert doc_line_text(1, 1, 1.0) == b"1\t1\t1.000000\n" == doc_lines_text([1], [1], [1.0])
    assert doc_line_text(0x7ffffffe, 1024, 0.5) == b"2147483646\t1024\t0.500000\n"
    assert doc_line_text(10, 7, np.float32(2.0 ** -126)) == b"10\t7\t0.000000\n"
    assert doc_line_text(0, 3, 0.125) == b"0\t3\t0.125000\n" == reference_line(0, 3, 0.125)
    assert doc_lines_text([], [], []) == b""


def test_outside_the_domain():
    bad = [(0x7fffffff, 1, 0.5), (1, 0x7fffffff, 0.5), (2 ** 32 + 1, 1, 0.5), (1, 1, -0.25), (1, 1, np.inf), (1, 1, 2.0 ** 31), (1, 1, np.nan),
           (1, 1, -np.inf)]
    for d, t, w in bad:
        assert doc_line_text(d, t, w) == -1, (d, t, w)
        with pytest.raises(ValueError):
            doc_lines_text([1, d], [1, t], [0.5, w])
    import ctypes as C
    from isle_amd import load_library
    assert load_library().isle_hip_doc_line_text(1, 1, C.c_float(0.5), None) == -1
    below = np.nextafter(np.float32(2.0 ** 31), np.float32(0))
    assert doc_line_text(0x7ffffffe, 0x7ffffffe, below) == b"2147483646\t2147483646\t483520.000000\n" == doc_lines_text([NUM_END - 1], [NUM_END - 1], [below])


def test_csr_and_slot_layouts():
    offs = np.array([0, 2, 2, 3], np.int64)
    topic = np.array([0, 6, 1023], np.uint32)
    weight = np.array([0.75, 0.25, 1.0], np.float32)
    assert entries_text(offs, topic, weight) == b"1\t1\t0.750000\n1\t7\t0.250000\n3\t1024\t1.000000\n"
    assert entries_text(offs, topic, weight, base=98, rows=(1, 3)) == b"100\t1024\t1.000000\n"
    assert entries_text(offs, topic, weight, rows=(1, 2)) == b""
    tt = np.array([[4, 2, -1, -1, -1], [-1, -1, -1, -1, -1], [0, 1, 2, 3, 5]], np.int32)
    tw = np.array([[0.5, 0.25, 0, 0, 0], [0, 0, 0, 0, 0], [0.3, 0.25, 0.2, 0.15, 0.1]], np.float32)
    assert top_text(tt, tw, base=7) == (b"7\t5\t0.500000\n7\t3\t0.250000\n" +
                                        b"".join(b"9\t%d\t%s\n" % (t + 1, concat_float(w).encode()) for t, w in zip(tt[2], tw[2])))
    tt2 = tt.copy()
    tt2[2, 2] = -1   # the walk stops at the first absent slot
    assert top_text(tt2, tw, base=7, rows=(2, 3)) == b"9\t1\t%s\n9\t2\t0.250000\n" % concat_float(np.float32(0.3)).encode()
