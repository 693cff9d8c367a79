"""The text form of model files (include/isle_hip.h, isle_hip_model_text): the library's host copy of the digit rule
(isle_hip_entry_text -> isle_amd.hot_path.entry_text, compiled from the same function as the kernels of isle_amd/csrc/model_text.hip)
against the Python restatement of the C++ writer in tests/test_avg_model_cpu.py, and a vectorised numpy restatement of both file
layouts (sparse_text / dense_text_np below, float32 element-wise operations), which the GPU tests import as their yardstick.  No GPU."""
import numpy as np
import pytest

from isle_amd.hot_path import entry_text
from test_avg_model_cpu import KNOWN, dense_text
from test_avg_model_cpu import entry_text as entry_text_py

TINY = np.float32(1e-8)          # the sparse writer prints w > 1e-8f
TWO31 = np.float32(2.0 ** 31)    # the writer's (int)w is undefined from here on


# ---- the vectorised restatement ------------------------------------------------------------------------------------------------
def _uint_field(v, width):
    """v (N,) non-negative ints -> ((N, width) uint8 digits right-aligned, (N, width) bool: the digits without leading zeros)."""
    v = np.asarray(v, np.int64)
    p = 10 ** np.arange(width - 1, -1, -1, dtype=np.int64)
    digits = (v[:, None] // p[None, :]) % 10
    nd = np.maximum(1, (v[:, None] >= p[None, :]).sum(axis=1))
    valid = np.arange(width)[None, :] >= (width - nd)[:, None]
    return (digits + ord("0")).astype(np.uint8), valid


def _weight_field(w):
    """w (N,) float32 inside the writer's domain -> (N, 13) uint8 "<six low digits>.<six digits>" and the mask of the bytes printed."""
    w = np.asarray(w, np.float32)
    whole = w.astype(np.int64)
    head, _ = _uint_field(whole % 10 ** 6, 6)
    nd = np.minimum(6, np.maximum(1, (whole[:, None] >= 10 ** np.arange(10, dtype=np.int64)[None, :]).sum(axis=1)))   # at most the six low digits
    valid = np.arange(6)[None, :] >= (6 - nd)[:, None]
    rest = w - whole.astype(np.float32)
    assert rest.dtype == np.float32
    frac = np.empty((w.size, 6), np.uint8)
    for place in range(6):
        rest = rest * np.float32(10)
        d = rest.astype(np.int32)
        frac[:, place] = (d + ord("0")).astype(np.uint8)
        rest = rest - d.astype(np.float32)
        assert rest.dtype == np.float32
    dot = np.full((w.size, 1), ord("."), np.uint8)
    return np.hstack([head, dot, frac]), np.hstack([valid, np.ones((w.size, 7), bool)])


def _check_domain(w, printed):
    bad = printed & ~((w >= 0) & (w < TWO31))
    if bad.any():
        raise ValueError("an entry that would be printed is negative, infinite or >= 2^31")


def _const(n, ch):
    return np.full((n, 1), ord(ch), np.uint8), np.ones((n, 1), bool)


def sparse_text(M, block=1 << 20):
    """trainer_detail::write_dense_as_sparse for a (V, cols) model -> bytes: "<col+1>\\t<row+1>\\t<weight>\\n" for every entry
    w > 1e-8f, columns ascending, rows ascending."""
    M = np.asarray(M, np.float32)
    V, cols = M.shape
    flat = M.reshape(-1, order="F")
    out = []
    for s in range(0, flat.size, block):
        w = flat[s:s + block]
        idx = np.arange(s, s + w.size, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            keep = w > TINY
        _check_domain(w, keep)
        w, idx = w[keep], idx[keep]
        parts = [_uint_field(idx // V + 1, 10), _const(w.size, "\t"), _uint_field(idx % V + 1, 10), _const(w.size, "\t"), _weight_field(w),
                 _const(w.size, "\n")]
        out.append(np.hstack([p[0] for p in parts])[np.hstack([p[1] for p in parts])].tobytes())
    return b"".join(out)


def dense_text_np(M, block=1 << 20):
    """trainer_detail::write_dense for a (V, cols) model -> bytes: one column per line, every entry followed by a tab; "0.0" for zero
    and -0, "nan" for NaN, else the weight."""
    M = np.asarray(M, np.float32)
    V, cols = M.shape
    flat = M.reshape(-1, order="F")
    out = []
    for s in range(0, flat.size, block):
        w = flat[s:s + block]
        idx = np.arange(s, s + w.size, dtype=np.int64)
        nan, zero = np.isnan(w), w == 0
        plain = ~(nan | zero)
        _check_domain(w, plain)
        body, mask = _weight_field(np.where(plain, w, np.float32(0)))
        for sel, word in ((nan, b"nan"), (zero, b"0.0")):
            body[sel, :3] = np.frombuffer(word, np.uint8)
            mask[sel, :3] = True
            mask[sel, 3:] = False
        tab = _const(w.size, "\t")
        nl = (np.full((w.size, 1), ord("\n"), np.uint8), (idx % V == V - 1)[:, None])
        out.append(np.hstack([body, tab[0], nl[0]])[np.hstack([mask, tab[1], nl[1]])].tobytes())
    return b"".join(out)


# ---- the library's host formatter against the restatement of the C++ writer ---------------------------------------------------------
def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def hand_picked():
    tiny_bits = int(TINY.view(np.uint32))
    below_one = np.nextafter(np.float32(1), np.float32(0))
    vals = [TINY, _f32(tiny_bits - 1), _f32(tiny_bits + 1), below_one, np.float32(999999.9), np.float32(1000000), np.float32(1000001.5),
            np.float32(2.0 ** 31 - 128), _f32(1), _f32(0x007fffff), _f32(0x00400000), np.float32(-0.0), np.float32(0.0), np.float32(9.999999),
            np.float32(99999.99), np.float32(123456.78)]
    return [np.float32(v) for v in vals]


def random_domain_floats(n, seed):
    """uniform random bit patterns over [0, 2^31) with NaN patterns mixed in"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, int(TWO31.view(np.uint32)), size=n, dtype=np.uint32)
    bits[rng.integers(0, n, size=n // 100)] = np.uint32(0x7fc00000)
    bits[rng.integers(0, n, size=n // 100)] = rng.integers(0x7f800001, 0x80000000, size=n // 100, dtype=np.uint32)  # other NaN payloads
    return bits.view(np.float32)


@pytest.mark.parametrize("w,text", KNOWN)
def test_known_strings(w, text):
    assert entry_text(w, "dense") == text == entry_text_py(w)


def test_dense_entries_equal_the_writer_restatement_on_random_bit_patterns():
    w = random_domain_floats(200_000, seed=11)
    assert np.isnan(w).any()
    got = [entry_text(x, "dense") for x in w]
    want = [entry_text_py(x) for x in w]
    assert got == want
    # the vectorised restatement, entry for entry, on the same sample: its text is the tab-joined strings
    assert dense_text_np(w[:, None]) == ("\t".join(want) + "\t\n").encode()


def test_hand_picked_entries():
    for w in hand_picked():
        assert entry_text(w, "dense") == entry_text_py(w), repr(w)
    assert entry_text(np.float32(1e-8), "dense") == "0.000000"
    assert entry_text(np.float32(2.0 ** 31 - 128), "dense") == "483520.000000"   # 2147483520: the six low digits
    assert entry_text(np.float32(1000000), "dense") == "000000.000000"
    assert entry_text(np.float32(1000001.5), "dense") == "000001.500000"
    assert entry_text(-0.0, "dense") == "0.0" and entry_text(_f32(1), "dense") == "0.000000"


def test_sparse_skips_exactly_what_is_not_above_the_threshold():
    w = np.concatenate([random_domain_floats(50_000, seed=12), np.array(hand_picked(), np.float32),
                        np.array([-1.0, -1e-20, -3e9, -np.inf], np.float32)])
    for x in w:
        s = entry_text(x, "sparse")
        with np.errstate(invalid="ignore"):
            printed = bool(x > TINY)
        assert (s == "") == (not printed), repr(x)
        if printed:
            assert s == entry_text(x, "dense") == entry_text_py(x)


def test_outside_the_domain_is_refused():
    for x in (np.inf, 2.0 ** 31, 3e9, 1e38):
        assert entry_text(x, "dense") == -1 and entry_text(x, "sparse") == -1
    for x in (-1.0, -1e-20, -0.5, -3e9, -np.inf):   # printed by the dense writer only: the sparse writer skips what is not > 1e-8
        assert entry_text(x, "dense") == -1 and entry_text(x, "sparse") == ""
    assert entry_text(np.nextafter(np.float32(2.0 ** 31), np.float32(0)), "dense") == "483520.000000"


def test_unknown_format_is_refused():
    import ctypes as C
    from isle_amd import load_library
    buf = C.create_string_buffer(16)
    assert load_library().isle_hip_entry_text(C.c_float(0.5), 2, buf) == -1
    assert load_library().isle_hip_entry_text(C.c_float(0.5), 1, None) == -1


def test_layouts_of_a_small_model():
    M = np.array([[0.5, 1e-9], [np.nan, 12.25], [-0.0, 0.0625]], np.float32)   # column 1: 0.5, NaN, -0; column 2: skipped, 12.25, 0.0625
    assert sparse_text(M) == b"1\t1\t0.500000\n2\t2\t12.250000\n2\t3\t0.062500\n"
    assert dense_text_np(M) == b"0.500000\tnan\t0.0\t\n0.000000\t12.250000\t0.062500\t\n"
    assert dense_text_np(M).decode() == dense_text(M)


def test_vectorised_layouts_equal_the_entrywise_writer():
    rng = np.random.default_rng(5)
    M = random_domain_floats(7 * 1031, seed=13).reshape(1031, 7)
    M[rng.integers(0, 1031, 300), rng.integers(0, 7, 300)] = 0
    M[rng.integers(0, 1031, 50), rng.integers(0, 7, 50)] = -0.0
    M[:, 3] = 0
    assert dense_text_np(M, block=1000).decode() == dense_text(M)
    want = "".join("%d\t%d\t%s\n" % (t + 1, r + 1, entry_text_py(M[r, t])) for t in range(7) for r in range(1031) if M[r, t] > TINY)
    assert sparse_text(M, block=1000).decode() == want
    assert sparse_text(np.zeros((5, 2), np.float32)) == b"" and dense_text_np(np.zeros((2, 1), np.float32)) == b"0.0\t0.0\t\n"
    with pytest.raises(ValueError):
        dense_text_np(np.array([[-1.0]], np.float32))
    with pytest.raises(ValueError):
        sparse_text(np.array([[np.inf]], np.float32))
