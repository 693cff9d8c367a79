"""The dense model writer of the trainer mirror (trainer_detail::write_dense, isle_amd/host/trainer_hip.h: DenseMatrix::write_to_file
with ftoa_mv, src/denseMatrix.cpp:124-151, include/utils.h:421-466) restated in Python, checked against strings the writer produces.
tests/test_gpu_trainer_avg_model.py parses M_hat_avg with it."""
import numpy as np
import pytest


def entry_text(w):
    """One entry as the writer emits it: "0.0" for zero, "nan" for NaN, else the integer part (its six low digits), '.', and six
    fraction digits peeled off by multiplying the float32 remainder by ten, truncating."""
    w = np.float32(w)
    if np.isnan(w):
        return "nan"
    if w == 0:
        return "0.0"
    whole = int(w)
    head = str(whole) if whole < 10 ** 6 else str(whole % 10 ** 6).rjust(6, "0")
    rest = np.float32(w - np.float32(whole))
    digits = []
    for _ in range(6):
        rest = np.float32(rest * np.float32(10))
        d = int(rest)
        digits.append(str(d))
        rest = np.float32(rest - np.float32(d))
    return head + "." + "".join(digits)


def dense_text(M):
    """The whole file for a (V, k) model: one topic per line, every entry followed by a tab."""
    M = np.asarray(M, np.float32)
    return "".join("".join(entry_text(x) + "\t" for x in M[:, t]) + "\n" for t in range(M.shape[1]))


KNOWN = [(0.0, "0.0"), (-0.0, "0.0"), (0.5, "0.500000"), (0.1, "0.100000"), (1.0, "1.000000"), (123.456, "123.456001"),
         (1e-7, "0.000000"), (3.3333333e-5, "0.000033"), (0.99999994, "0.999999"), (1234567.875, "234567.875000"),
         (2.5e-3, "0.002499"), (0.7, "0.700000"), (42.0, "42.000000"), (float("nan"), "nan")]


@pytest.mark.parametrize("w,text", KNOWN)
def test_entry_text_matches_the_writer(w, text):
    assert entry_text(w) == text


def test_dense_text_layout():
    M = np.array([[0.5, 0.0], [0.25, np.nan]], np.float32)
    assert dense_text(M) == "0.500000\t0.250000\t\n0.0\tnan\t\n"
