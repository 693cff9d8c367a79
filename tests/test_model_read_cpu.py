"""The weight rule of the model readers (include/isle_hip.h, isle_hip_parse_weight: the library's host copy of the function its loader
kernels compile) against the independent restatement of tests/model_read_rule.py, bit for bit; and the serial host parser of
isle_amd/host/model_read.h, through isle_amd/host/model_read_main, against the same restatement on hand-made files.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import model_read_rule as rule
from isle_amd import hot_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "model_read_main")


def bits(x):
    return None if x is None else int(np.float32(x).view(np.uint32))


def same(tok, fmt="sparse"):
    want, got = rule.parse_weight(tok, fmt), hot_path.parse_weight(tok, fmt)
    assert bits(got) == bits(want), (tok, fmt, got, want)
    return want


def test_every_writer_output_reads_back_by_the_rule():
    rng = np.random.default_rng(11)
    w = np.concatenate([rng.random(1000, np.float32) ** 6, (rng.random(1000) * 10.0 ** rng.integers(-7, 7, 1000)).astype(np.float32)])
    seen = 0
    for x in w:
        for fmt in ("sparse", "dense"):
            tok = hot_path.entry_text(x, fmt)
            if tok:
                same(tok.encode(), fmt)
                seen += 1
    assert seen >= 3000


def test_long_digit_strings_where_fusing_or_an_fp32_combine_would_differ():
    rng = np.random.default_rng(12)

    def digits(n):
        return "".join(map(str, rng.integers(0, 10, n)))

    for i in range(2000):
        n = int(rng.integers(8, 15))
        tok = digits(n) + "." + digits(int(rng.integers(0, 4))) if i % 2 else digits(int(rng.integers(1, 3))) + "." + digits(n)
        assert same(tok.encode()) is not None


def test_edges_of_the_grammar():
    assert bits(same(b".5")) == bits(np.float32(0.5)) and bits(same(b"5.")) == bits(np.float32(5))
    assert bits(same(b"0.0")) == 0 and same(b"000.1") == np.float32(0.1)
    for tok in (b"0.1234", b"0.12345", b"0.1234567", b"3.0007", b"12.00009", b"7.0000001", b"1." + b"3" * 16, b"9" * 64, b"1." + b"0" * 62):
        assert same(tok) is not None     # 4, 5, 7 and 16 places: where repeated multiplication leaves pow
    for tok in (b"1.2.3", b"-1", b"1e-3", b"", b"1" * 65, b"nan", b".", b"1 ", b"1\r", b"+1", b"0x1"):
        assert same(tok) is None, tok
    assert bits(same(b"nan", "dense")) == 0x7fc00000
    for tok in (b"nan ", b"NaN", b"na", b"nann", b"inf"):
        assert same(tok, "dense") is None


def run_host(tmp_path, text, vocab, ncols, fmt, base=1):
    src, out = str(tmp_path / "model.txt"), str(tmp_path / "model.f32")
    open(src, "wb").write(text)
    r = subprocess.run([EXE, src, str(vocab), str(ncols), fmt, str(base), out], capture_output=True, text=True, timeout=120)
    if r.returncode:
        assert r.returncode == 3, r.stderr
        return r.stderr.strip()
    return np.fromfile(out, np.float32).reshape((vocab, ncols), order="F")


SPARSE = (b"  1 \t 2   0.123456789012\r\n\n3 1 12345678.5\n \t \n2 2 .5\n1 2 7.\n" b"3\t4\t00012345678901234.000001\n   2 3 0.000001")


def test_host_parser_follows_the_rule_on_hand_made_files(tmp_path):
    for base in (0, 1):
        want, n = rule.parse_sparse(SPARSE, 5, 4, base)
        assert n == 6
        got = run_host(tmp_path, SPARSE, 5, 4, "sparse", base)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want[1, 0] == np.float32(7)                                     # the last of two lines naming (topic 1, word 2)
    dense = b"0.5\t nan\t1.25 \t\r\n\n  3. .75 00.001\n"
    want, _ = rule.parse_dense(dense, 3, 2)
    got = run_host(tmp_path, dense, 3, 2, "dense")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and bits(got[1, 0]) == 0x7fc00000


@pytest.mark.parametrize("fmt,text", [
    ("sparse", b"1 1 0.5\n1 x 0.5\n"), ("sparse", b"1 1 0.5 7\n"), ("sparse", b"1 1 0.5\n1 1\n"), ("sparse", b"0 1 0.5\n"),
    ("sparse", b"1 9 0.5\n"), ("sparse", b"1 1 " + b"1" * 65 + b"\n"), ("sparse", b"1 1 nan\n"), ("sparse", b"1 1 .\n"),
    ("sparse", b"1" * 19 + b" 1 0.5\n"), ("sparse", b"1 1 1.2.3"),
    ("dense", b"1 2 3\n1 2\n"), ("dense", b"1 2 3\n"), ("dense", b"1 2 3\n1 2 3\n\n1 2 3\n"), ("dense", b"1 2 3\n1 2 3 4\n"),
    ("dense", b"1 2 x\n1 2 3\n"), ("dense", b""), ("sparse", b"1 1 0.5\n" + b" " * 4090 + b"1 1 0.5\n"), ("dense", b"1 2 3\n1 2" + b"\r" * 65 + b" 3\n"), ("dense", b"1 2 " + b"7" * 65 + b"\n1 2 3"),
])
def test_host_parser_refuses_what_the_rule_refuses_with_the_same_line_and_kind(tmp_path, fmt, text):
    with pytest.raises(rule.ModelReadError) as e:
        (rule.parse_sparse if fmt == "sparse" else rule.parse_dense)(text, 3, 2)
    msg = run_host(tmp_path, text, 3, 2, fmt)
    assert isinstance(msg, str) and msg.endswith(str(e.value)), (msg, str(e.value))
