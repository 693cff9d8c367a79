"""tdf_pump::file_range (isle_amd/host/tdf_pump.h), the lines of one byte range of a file, without the library and without a GPU:
tdf_range_main is built here with the address and undefined-behaviour sanitizers (a stand-alone program) and pumps ranges of a file
through a two-buffer sink in host memory, once with read() as it is and once with short reads and EINTR.  What the sink must have been
given is tests/tdf_shard_rule.owned, the plain rule: the lines whose first byte lies in the range."""
import os
import subprocess

import pytest

import tdf_shard_rule as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")
TEXT40 = b"1 2 3\r\n\r\n\n 2 1 7 \r\n12 10 345\n\n3 3 9\r\n4 4"      # '\r\n', blank lines, no final newline
assert len(TEXT40) == 40


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tdf_range") / "tdf_range_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(HOST, "tdf_range_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def pump(exe, path, piece, *rng):
    r = subprocess.run([exe, path, str(piece)] + [str(x) for x in rng], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr and "DIFFERENT" not in r.stdout, r.stdout[-2000:] + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        b, e, hx = line.split()
        out[(int(b), int(e))] = b"" if hx == "-" else bytes.fromhex(hx)
    return out


def write(tmp_path, name, text):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(text)
    return path


@pytest.mark.parametrize("piece", (1, 3, 64))
def test_every_range_of_a_40_byte_text(exe, tmp_path, piece):
    """every 0 <= b, e <= 41: empty ranges, ranges inside one line, b on, just before and just behind every '\\n', e equal to and past the
    file's size"""
    got = pump(exe, write(tmp_path, "t40", TEXT40), piece)
    assert len(got) == 42 * 42
    for (b, e), text in got.items():
        assert text == tr.owned(TEXT40, b, e), (b, e, text)
    assert got[(0, 40)] == got[(0, 41)] == TEXT40 and got[(7, 7)] == got[(9, 3)] == b""


def test_the_ranges_of_the_ranks_side_by_side_are_the_file(exe, tmp_path):
    got = pump(exe, write(tmp_path, "t40", TEXT40), 5)
    for n in range(1, 42):
        assert b"".join(got[tr.rank_range(40, r, n)] for r in range(n)) == TEXT40, n


def test_named_edges(exe, tmp_path):
    text = b"1 1 1\n" + b"0" * 9000 + b"2 2 2\n3 3 3\n"               # a line of 9006 bytes: longer than the pump's own 4096-byte skip buffer
    path = write(tmp_path, "long", text)
    size, nl = len(text), 5
    for b, e in ((nl, size), (nl - 1, size), (nl + 1, size),          # b on, just before and just behind a '\n'
                 (100, 8000),                                         # a range inside one long line owns nothing
                 (3, 3), (size, size), (0, 0),                        # empty ranges
                 (0, size), (7, size), (size - 3, size),              # e equal to the file size
                 (0, nl), (0, nl + 1), (0, nl + 2), (6, 7), (9011, 9013), (size - 1, size + 5)):
        for piece in (1, 4096, 100000):
            got = pump(exe, path, piece, b, e)
            assert got[(b, e)] == tr.owned(text, b, e), (b, e, piece)
    assert tr.owned(text, 100, 8000) == b"" and tr.owned(text, nl + 1, size) == text[6:] and tr.owned(text, nl, size) == text[6:]


def test_a_missing_file_is_an_error(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path / "none"), "4096", "0", "10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot open" in r.stderr
