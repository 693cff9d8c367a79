"""isle_amd/host/tdf_pump.h, the file loop of the tdf text stream, without the library and without a GPU: tdf_pump_main is built here with
the address and undefined-behaviour sanitizers (a stand-alone program) and pumps files of sizes around a piece through a two-buffer sink
in host memory, once with read() as it is and once with short reads and EINTR.  It exits 0 only if what the sink was given equals the file
and the sink saw one buffer out at a time and no commit above its capacity."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")
SMALL_SIZES = (0, 1, 4095, 4096, 4097)
MEGABYTE = 1000000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tdf_pump") / "tdf_pump_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(HOST, "tdf_pump_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tdf_pump_files")
    rng = np.random.default_rng(3)
    paths = {}
    for n in SMALL_SIZES + (MEGABYTE,):
        paths[n] = str(d / ("f%d" % n))
        with open(paths[n], "wb") as f:
            f.write(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
    return paths


@pytest.mark.parametrize("size,piece", [(n, p) for n in SMALL_SIZES for p in (1, 4096, 65536)] + [(MEGABYTE, 4096), (MEGABYTE, 65536)])
def test_the_pump_delivers_the_file(exe, files, size, piece):
    r = subprocess.run([exe, files[size], str(piece)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("%d bytes in" % size) == 2 and r.stdout.count("equal") == 2 and "DIFFERENT" not in r.stdout


def test_a_missing_file_is_an_error(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path / "none"), "4096"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot open" in r.stderr
