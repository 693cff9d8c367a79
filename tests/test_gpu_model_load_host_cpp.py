"""FPSparseMatrixHip::load_model_file (isle_amd/host/fpsparse_hip.h) run as a real process on the GPU, through isle_amd/host/model_load_main:
a model goes through FPSparseMatrixHip::write_model_text into a file of either format and comes back through the device loader and
through the C++ host parser of isle_amd/host/model_read.h; the two models must agree bit for bit, and with the Python rule."""
import os
import subprocess

import numpy as np
import pytest

import model_read_rule as rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "model_load_main")


def test_load_model_file_equals_the_host_parser(tmp_path):
    V, k = 700, 9
    rng = np.random.default_rng(21)
    M = (rng.random((V, k)) * 10.0 ** rng.integers(-7, 4, (V, k))).astype(np.float32)
    M[rng.random((V, k)) < 0.5] = 0
    src, base = str(tmp_path / "model.f32"), str(tmp_path / "m")
    np.asfortranarray(M).ravel(order="F").tofile(src)
    assert os.path.exists(EXE), "build with make -C isle_amd/csrc"
    r = subprocess.run([EXE, src, str(V), str(k), base], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    entries = dict(ln.split() for ln in r.stdout.splitlines())
    for fmt in ("sparse", "dense"):
        text = open("%s.%s" % (base, fmt), "rb").read()
        dev = np.fromfile("%s.%s.dev.f32" % (base, fmt), np.uint32)
        host = np.fromfile("%s.%s.host.f32" % (base, fmt), np.uint32)
        want, n = (rule.parse_sparse if fmt == "sparse" else rule.parse_dense)(text, V, k)
        assert dev.size == V * k and np.array_equal(dev, host)
        assert np.array_equal(dev, want.ravel(order="F").view(np.uint32)) and int(entries[fmt]) == n
