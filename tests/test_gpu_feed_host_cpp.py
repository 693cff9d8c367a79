"""isle_amd/host/feed_main run as a real process on the GPU: the base corpus of tests/feed_rule.py as a tdf file (repeated pairs and zero
counts included: the driver reads the file itself), shuffled by the driver, built into A by trainer_detail::csc_from_fed on the host and by
the device feed in batches of <flush_entries>; the driver exits 0 only if the two matrices agree in every bit."""
import os
import subprocess

import numpy as np
import pytest

from feed_rule import BASE_D, BASE_V, base_corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "feed_main")


@pytest.fixture(scope="module")
def tdf(tmp_path_factory):
    d, w, c = base_corpus()
    path = str(tmp_path_factory.mktemp("feed") / "base.tdf")
    np.savetxt(path, np.stack([d.astype(np.int64) + 1, w.astype(np.int64) + 1, c.astype(np.int64)], axis=1), fmt="%d")
    return path, len(d), int(np.count_nonzero(c))


@pytest.mark.parametrize("flush", [1, 7, 4096])
def test_the_device_feed_equals_csc_from_fed(tdf, flush):
    path, n, nonzero = tdf
    assert os.path.exists(EXE), "build with make -C isle_amd/csrc"
    r = subprocess.run([EXE, path, str(BASE_V), str(BASE_D), str(flush)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "identical: %d entries fed, %d kept, nnz 5600" % (n, nonzero)
