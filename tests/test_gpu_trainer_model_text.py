"""The trainer's model files come from the device text path (ISLETrainer::output_model, write_edgemodel_to_file and the M_hat_avg write of
output_avg_topic_coherence, isle_amd/host/trainer_hip.h): isle_amd/host/trainer_model_text_main runs the ISLETrain command's sequence with
edge topics on, then the average model, and dumps the floats behind the three files (get_basic_model, get_edge_model, the average
model).  M_hat_catch_sparse, EdgeModel_sparse and M_hat_avg must be, byte for byte, the numpy restatement of the host writers
(tests/test_model_text_cpu.py) applied to those floats.  The ISLETrain command itself then runs on the same corpus: its two model
files must have the same lines (topic, word) as the dump's and weights within the fp32 summation-order noise the CLI test allows."""
import glob
import os
import subprocess

import numpy as np
import pytest

from test_cli_cpu import write_tdf
from test_model_text_cpu import dense_text_np, sparse_text
from tools.synth import Corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def test_trainer_model_files_are_the_text_of_its_models(tmp_path):
    V, D, k, max_edge = 1500, 4000, 20, 30
    c = Corpus(V, D, k, seed=6)
    counts, rows, offs = c.A()
    tdf = str(tmp_path / "corpus.tdf")
    n = write_tdf(tdf, counts, rows, offs)
    vocab = str(tmp_path / "vocab.txt")
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    dump = str(tmp_path / "dump")
    r = subprocess.run([os.path.join(HOST, "trainer_model_text_main"), tdf, vocab, str(out), str(V), str(D), str(n), str(k), str(max_edge), dump],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    ne = int(open(dump + ".nedge").read())
    assert 0 < ne <= max_edge
    catch = np.fromfile(dump + ".catch.f32", np.float32).reshape(V, k, order="F")
    edge = np.fromfile(dump + ".edge.f32", np.float32).reshape(V, ne, order="F")
    avg = np.fromfile(dump + ".avg.f32", np.float32).reshape(V, k, order="F")
    files = {}
    for name, want in (("M_hat_catch_sparse", sparse_text(catch)), ("EdgeModel_sparse", sparse_text(edge)), ("M_hat_avg", dense_text_np(avg))):
        files[name] = open(os.path.join(log_dir, name), "rb").read()
        assert len(files[name]) > 0 and files[name] == want, name

    out2 = tmp_path / "cli"
    out2.mkdir()
    r = subprocess.run([os.path.join(HOST, "ISLETrain"), tdf, vocab, str(out2), str(V), str(D), str(n), str(k), "0", "0", "0", "1", str(max_edge)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ISLE Trainer failed" not in r.stderr, r.stderr[-2000:]
    cli_dir = glob.glob(str(out2 / "*"))[0]
    for name, cols in (("M_hat_catch_sparse", k), ("EdgeModel_sparse", ne)):
        A, B = np.zeros((V, cols)), np.zeros((V, cols))
        for M, text in ((A, open(os.path.join(cli_dir, name)).read()), (B, files[name].decode())):
            for ln in text.splitlines():
                t, w, x = ln.split("\t")
                assert len(x.split(".")[1]) == 6
                M[int(w) - 1, int(t) - 1] = float(x)
        assert np.abs(A - B).max() <= 2e-6, name
