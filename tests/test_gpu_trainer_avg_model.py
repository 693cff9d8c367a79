"""ISLETrainer::output_avg_topic_coherence and output_topic_diversity (isle_amd/host/trainer_hip.h) end to end: the trainer mirror
loads a tdf file, trains, writes its summary and model files, then runs the two methods.  TopWordsPerTopic_avg.txt must hold the
words of top_words(average model, 10), the coherence line the brute-force UMass value of their first five, M_hat_avg the model in the
reference's dense text form, the diversity line the fp64 value of the catch model, and every output that existed before the two
calls must keep its bytes."""
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

from test_avg_model_cpu import dense_text
from test_cli_cpu import write_tdf
from test_gpu_coherence import brute
from isle_amd.hot_path import top_words
from tools.synth import Corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "trainer_avg_coherence_main")


def test_trainer_avg_coherence_and_diversity(tmp_path):
    V, D, k = 1500, 4000, 20
    c = Corpus(V, D, k, seed=6)
    counts, rows, offs = c.A()
    tdf = str(tmp_path / "corpus.tdf")
    write_tdf(tdf, counts, rows, offs)
    vocab = str(tmp_path / "vocab.txt")
    words = ["w%d" % i for i in range(V)]
    open(vocab, "w").write("\n".join(words))
    out = tmp_path / "out"
    out.mkdir()
    base = str(tmp_path / "dump")
    r = subprocess.run([EXE, tdf, vocab, str(out), str(V), str(D), str(k), "1", base], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    avg = np.fromfile(base + ".avg.f32", np.float32).reshape(V, k, order="F")
    catch = np.fromfile(base + ".catch.f32", np.float32).reshape(V, k, order="F")

    tw = np.array([[int(x) for x in line.split()[1:]] for line in open(base)], np.int64)
    np.testing.assert_array_equal(tw, top_words(avg, 10))
    lines = open(os.path.join(log_dir, "TopWordsPerTopic_avg.txt")).read().split("\n")
    assert lines[:k] == ["".join(words[w] + "\t" for w in tw[t]) for t in range(k)] and lines[k:] == [""]

    coh, _, _ = brute(V, rows, offs, tw[:, :5])
    fin = np.isfinite(coh)
    s = 0.0
    for v in coh[fin]:
        s += float(v)
    diag = open(os.path.join(log_dir, "diagnosticLog.txt")).read()
    coh_line = "\nAvg coherence without catchwords: %f\n" % (s / fin.sum())
    assert coh_line in diag

    assert open(os.path.join(log_dir, "M_hat_avg")).read() == dense_text(avg)

    M = catch.astype(np.float64)
    ok = np.isfinite(M).all(axis=0)
    abar = M[:, ok].sum(axis=1) / ok.sum()
    dist = ((M[:, ok] - abar[:, None]) ** 2).sum(axis=0)
    div_line = "\n Average topic diversity: %f\n\n" % float(np.float32(dist.mean()))
    assert div_line in diag

    for name in ("M_hat_catch_sparse", "TopWordsPerTopic_catch.txt"):
        assert open(os.path.join(log_dir, name), "rb").read() == open(base + ".before." + name, "rb").read(), name
    before = open(base + ".before.diagnosticLog.txt").read()
    assert diag.startswith(before)
    extra = diag[len(before):]
    if not fin.all():
        extra = extra.replace("\n Topics without a coherence (a top word occurs in no document): %d(%d)\n" % ((~fin).sum(), k), "", 1)
    assert extra == coh_line + div_line
    assert re.search(r"raw_coh:\s*0\s", diag)
    assert not math.isnan(s)
