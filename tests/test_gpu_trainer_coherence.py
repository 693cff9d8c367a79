"""ISLETrainer's compute_avg_coherence (isle_amd/host/trainer_hip.h) end to end: the trainer mirror loads a tdf file, trains and writes
its cluster summary; the coherence lines of diagnosticLog.txt must be the brute-force values of the top words it chose.  With the
flag off the summary keeps its zeros."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli_cpu import write_tdf
from test_gpu_coherence import brute
from tools.synth import Corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "trainer_coherence_main")


def run(tmp_path, flag):
    V, D, k = 1500, 4000, 20
    c = Corpus(V, D, k, seed=6)
    counts, rows, offs = c.A()
    tdf = str(tmp_path / "corpus.tdf")
    write_tdf(tdf, counts, rows, offs)
    vocab = str(tmp_path / "vocab.txt")
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / ("out%d" % flag)
    out.mkdir()
    tw_file = str(tmp_path / ("topwords%d.txt" % flag))
    r = subprocess.run([EXE, tdf, vocab, str(out), str(V), str(D), str(k), str(flag), tw_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    diag = open(glob.glob(str(out / "*" / "diagnosticLog.txt"))[0]).read()
    tw = np.array([[int(x) for x in line.split()[1:]] for line in open(tw_file)], np.int64)
    return V, rows, offs, k, diag, tw


def cluster_rows(diag):
    return {int(m.group(1)): m.group(2) for m in re.finditer(r"^Cluster\s*(\d+)\s.*flt_coh:\s*(\S+)\s+#catchwords", diag, flags=re.M)}


def test_trainer_prints_the_coherence_of_its_top_words(tmp_path):
    V, rows, offs, k, diag, tw = run(tmp_path, 1)
    assert tw.shape == (k, 10)
    coh, _, _ = brute(V, rows, offs, tw[:, :5])                  # DEFAULT_COHERENCE_NUM_WORDS = 5
    assert np.isfinite(coh).all()
    lines = re.findall(r"^Coherence: (\S+)$", diag, flags=re.M)
    assert lines == ["%f" % v for v in coh]                      # std::to_string(double), topic order
    avg = 0.0
    for v in coh:                                                # the trainer's order: topics ascending, in double
        avg += float(v)
    avg /= k
    assert "\n Avg coherence: %f\n" % avg in diag
    flt = cluster_rows(diag)
    assert sorted(flt) == list(range(k))
    for t in range(k):
        assert flt[t] == "%g" % coh[t], t                          # each row carries its own topic's value
    assert "Topics without a coherence" not in diag
    assert re.search(r"raw_coh:\s*0\s", diag)


def test_flag_off_keeps_the_zero_summary(tmp_path):
    _, _, _, k, diag, _ = run(tmp_path, 0)
    assert "\n Avg coherence: 0.000000\n" in diag
    assert "\nCoherence: " not in diag
    flt = cluster_rows(diag)
    assert sorted(flt) == list(range(k)) and set(flt.values()) == {"0"}
