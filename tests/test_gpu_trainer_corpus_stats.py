"""ISLETrainer's compute_log_combinatorial / compute_distinct_top_five_sets flags (isle_amd/host/trainer_hip.h) end to end, in both ingest
modes, through isle_amd/host/trainer_diagnostics_main: LogCombinatorial.txt, the "Distinct top five sets:" line of diagnosticLog.txt and
the two timer lines must be what the reference's print_log_combinatorial / print_distinct_top_five_sets (src/trainer.cpp:373-403) write
for the checker's values.  With the flags off none of it appears."""
import glob
import os
import subprocess

import numpy as np
import pytest

from test_cli_cpu import write_tdf
from test_gpu_corpus_stats import log_comb_checker, top5_checker
from tools.synth import Corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "trainer_diagnostics_main")
V, D, K = 1500, 4000, 20


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    cnt, rows, offs = Corpus(V, D, K, seed=6).A()
    d = tmp_path_factory.mktemp("corpus")
    tdf = str(d / "corpus.tdf")
    write_tdf(tdf, cnt, rows, offs)
    vocab = str(d / "vocab.txt")
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    return tdf, vocab, cnt, offs


def run(tmp_path, corpus, flags, mode):
    tdf, vocab = corpus[:2]
    out = tmp_path / ("out_%s_%d" % (mode, flags))
    out.mkdir()
    r = subprocess.run([EXE, tdf, vocab, str(out), str(V), str(D), str(K), str(flags), str(flags), mode], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    logdir = glob.glob(str(out / "*" / "diagnosticLog.txt"))[0].rsplit("/", 1)[0]
    return logdir, r.stdout


@pytest.mark.parametrize("mode", ["file", "iterative"])
def test_trainer_writes_both_diagnostics(tmp_path, corpus, mode):
    _, _, cnt, offs = corpus
    logdir, stdout = run(tmp_path, corpus, 1, mode)
    lines = open(os.path.join(logdir, "LogCombinatorial.txt")).read().split("\n")
    assert lines[-1] == ""
    assert lines[:-1] == ["%g" % v for v in log_comb_checker(cnt, offs)]     # std::ostream << float, precision 6, document order
    T, counts = top5_checker(cnt, offs)
    line = "Distinct top five sets: " + "".join("%d " % counts[m] for m in (2, 5, 10, 20, 50, 100, 200, 500)) + "\n"
    diag = open(os.path.join(logdir, "diagnosticLog.txt")).read()
    assert line in diag
    assert line in stdout
    assert stdout.count("top five vec size: %d\n" % len(T)) == 8
    timer = open(os.path.join(logdir, "timerLog.txt")).read()
    assert "Time for Print Log Combinatorial" in timer and "Time for Distinct top-5 words" in timer
    # the reference's place: after the data is in, before the thresholding lines of train()
    assert timer.index("Populating CSC") < timer.index("Print Log Combinatorial") < timer.index("Distinct top-5 words") < timer.index(
        "Computing thresholds")


def test_flags_off_write_nothing(tmp_path, corpus):
    logdir, stdout = run(tmp_path, corpus, 0, "file")
    assert not os.path.exists(os.path.join(logdir, "LogCombinatorial.txt"))
    diag = open(os.path.join(logdir, "diagnosticLog.txt")).read()
    assert "Distinct top five sets" not in diag and "top five vec size" not in stdout
    timer = open(os.path.join(logdir, "timerLog.txt")).read()
    assert "Print Log Combinatorial" not in timer and "Distinct top-5 words" not in timer
