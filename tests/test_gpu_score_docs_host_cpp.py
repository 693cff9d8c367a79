"""FPSparseMatrixHip::score_documents and ISLETrainer::output_doc_scores (isle_amd/host/fpsparse_hip.h, trainer_hip.h) end to end through
isle_amd/host/score_docs_main.cpp as a real process: built here against the library, run once under a time limit on a small corpus.  The
program holds the device's arrays, on the resident count matrix and on a held-out third of every document, to the host statement of the rule
(score_docs_host, isle_amd/csrc/score_host.h) on the fetched matrix, model and weights: == on the bits for "prob", on tokens and counters for
"log" with two calls the same bits; and DocScores.tsv to trainer_detail::doc_scores_text byte for byte.  It prints one line per check; this
test asserts those lines, reads the file once more itself and finds the two lines of the log."""
import glob
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def test_trainer_writes_the_scores_of_its_documents(tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    exe = str(tmp_path / "score_docs_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", exe, os.path.join(HOST, "score_docs_main.cpp"),
                        "-L" + os.path.join(ROOT, "isle_amd"), "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, tdf, vocab, str(out), str(V), str(D), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    checks = [l for l in r.stdout.splitlines() if l.startswith(("ok ", "FAILED "))]
    assert len(checks) == 7 and all(l.startswith("ok ") for l in checks), checks
    assert "before train() is refused" in checks[0] and "before an inference is refused" in checks[1]
    for line, name in zip(checks[2:6], ("(prob) on the resident count matrix", "(log, normalise) on the resident count matrix",
                                        "(prob) on the held-out third", "(log, normalise) on the held-out third")):
        assert "score_documents " + name in line
    assert "%d entries" % counts.size in checks[2] and "DocScores.tsv is the host loop's text byte for byte" in checks[6] and "%d lines" % D in checks[6]
    held = int(checks[4].split(" entries")[0].split()[-1])
    assert 0.25 * counts.size < held < 0.42 * counts.size  # one entry in three
    log_dir = glob.glob(str(out / "*"))[0]
    got = open(os.path.join(log_dir, "DocScores.tsv"), "rb").read()
    lines = [l.split(b"\t") for l in got.split(b"\n")[:-1]]
    assert got.endswith(b"\n") and len(lines) == D and all(len(x) == 4 for x in lines)
    assert [int(x[0]) for x in lines] == list(range(1, D + 1))
    tokens = np.array([float(x[1]) for x in lines])
    score = np.array([float(x[2]) for x in lines])
    assert all(x[1] == b"%.17g" % t and x[2] == b"%.17g" % s for x, t, s in zip(lines, tokens, score))  # the doubles as %.17g: they read back exactly
    assert (tokens >= 0).all() and (tokens == np.floor(tokens)).all() and (score <= 0).all() and (score[tokens > 0] < 0).all()
    assert all(x[3].isdigit() for x in lines)
    text = "".join(open(p, errors="replace").read() for p in glob.glob(os.path.join(log_dir, "*")) if os.path.isfile(p)) + r.stdout + r.stderr
    llh = [l for l in text.splitlines() if "Held-out log-likelihood per token: " in l]
    ppl = [l for l in text.splitlines() if "Perplexity: " in l]
    assert llh and ppl
    per_token, perplexity = float(llh[0].split(": ")[1]), float(ppl[0].split(": ")[1])
    assert per_token < 0 and abs(perplexity - np.exp(-per_token)) <= 1e-12 * perplexity and 1.0 < perplexity < float("inf")
