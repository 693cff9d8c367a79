"""The C++ host side of the model comparison as real processes, each run once under a time limit.  isle_amd/host/model_compare_main.cpp is
built here against the library: `check` holds FPSparseMatrixHip::compare_models / match_topics to isle_amd/csrc/match_host.h
(model_dist_plain, match_greedy) on a handful of the cases of tests/match_rule.py, read from a file this test writes; `train` runs a small
ISLETrainer and output_model_comparison (isle_amd/host/trainer_hip.h) on the model file the run itself wrote: TopicMatch.tsv must equal
trainer_detail::topic_match_text byte for byte, and the log line must be there."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import match_rule as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("model_compare_main") / "model_compare_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", out, os.path.join(HOST, "model_compare_main.cpp"), "-L" + os.path.join(ROOT, "isle_amd"),
                        "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def lst(a):
    a = np.asarray(a).reshape(-1)
    return [a.size] + [int(x) for x in a]


def test_the_device_is_match_host_h_on_a_handful_of_cases(exe, tmp_path):
    dist = [c for c in mr.DIST_CASES if c.name in ("nonfinite", "same", "ties")] + mr.DIST_CASES[:36:5]
    match = [c for c in mr.MATCH_CASES if c.name in ("zeros", "nan_row", "nan_col", "all_nan", "infs", "one", "i_plus_j", "near_diagonal", "ints1_17x9")]
    assert len(dist) == 11 and len(match) == 9
    lines = []
    for c in dist:
        lines.append(["dist", c.a.shape[0], c.a.shape[1], c.b.shape[1]] + lst(c.a.reshape(-1, order="F").view(np.uint32)) + lst(c.b.reshape(-1, order="F").view(np.uint32)))
    for c in match:
        lines.append(["match", c.dist.shape[0], c.dist.shape[1]] + lst(np.ascontiguousarray(c.dist).view(np.uint64)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(t) for t in line) for line in lines) + "\n")
    r = subprocess.run([exe, "check", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "11 distance cases and 9 matching cases equal match_host.h bit for bit" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_trainer_compares_its_model_with_the_file_it_wrote(exe, tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 8
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, np.asarray(counts, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64))
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "train", tdf, vocab, str(out), str(V), str(D), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert "bytes equal topic_match_text" in r.stdout and "log directory: " in r.stdout
    log_dir = glob.glob(str(out / "*"))[0]
    text = open(os.path.join(log_dir, "TopicMatch.tsv")).read()
    rows_ = [line.split("\t") for line in text.splitlines()]
    assert [int(x[0]) for x in rows_] == list(range(1, k + 1)) and all(len(x) == 3 for x in rows_)
    m = re.search(r"Avg L1 distance of matched topics: (\S+) \((\d+) of %d matched\)" % k, r.stdout)
    assert m, r.stdout[-1000:]
    matched = [x for x in rows_ if x[1] != "-1"]
    assert int(m.group(2)) == len(matched) and all(x[2] == "nan" for x in rows_ if x[1] == "-1")
    assert all(int(x[1]) == int(x[0]) for x in matched)                # the file is this run's model: every topic finds itself
    s = 0.0
    for x in matched:                                                  # the mean: ascending topic, in double, as %.17g prints it
        s += float(x[2])
    assert matched and float(m.group(1)) == s / len(matched)
