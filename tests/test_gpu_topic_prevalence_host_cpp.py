"""FPSparseMatrixHip::topic_prevalence and ISLETrainer::output_topic_prevalence (isle_amd/host/fpsparse_hip.h, trainer_hip.h) end to end
through isle_amd/host/topic_prevalence_main.cpp as a real process: built here against the library, run once under a time limit on a small
corpus.  The program holds the device's arrays, with and without labels and normalise, to the host statement of the rule (prevalence_host,
isle_amd/csrc/prevalence_host.h) on the fetched catchword sums, == on the integers and on the bits of the doubles, and TopicPrevalence.tsv,
parsed again, to the arrays, and prints one line per check; this test asserts those lines and reads the file once more itself."""
import glob
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def test_trainer_writes_the_topic_prevalence_of_its_groups(tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k, G = 1500, 4000, 20, 7
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    exe = str(tmp_path / "topic_prevalence_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", exe, os.path.join(HOST, "topic_prevalence_main.cpp"),
                        "-L" + os.path.join(ROOT, "isle_amd"), "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, tdf, vocab, str(out), str(V), str(D), str(k), str(G)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    checks = [l for l in r.stdout.splitlines() if l.startswith(("ok ", "FAILED "))]
    assert len(checks) == 6 and all(l.startswith("ok ") for l in checks), checks
    assert "before train() is refused" in checks[0] and "TopicPrevalence.tsv parsed again is the arrays" in checks[5]
    for line, name in zip(checks[1:5], ("(no labels)", "(no labels, normalise)", "(labels)", "(labels, normalise)")):
        assert "topic_prevalence %s is the host statement bit for bit" % name in line
    none = sum(1 for d in range(D) if d % 17 == 16)
    assert "1 groups" in checks[1] and " 0 rows in no group" in checks[1] and "%d groups" % G in checks[3] and " %d rows in no group" % none in checks[3]
    log_dir = glob.glob(str(out / "*"))[0]
    got = open(os.path.join(log_dir, "TopicPrevalence.tsv"), "rb").read()
    lines = [l.split(b"\t") for l in got.split(b"\n")[:-1]]
    assert got.endswith(b"\n") and "%d lines" % len(lines) in checks[5] and 0 < len(lines) <= G * k and all(len(x) == 7 for x in lines)
    cells = [(int(x[0]), int(x[1])) for x in lines]
    assert cells == sorted(set(cells)) and all(0 <= g < G and 1 <= t <= k for g, t in cells)  # group ascending, then topic ascending, 1-based
    docs = {g: sum(1 for d in range(D) if d % 17 != 16 and d % G == g) for g in range(G)}
    for x in lines:
        g, n, with_topic, dominant, total, mean = int(x[0]), int(x[2]), int(x[3]), int(x[4]), float(x[5]), float(x[6])
        assert n == docs[g] and 0 < with_topic <= n and dominant <= with_topic and total >= 0
        assert np.float64(mean) == np.float64(total) / np.float64(n) and x[5] == b"%.17g" % total  # the doubles as %.17g: they read back exactly
    by_group = {}
    for x in lines:
        by_group[int(x[0])] = by_group.get(int(x[0]), 0) + int(x[4])
    assert all(by_group[g] <= docs[g] for g in by_group) and sum(by_group.values()) > 0  # a document has one dominant topic at most
