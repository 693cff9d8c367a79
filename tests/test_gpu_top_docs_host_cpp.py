"""ISLETrainer::output_topic_top_docs (isle_amd/host/trainer_hip.h) end to end through isle_amd/host/trainer_top_docs_main.cpp as a real
process: built here against the library, run once under a time limit on a small corpus; TopDocsPerTopic.tsv, selected on the device, equals
byte for byte the lines the host statement of the rule (topdocs_select_host) gives on the fetched catchword sums."""
import glob
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def test_trainer_writes_the_top_documents_of_every_topic(tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k, n = 1500, 4000, 20, 10
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    exe = str(tmp_path / "trainer_top_docs_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", exe, os.path.join(HOST, "trainer_top_docs_main.cpp"), "-L" + os.path.join(ROOT, "isle_amd"),
                        "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    out = tmp_path / "out"
    out.mkdir()
    want_path = str(tmp_path / "want.tsv")
    r = subprocess.run([exe, tdf, vocab, str(out), str(V), str(D), str(k), str(n), want_path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    got = open(os.path.join(log_dir, "TopDocsPerTopic.tsv"), "rb").read()
    assert got == open(want_path, "rb").read() and got.endswith(b"\n")
    lines = [l.split(b"\t") for l in got.split(b"\n")[:-1]]
    topics = [int(x[1]) for x in lines]
    assert topics == sorted(topics) and 1 <= topics[0] and topics[-1] <= k and all(topics.count(t) <= n for t in set(topics)) and len(lines) > k
    assert all(1 <= int(x[0]) <= D for x in lines)
    for t in set(topics):  # within a topic: the heavier value first (as printed: six digits), so the printed weights do not ascend
        w = [float(x[2]) for x in lines if int(x[1]) == t]
        assert all(a >= b_ for a, b_ in zip(w, w[1:]))
