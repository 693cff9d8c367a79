"""FPSparseMatrixHip::similar_documents and ISLETrainer::output_similar_docs (isle_amd/host/fpsparse_hip.h, trainer_hip.h) end to end through
isle_amd/host/similar_docs_main.cpp as a real process: built here against the library, run once under a time limit on a small corpus.  The
program holds the device's lists under every measure to the host statement of the rule (simdocs_select_host) on the fetched catchword sums,
bit for bit, and SimilarDocs.tsv to the lists, byte for byte, and prints one line per check; this test asserts those lines and the file."""
import glob
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def test_trainer_writes_the_similar_documents_of_its_queries(tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k, n = 1500, 4000, 20, 10
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    exe = str(tmp_path / "similar_docs_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", exe, os.path.join(HOST, "similar_docs_main.cpp"), "-L" + os.path.join(ROOT, "isle_amd"),
                        "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, tdf, vocab, str(out), str(V), str(D), str(k), str(n)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    checks = [l for l in r.stdout.splitlines() if l.startswith(("ok ", "FAILED "))]
    assert len(checks) == 5 and all(l.startswith("ok ") for l in checks), checks
    assert "before train() is refused" in checks[0] and "SimilarDocs.tsv is the lists byte for byte" in checks[4]
    for line, name in zip(checks[1:4], ("dot", "cosine", "bhattacharyya")):
        assert "(%s) is the host statement bit for bit: 5 queries" % name in line
    log_dir = glob.glob(str(out / "*"))[0]
    got = open(os.path.join(log_dir, "SimilarDocs.tsv"), "rb").read()
    lines = [l.split(b"\t") for l in got.split(b"\n")[:-1]]
    assert got.endswith(b"\n") and "%d lines" % len(lines) in checks[4] and 0 < len(lines) <= 5 * n
    queries = [1, D // 3 + 1, D // 2 + 1, D // 3 + 1, D]
    seen = [int(x[0]) for x in lines]
    assert [q for i, q in enumerate(seen) if i == 0 or seen[i - 1] != q] == [q for q in queries if q in seen]  # the queries in the order given
    assert all(1 <= int(x[1]) <= D and int(x[1]) != int(x[0]) for x in lines)                                    # a document is not its own neighbour
    runs = []  # a query's neighbours lie together (the query given twice has two runs): the higher score first, as printed (six digits)
    for i, x in enumerate(lines):
        if i == 0 or seen[i - 1] != seen[i]:
            runs.append([])
        runs[-1].append(float(x[2]))
    assert all(len(r) <= n and all(a >= b_ for a, b_ in zip(r, r[1:])) for r in runs)
