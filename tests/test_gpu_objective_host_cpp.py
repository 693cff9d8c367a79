"""FPSparseMatrixHip::set_compute_residual and kmeans_objective (isle_amd/host/fpsparse_hip.h) through hot_path_main as a real process:
with the flag the two Lloyd loops print the reference's residual lines, non-zero, whose squares are the objective of the state each loop
ended in; without it stdout is what it was: the same text with every residual printed as 0 and no line added."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "hot_path_main")
LINE = re.compile(r"^Lloyd's iter (\d+)  dist_sq residual: (\S+)$")


def test_residual_lines_and_the_unchanged_default(tmp_path):
    B = corpus(2000, 5000, 20, 0)
    k = 20
    fin = str(tmp_path / "B.bin")
    with open(fin, "wb") as f:
        np.array([B["V"], B["D"], B["nnz"]], np.uint64).tofile(f)
        B["vals"].astype(np.float32).tofile(f)
        B["rows"].astype(np.uint64).tofile(f)
        B["offs"].astype(np.int64).tofile(f)
    plain = subprocess.run([EXE, fin, str(k), str(tmp_path / "a.bin")], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr[-2000:]
    flag = subprocess.run([EXE, fin, str(k), str(tmp_path / "b.bin"), "residual"], capture_output=True, text=True, timeout=120)
    assert flag.returncode == 0, flag.stderr[-2000:]
    assert open(tmp_path / "a.bin", "rb").read() == open(tmp_path / "b.bin", "rb").read()  # the flag changes no result

    # the default: every residual line of Lloyd on B says 0, as it always did, and the loop in span(U) prints none
    lines = plain.stdout.split("\n")
    res = [LINE.match(l) for l in lines if l.startswith("Lloyd's iter")]
    assert res and all(m and m.group(2) == "0" for m in res) and [int(m.group(1)) for m in res] == list(range(len(res)))
    assert "k-means objective" not in plain.stdout

    # with the flag: two runs of residual lines (span(U), then B), each numbered from 0, all non-zero ...
    flines = flag.stdout.split("\n")
    runs, totals = [], {}
    for l in flines:
        m = LINE.match(l)
        if m:
            if int(m.group(1)) == 0:
                runs.append([])
            runs[-1].append(float(m.group(2)))
        elif l.startswith("k-means objective ("):
            space, rest = l[len("k-means objective ("):].split("): ")
            totals[space] = [float(x) for x in rest.split()]
    assert len(runs) == 2 and all(v > 0 for r in runs for v in r) and len(runs[1]) == len(res)
    # ... the last of each squared is the objective of the state the loop ended in (ostream prints six digits; the returned residual is
    # the objective rounded to float), and the total is the clusters' sums added in ascending order
    for space, run in (("projected", runs[0]), ("word", runs[1])):
        ret, total, summed = totals[space]
        assert total == summed and total > 0
        assert abs(ret - total) <= 2.0 ** -23 * total
        assert abs(run[-1] ** 2 - total) <= 1e-5 * total
    # ... and nothing else differs: the flag's text with its residuals put back to 0 and its added lines taken out is the default's
    back, n_run = [], 0
    for l in flines:
        m = LINE.match(l)
        if m:
            n_run += int(m.group(1)) == 0
            if n_run == 2:
                back.append("Lloyd's iter %s  dist_sq residual: 0" % m.group(1))
        elif not l.startswith("k-means objective ("):
            back.append(l)
    assert "\n".join(back) == plain.stdout


def test_trainer_writes_the_cluster_objective_and_only_adds_to_the_log(tmp_path):
    """ISLETrainer::output_kmeans_objective after train(): ClusterObjective.tsv holds "<topic>\\t<size>\\t<distsq_sum>" for every topic,
    1-based, the sizes of the partition, and the log gains the total, which is the file's sums added in order (both printed as %.9g)"""
    import glob
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    base = str(tmp_path / "dump")
    exe = os.path.join(ROOT, "isle_amd", "host", "trainer_objective_main")
    r = subprocess.run([exe, tdf, vocab, str(out), str(V), str(D), str(k), base], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    sizes = [int(l.split()[1]) for l in open(base)]
    text = open(os.path.join(log_dir, "ClusterObjective.tsv")).read()
    rows_ = [l.split("\t") for l in text.split("\n")[:-1]]
    assert text.endswith("\n") and [int(x[0]) for x in rows_] == list(range(1, k + 1)) and [int(x[1]) for x in rows_] == sizes
    sums = [float(x[2]) for x in rows_]
    assert all(x[2] == "%.9g" % float(x[2]) for x in rows_) and all(s > 0 for s, n in zip(sums, sizes) if n > 1) and all(s == 0 for s, n in zip(sums, sizes) if n == 0)
    diag = open(os.path.join(log_dir, "diagnosticLog.txt")).read()
    before = open(base + ".before.diagnosticLog.txt").read()
    assert diag.startswith(before)
    m = re.search(r"k-means objective on B: (\S+)\n", diag[len(before):])
    assert m and abs(float(m.group(1)) - sum(sums)) <= 1e-7 * sum(sums)
