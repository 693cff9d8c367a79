"""The C++ host side of the document prune as real processes, each run once under a time limit.  isle_amd/host/docs_prune_main.cpp is built
here against the library: `check` holds the device result (lengths, first_of, kept_docs, dropped, the new A) to the plain loop of
isle_amd/csrc/docs_host.h on a generated corpus with copies in it, accepted and refused; `train` runs a small ISLETrainer with
prune_documents (isle_amd/host/trainer_hip.h), whose DocsKept.tsv must equal the rule's bytes and whose training and cluster summary
must complete with the new number of documents."""
import glob
import os
import subprocess

import numpy as np
import pytest

import docs_rule as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("docs_prune_main") / "docs_prune_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", out, os.path.join(HOST, "docs_prune_main.cpp"), "-L" + os.path.join(ROOT, "isle_amd"),
                        "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


@pytest.mark.parametrize("args,says", [((20000, 6000, 1, 5, 40, 0, 0, 1), "equal the plain loop bit for bit"),
                                       ((3000, 9000, 2, 1, 0, 10, 100000, 0), "equal the plain loop bit for bit"),
                                       ((500, 300, 3, 9, 8, 0, 0, 1), "refused alike: prune_docs: min_words = 9 > max_words = 8"),
                                       ((500, 300, 4, 400, 0, 0, 0, 1), "refused alike: prune_docs: no document kept")])
def test_the_device_result_is_the_plain_loops(exe, args, says):
    r = subprocess.run([exe, "check"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and says in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_trainer_prunes_and_trains_on_the_kept_documents(exe, tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    counts, rows, offs = np.asarray(counts, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    words, tokens = dr.lengths(offs, counts)
    min_words, max_tokens = int(np.percentile(words, 10)), int(np.percentile(tokens, 90))
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "train", tdf, vocab, str(out), str(V), str(D), str(k), str(min_words), "0", "0", str(max_tokens), "1"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    want = dr.rule(dr.Case("trainer", V, offs, rows, counts, min_words, 0, 0, max_tokens, 1, ""))
    assert 0 < want["docs"] < D and want["dropped"][0] > 0 and want["dropped"][1] > 0
    text = "".join("%d\t%d\t%d\t%d\n" % (n + 1, o + 1, want["words"][o], want["tokens"][o]) for n, o in enumerate(want["kept_docs"].tolist()))
    assert open(os.path.join(log_dir, "DocsKept.tsv"), "rb").read() == text.encode()
    line = "Documents pruned: kept %d of %d, too short %d, too long %d, duplicates %d, entries kept %d dropped %d" % (
        want["docs"], D, want["dropped"][0], want["dropped"][1], want["dropped"][2], want["nnz"], rows.size - want["nnz"])
    assert line in r.stdout and "log directory: " in r.stdout     # train() and output_cluster_summary() completed behind the prune
