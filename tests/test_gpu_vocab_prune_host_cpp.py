"""The C++ host side of the vocabulary prune as real processes, each run once under a time limit.  isle_amd/host/vocab_prune_main.cpp is
built here against the library: `check` holds the device result (df, kept_words, the new A) to the plain loop of isle_amd/csrc/vocab_host.h on
a generated corpus, accepted and refused; `train` runs a small ISLETrainer with prune_vocabulary (isle_amd/host/trainer_hip.h), whose
VocabKept.tsv must equal the rule's bytes and whose TopWordsPerTopic_catch.txt may name only kept words of the vocabulary file."""
import glob
import os
import subprocess

import numpy as np
import pytest

import vocab_rule as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vocab_prune_main") / "vocab_prune_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", out, os.path.join(HOST, "vocab_prune_main.cpp"), "-L" + os.path.join(ROOT, "isle_amd"),
                        "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


@pytest.mark.parametrize("args,says", [((20000, 6000, 1, 3, 1500, 4000), "equal the plain loop bit for bit"),
                                       ((40000, 3000, 2, 2, 0, 0), "equal the plain loop bit for bit"),
                                       ((500, 300, 3, 301, 0, 0), "refused alike: prune_vocab: min_df = 301 > max_df = 300"),
                                       ((500, 300, 4, 290, 295, 0), "refused alike: prune_vocab: no word kept")])
def test_the_device_result_is_the_plain_loops(exe, args, says):
    r = subprocess.run([exe, "check"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and says in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_trainer_prunes_and_names_the_kept_words(exe, tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    min_df, max_df, keep_n = 5, D // 2, 1000
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "train", tdf, vocab, str(out), str(V), str(D), str(k), str(min_df), str(max_df), str(keep_n)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    case = vr.Case("trainer", V, np.asarray(offs, np.int64), np.asarray(rows, np.uint32), np.asarray(counts, np.float32), min_df, max_df, keep_n, "", True)
    want = vr.rule(case)
    assert want["vocab"] == keep_n < V
    text = "".join("%d\t%d\t%d\n" % (n + 1, o + 1, want["df"][o]) for n, o in enumerate(want["kept_words"].tolist()))
    assert open(os.path.join(log_dir, "VocabKept.tsv"), "rb").read() == text.encode()
    kept = {"w%d" % o for o in want["kept_words"].tolist()}
    lines = open(os.path.join(log_dir, "TopWordsPerTopic_catch.txt")).read().split("\n")[:-1]
    assert len(lines) == k
    named = [w for l in lines for w in l.split("\t") if w]
    assert len(named) == 10 * k and set(named) <= kept
    # the summary prints word:id pairs, the id in the pruned numbering: every name is the vocabulary file's line of that id's old word
    import re
    pairs = re.findall(r"(w\d+):(\d+)\(", open(os.path.join(log_dir, "diagnosticLog.txt")).read())
    assert len(pairs) >= 10 * k and all(name == "w%d" % want["kept_words"][int(i)] for name, i in pairs)
    assert any(name != "w" + i for name, i in pairs)   # (the numbering did change: an unmapped vocabulary would fail above)
    line = "Vocabulary pruned: words kept %d dropped %d, entries kept %d dropped %d, documents emptied %d" % (
        want["vocab"], V - want["vocab"], want["nnz"], rows.size - want["nnz"], want["docs_emptied"])
    assert line in r.stdout
