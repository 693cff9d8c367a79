"""The C++ host side of the near-duplicate prune as real processes, each run once under a time limit.  isle_amd/host/near_dups_main.cpp is
built here against the library: `check` holds the device result through FPSparseMatrixHip (signatures, band keys, the sizes of (document,
parent), parent, first_of, the counters, kept_docs, the new A) to the plain loops of isle_amd/csrc/neardup_host.h on a generated corpus
with near and exact copies in it, in both forms of the key, and a refused shape to the header's text; `train` runs a small ISLETrainer
with prune_near_duplicates (isle_amd/host/trainer_hip.h), whose DocsKept.tsv and NearDuplicates.tsv must equal the rule's bytes and whose
training and cluster summary must complete with the new number of documents."""
import glob
import os
import subprocess

import numpy as np
import pytest

import docs_rule as dr
import neardup_rule as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("near_dups_main") / "near_dups_main")
    b = subprocess.run(["g++", "-O2", "-fopenmp", "-std=c++14", "-Wall", "-o", out, os.path.join(HOST, "near_dups_main.cpp"), "-L" + os.path.join(ROOT, "isle_amd"),
                        "-lisle_hip", "-Wl,-rpath," + os.path.join(ROOT, "isle_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


@pytest.mark.parametrize("args,says", [((20000, 6000, 1, 4, 5, 16, 4, 0), "equal the plain loops"),
                                       ((3000, 1500, 2, 2, 3, 13, 5, 1), "equal the plain loops"),
                                       ((500, 300, 3, 4, 5, 17, 8, 0), "refused alike: doc_near_duplicates: bands = 17, rows_per_band = 8")])
def test_the_device_result_is_the_plain_loops(exe, args, says):
    r = subprocess.run([exe, "check"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and says in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    if says.startswith("equal"):
        assert "(near duplicates 0," not in r.stdout          # the generated corpus has copies in it, and they are found


def test_trainer_prunes_near_duplicates_and_trains_on_the_kept_documents(exe, tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    counts, rows, offs = np.asarray(counts, np.float32), np.asarray(rows, np.uint32), np.asarray(offs, np.int64)
    rng = np.random.default_rng(4)
    docs = [(rows[offs[d]:offs[d + 1]].astype(np.int64), counts[offs[d]:offs[d + 1]]) for d in range(D)]
    for d in rng.choice(np.arange(100, D), size=D // 10, replace=False):      # a tenth of the documents: an earlier one with a word in twenty taken out
        w, x = docs[int(rng.integers(0, d))]
        keep = rng.random(w.size) >= 0.05
        if keep.any():
            docs[d] = (w[keep], x[keep])
    offs, rows, counts = dr.csc(V, docs)
    tdf, vocab = str(tmp_path / "corpus.tdf"), str(tmp_path / "vocab.txt")
    write_tdf(tdf, counts, rows, offs)
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "train", tdf, vocab, str(out), str(V), str(D), str(k), "4", "5", "16", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    case = nr.Case("trainer", V, offs, rows, counts, 4, 5, 16, 4, np.zeros((0, 2), np.uint32), "")
    want = nr.rule(case, "full")
    assert 200 < want["n_dropped"] < D // 2
    words, tokens = dr.lengths(offs, counts)
    text = "".join("%d\t%d\t%d\t%d\n" % (n + 1, o + 1, words[o], tokens[o]) for n, o in enumerate(want["kept_docs"].tolist()))
    assert open(os.path.join(log_dir, "DocsKept.tsv"), "rb").read() == text.encode()
    gone = np.flatnonzero(~want["keep"])
    inter, uni = nr.jaccard(offs, rows, np.stack([gone, want["parent"][gone]], axis=1))
    text = "".join("%d\t%d\t%d\t%d\t%d\n" % (d + 1, want["parent"][d] + 1, want["first_of"][d] + 1, i, u) for d, i, u in zip(gone.tolist(), inter.tolist(), uni.tolist()))
    assert open(os.path.join(log_dir, "NearDuplicates.tsv"), "rb").read() == text.encode()
    line = "Near duplicates pruned: kept %d of %d at 4/5, 16 bands of 4, entries kept %d dropped %d" % (want["docs"], D, want["nnz"], rows.size - want["nnz"])
    assert line in r.stdout and "log directory: " in r.stdout     # train() and output_cluster_summary() completed behind the prune
