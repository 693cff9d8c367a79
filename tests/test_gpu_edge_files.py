"""The two report files of the edge-topic stage as ISLETrainer::train_edge_topics writes them (isle_amd/host/trainer_hip.h;
construct_edge_topics_v2's print_edge_topic_composition / print_edge_topic_top_words, src/trainer.cpp:1163-1245): trainer_model_text_main
runs the ISLETrain sequence with edge topics on and dumps the floats of its models; EdgeTopicComposition.txt and EdgeTopicTopWords.txt
must be, byte for byte, the Python restatement (tests/test_edge_rule_cpu.py) over those floats and the vocabulary.  The pairs were
selected on the device from the resident top-two topics, the edge topics' words from the catch model's columns without an edge model.
Sizes compared: V = 1500 words, 4000 documents, 20 topics, at most 30 edge topics.
Then the yardstick of the selection, edge_select_main: host rule against device entry, entry for entry."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli_cpu import write_tdf
from test_edge_rule_cpu import composition_text, top_words_text, top_words_with_weights
from tools.synth import Corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def run_trainer(tmp_path, V, D, k, max_edge, seed):
    """The corpus as a tdf file, trainer_model_text_main on it -> (stdout, log directory, dump prefix, vocabulary)."""
    c = Corpus(V, D, k, seed=seed)
    counts, rows, offs = c.A()
    tdf = str(tmp_path / "corpus.tdf")
    n = write_tdf(tdf, counts, rows, offs)
    words = ["w%d" % i for i in range(V)]
    vocab = str(tmp_path / "vocab.txt")
    open(vocab, "w").write("\n".join(words))
    out = tmp_path / "out"
    out.mkdir()
    dump = str(tmp_path / "dump")
    r = subprocess.run([os.path.join(HOST, "trainer_model_text_main"), tdf, vocab, str(out), str(V), str(D), str(n), str(k), str(max_edge), dump],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, glob.glob(str(out / "*"))[0], dump, words


def check_files(stdout, log_dir, dump, words, V, D, k, max_edge):
    ne = int(open(dump + ".nedge").read())
    catch = np.fromfile(dump + ".catch.f32", np.float32).reshape(V, k, order="F")
    edge = np.fromfile(dump + ".edge.f32", np.float32).reshape(V, ne, order="F")
    comp = open(os.path.join(log_dir, "EdgeTopicComposition.txt"), "rb").read().decode()
    pairs = np.array([[int(x) for x in ln.split("\t")] for ln in comp.splitlines()], np.int64).reshape(-1, 3)
    # the pairs against the log: their number, the candidates, the order of the rule, the threshold where something was cut
    m = re.search(r"#Candidates for edge topics: (\d+)\n(?:Edge topic threshold: (\d+)\n)?#Edge topics: (\d+)\nCompleted edge topic construction\n", stdout)
    assert m, stdout[-2000:]
    cand = int(m.group(1))
    assert int(m.group(3)) == ne == pairs.shape[0] == min(cand, max_edge) and 0 < ne
    assert (m.group(2) is not None) == (cand > ne)
    if cand > ne:
        assert int(m.group(2)) <= pairs[-1, 2]
    assert pairs[:, :2].min() >= 0 and pairs[:, :2].max() < k and pairs[:, 2].min() >= 1 and pairs[:, 2].sum() <= D
    key = [(-c, p, s) for p, s, c in pairs.tolist()]
    assert key == sorted(key) and len(set(key)) == len(key)
    assert comp == composition_text(pairs)
    e_ids, e_w = top_words_with_weights(edge, 20)
    t_ids, t_w = top_words_with_weights(catch, 10)
    got = open(os.path.join(log_dir, "EdgeTopicTopWords.txt"), "rb").read().decode()
    assert len(got) > 0 and got == top_words_text(pairs, words, e_ids, e_w, t_ids, t_w)
    return pairs


def test_trainer_writes_the_two_edge_report_files(tmp_path):
    V, D, k, max_edge = 1500, 4000, 20, 30
    stdout, log_dir, dump, words = run_trainer(tmp_path, V, D, k, max_edge, 6)
    pairs = check_files(stdout, log_dir, dump, words, V, D, k, max_edge)
    text = open(os.path.join(log_dir, "EdgeTopicTopWords.txt")).read()
    assert text.count("Top words in edge_topic: \n") == pairs.shape[0] and text.count("\t") == 40 * pairs.shape[0]


@pytest.mark.parametrize("n,k,max_edge", [(1000, 50, 100), (300000, 50, 1000)])
def test_edge_select_main_host_and_device_agree(n, k, max_edge):
    r = subprocess.run([os.path.join(HOST, "edge_select_main"), str(n), str(k), str(max_edge), "11"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    m = re.fullmatch(r"identical: (\d+) documents, (\d+) candidates, (\d+) selected", r.stdout.strip())
    assert m and int(m.group(1)) == n and int(m.group(3)) == min(int(m.group(2)), max_edge) > 0
