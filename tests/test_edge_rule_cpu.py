"""The host statements of the edge-topic stage, no GPU: fpsparse_detail::select_edge_pairs_host (isle_amd/host/fpsparse_hip.h) and the
builders of EdgeTopicComposition.txt / EdgeTopicTopWords.txt (trainer_detail::edge_composition_text / edge_top_words_text,
isle_amd/host/trainer_hip.h; print_edge_topic_composition / print_edge_topic_top_words, src/trainer.cpp:1169-1245) against
hot_path.select_edge_pairs and the Python restatement of the two files below, on drawn inputs.  The C++ side is reached through
isle_amd/host/edge_report_main, a stand-alone program the test compiles itself with -fsanitize=address,undefined (it links nothing of
the library and touches no device), and through edge_select_main --host-only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from isle_amd import hot_path as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")


def composition_text(pairs):
    """EdgeTopicComposition.txt: "<primary>\\t<secondary>\\t<documents>\\n", 0-based topic ids."""
    return "".join("%d\t%d\t%d\n" % (p, s, c) for p, s, c in np.asarray(pairs, np.int64).tolist())


def top_words_text(pairs, vocab, edge_ids, edge_w, topic_ids, topic_w):
    """EdgeTopicTopWords.txt (src/trainer.cpp:1207-1243).  edge_ids / edge_w: (n_edge, 20) top words of the edge topics; topic_ids /
    topic_w: (k, 10) top words of every basic topic; weights as operator<< prints a float: '%g'."""
    def entries(ids, w):
        return "".join("%s(%d,%s)\t" % (vocab[int(i)], int(i), "%g" % float(x)) for i, x in zip(ids, w))
    out = []
    for t, (p, s, c) in enumerate(np.asarray(pairs, np.int64).tolist()):
        out.append("Edge Topic: %d  (%d, %d): %d\n" % (t, p, s, c))
        out.append("Top words in edge_topic: \n" + entries(edge_ids[t], edge_w[t]) + "\n")
        out.append("Top words in topic: %d\n" % p + entries(topic_ids[p], topic_w[p]) + "\n")
        out.append("Top words in topic: %d\n" % s + entries(topic_ids[s], topic_w[s]) + "\n\n")
    return "".join(out)


def top_words_with_weights(model, n):
    ids = H.top_words(model, n)
    return ids, np.asarray(model)[ids.astype(np.int64), np.arange(ids.shape[0])[:, None]].astype(np.float32)


def draw(n, k, seed):
    g = np.random.default_rng(seed)
    t = [np.minimum((k * g.random(n) ** 3).astype(np.int32), k - 1) for _ in range(2)]
    for a in t:
        a[g.random(n) < 0.1] = -1
    return t


# (documents, topics, max_edge_topics, min_docs, vocabulary): a dozen, with empty inputs, cuts inside ties and nothing cut
CASES = [(0, 3, 5, 1, 30), (1, 1, 5, 1, 25), (40, 2, 0, 1, 20), (300, 4, 3, 1, 40), (300, 4, 100, 1, 21), (2000, 9, 17, 2, 64), (2000, 9, 17, 50, 64),
         (5000, 30, 60, 1, 100), (5000, 30, 10 ** 6, 3, 33), (777, 13, 12, 1, 20), (50, 50, 7, 1, 57), (10000, 5, 24, 1, 200)]


@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    """edge_report_main built with the address and undefined-behaviour sanitizers (host code only, run here)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build isle_amd/host/edge_report_main.cpp"
    exe = str(tmp_path_factory.mktemp("edge_rule") / "edge_report_main_san")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++14", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(HOST, "edge_report_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("n,k,max_edge,min_docs,V", CASES)
def test_host_rule_and_report_builders(report_main, tmp_path, n, k, max_edge, min_docs, V):
    t1, t2 = draw(n, k, n + k)
    pairs = H.select_edge_pairs(t1, t2, max_edge, min_docs)
    every = H.select_edge_pairs(t1, t2, 1 << 62, min_docs)
    g = np.random.default_rng(V)
    model = np.asfortranarray((g.integers(0, 50, (V, k)) * (g.random((V, k)) < 0.5)).astype(np.float32) / np.float32(1024))
    model[:, 0] *= np.float32(1e-3)                                              # weights '%g' prints with an exponent
    edge = (np.float32(0.75) * model[:, pairs[:, 0]] + np.float32(0.25) * model[:, pairs[:, 1]]).astype(np.float32)
    e_ids, e_w = top_words_with_weights(edge, 20)
    t_ids, t_w = top_words_with_weights(model, 10)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        np.array([n, max_edge, min_docs, k, pairs.shape[0], e_ids.shape[1], t_ids.shape[1]], np.int64).tofile(f)
        for a in (t1, t2, e_ids, e_w, t_ids, t_w):
            np.ascontiguousarray(a).tofile(f)
    comp, words = tmp_path / "comp.txt", tmp_path / "words.txt"
    r = subprocess.run([report_main, str(inp), str(comp), str(words)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    thr = int(every[max_edge, 2]) if every.shape[0] > max_edge else 0
    assert r.stdout.split() == ["candidates", str(every.shape[0]), "threshold", str(thr), "selected", str(pairs.shape[0])]
    assert comp.read_bytes().decode() == composition_text(pairs)
    vocab = ["w%d" % i for i in range(V)]
    assert words.read_bytes().decode() == top_words_text(pairs, vocab, e_ids, e_w, t_ids, t_w)


@pytest.mark.parametrize("n,k,max_edge,min_docs", [(1000, 50, 20, 1), (20000, 7, 1000, 2)])
def test_edge_select_main_host_only(tmp_path, n, k, max_edge, min_docs):
    """The yardstick's own draw through its host side alone: the triples it writes follow the rule on the pairs it was given."""
    t1, t2 = draw(n, k, 5)
    inp, out = tmp_path / "pairs.i32", tmp_path / "triples.txt"
    with open(inp, "wb") as f:
        t1.tofile(f)
        t2.tofile(f)
    r = subprocess.run([os.path.join(HOST, "edge_select_main"), str(n), str(k), str(max_edge), "0", "--min-docs", str(min_docs), "--host-only", "--input",
                        str(inp), "--triples", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = H.select_edge_pairs(t1, t2, max_edge, min_docs)
    lines = out.read_text().splitlines()
    got = np.array([[int(x) for x in ln.split()] for ln in lines[:-1]], np.int64).reshape(-1, 3)
    np.testing.assert_array_equal(got, want)
    every = H.select_edge_pairs(t1, t2, 1 << 62, min_docs)
    assert lines[-1] == "candidates %d threshold %d" % (every.shape[0], int(every[max_edge, 2]) if every.shape[0] > max_edge else 0)
    assert r.stdout.strip() == "host: %d documents, %d candidates, %d selected" % (n, every.shape[0], want.shape[0])
