"""The trainer's per-document report files formatted on the device (isle_hip_doc_report_text; HotPath.doc_report_text, write_doc_report,
doc_report_size; isle_amd/csrc/doc_report.hip): DocCatchword.tsv, DocTopicCatchwordSums.tsv (reference order and resident order) and
TopTwoTopicsPerDoc.txt.

The setup is that of tests/test_gpu_post.py.  Every expected text is the numpy restatement of tests/test_doc_report_cpu.py (held there
to a transcription of the reference's writers) applied to what the stage returned: catch_topic, dts_*, top1 / top2, and
O.post_normalize(...) for the values; tests/test_gpu_post.py holds those arrays to the oracle bit for bit.  Texts are compared as whole
bytes.  A tile is 1024 candidate lines, the offsets window 1024 documents, a piece at most CHUNK = 16 MiB."""
import glob
import os
import subprocess

import numpy as np
import pytest

from isle_amd.hot_path import HotPath, IsleHipError
from test_doc_report_cpu import catchwords_text, top_two_text, topic_sums_order, topic_sums_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "isle_amd", "host")
CHUNK = 16 << 20
KINDS = ("catchwords", "topic_sums", "topic_sums_by_doc", "top_two")
_A = {}


def matrix(V, D, k, seed):
    """(corpus, counts, rows, offs) of the synthetic corpus, made once."""
    from tools.synth import Corpus
    if (V, D, k, seed) not in _A:
        c = Corpus(V, D, k, seed)
        _A[(V, D, k, seed)] = (c,) + tuple(c.A())
    return _A[(V, D, k, seed)]


def stage(hp, V, D, k, c, cnt, rows, offs, r=None, assign=None):
    """upload_counts, threshold, the planted assignment, find_catchwords, construct_topic_model -> everything the restatements need"""
    from oracle import oracle as O
    hp.upload_counts(V, cnt, rows, offs)
    info = hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    if assign is None:
        assign = c.planted()[oc].astype(np.uint32)
    r = O.catchword_rank(D, k) if r is None else r
    got = hp.find_catchwords(k, r, assign=assign, fetch_thresholds=False)
    tm = hp.construct_topic_model(k, O.model_rank_threshold(D, k), D)
    return dict(V=V, D=D, k=k, offs=np.asarray(offs, np.int64), rows=rows, nv=O.post_normalize(offs, cnt, info["avg_doc_sz"]), assign=assign, r=r,
                catch_topic=got["catch_topic"], num_catchwords=got["num_catchwords"], tm=tm)


def expected(s, what, docs=None):
    tm = s["tm"]
    if what == "catchwords":
        return catchwords_text(s["catch_topic"], s["offs"], s["rows"], s["nv"], docs)
    if what == "top_two":
        return top_two_text(tm["top1"], tm["top2"], docs)
    return topic_sums_text(tm["dts_off"], tm["dts_topic"], tm["dts_val"], docs, by_doc=what == "topic_sums_by_doc")


def check(hp, s, what, docs=None):
    want = expected(s, what, docs)
    assert hp.doc_report_text(what, docs) == want, (what, docs)
    assert hp.doc_report_size(what, docs) == (len(want), want.count(b"\n")), (what, docs)
    return want


# ---- 1. all four kinds on the whole corpus ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,D,k,seed", [(3000, 12000, 10, 2), (5000, 30000, 20, 3)])
def test_all_kinds_whole_corpus_and_inner_range(hp, V, D, k, seed):
    s = stage(hp, V, D, k, *matrix(V, D, k, seed))
    assert s["num_catchwords"] > 5 * k
    for what in KINDS:
        want = check(hp, s, what)
        assert want
        print("doc_report %s: %d bytes, %d lines" % (what, len(want), want.count(b"\n")))
        check(hp, s, what, docs=(D // 7, D - D // 5))
        assert hp.doc_report_text(what, (0, D)) == want                          # a second call: the same bytes
    from oracle import oracle as O
    again = hp.construct_topic_model(k, O.model_rank_threshold(D, k), D)          # nothing resident was written
    for name in ("dts_off", "dts_topic", "dts_val", "top1", "top2", "model_threshold"):
        assert again[name].tobytes() == s["tm"][name].tobytes(), name


# ---- 2. the reference order against the resident order ---------------------------------------------------------------------------
def test_topic_sums_is_the_stated_order_of_the_resident_lines(hp):
    V, D, k, seed = 3000, 12000, 10, 2
    s = stage(hp, V, D, k, *matrix(V, D, k, seed))
    tm = s["tm"]
    pairs = (tm["dts_topic"].astype(np.uint64) << np.uint64(32)) | tm["dts_val"].view(np.uint32).astype(np.uint64)
    assert np.unique(pairs).size < pairs.size                                    # the case holds a tie on (topic, value)
    assert (tm["dts_val"] > 0).all() and np.isfinite(tm["dts_val"]).all()
    ref = hp.doc_report_text("topic_sums").splitlines(True)
    res = hp.doc_report_text("topic_sums_by_doc").splitlines(True)
    assert sorted(ref) == sorted(res) and len(ref) == tm["num_sums"]             # the same multiset of lines
    doc = np.repeat(np.arange(D), np.diff(tm["dts_off"]))
    o = topic_sums_order(tm["dts_topic"], tm["dts_val"])
    t, v, d = tm["dts_topic"][o].astype(np.int64), tm["dts_val"][o], doc[o]
    same_topic = t[1:] == t[:-1]
    assert (np.diff(t) >= 0).all() and (v[1:][same_topic] <= v[:-1][same_topic]).all()
    tie = same_topic & (v[1:] == v[:-1])
    assert tie.any() and (d[1:][tie] > d[:-1][tie]).all()                        # ties: document ascending
    assert ref == [res[i] for i in o]


# ---- 3. tile edges of the filtered source ----------------------------------------------------------------------------------------
def edited_matrix():
    """The seed-2 matrix with a run of 1100 empty documents (longer than the offsets window), one document cut to a single entry, and
    an empty document at row 0 and at the last row."""
    V, D, k, seed = 3000, 12000, 10, 2
    c, cnt, rows, offs = matrix(V, D, k, seed)
    offs = np.asarray(offs, np.int64)
    lens = np.diff(offs)
    assert lens.min() >= 1 and offs[-1] > 1_000_000                              # no empty document occurs naturally
    keep = np.ones(offs[-1], bool)
    run = (4000, 5100)
    for d in list(range(*run)) + [0, D - 1]:
        keep[offs[d]:offs[d + 1]] = False
    single = 7000
    keep[offs[single] + 1:offs[single + 1]] = False
    new_lens = np.array([keep[offs[d]:offs[d + 1]].sum() for d in range(D)], np.int64)
    new_offs = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.int64)
    assert new_lens[0] == 0 and new_lens[-1] == 0 and new_lens[single] == 1 and (new_lens[run[0]:run[1]] == 0).all() and run[1] - run[0] > 1024
    return V, D, k, c, np.ascontiguousarray(cnt[keep]), np.ascontiguousarray(rows[keep]), new_offs, run, single


def ranges_with(offs, n, lo, hi, count=2):
    """document ranges [b, e) inside [lo, hi) that hold exactly n entries"""
    out = []
    for b in range(lo, hi):
        e = int(np.searchsorted(offs, offs[b] + n))
        if e <= hi and offs[e] - offs[b] == n and offs[b + 1] > offs[b]:
            out.append((b, e))
            if len(out) == count:
                break
    return out


def test_tile_edges_and_empty_documents(hp):
    V, D, k, c, cnt, rows, offs, run, single = edited_matrix()
    s = stage(hp, V, D, k, c, cnt, rows, offs)
    assert s["num_catchwords"] > 5 * k
    docs = []
    for n in (1023, 1024, 1025, 2049):
        found = ranges_with(offs, n, 1, run[0])
        assert len(found) == 2, n                                                # such ranges exist
        docs += found
    docs += [(0, 0), (5, 5), (D, D), (run[0] + 3, run[0] + 3)]                   # ranges of 0 documents
    docs += [(0, 1), (0, 40), (D - 1, D), (D - 30, D), (single, single + 1), (single - 1, single + 2)]
    docs += [(run[0] + 10, run[1] - 10),                                         # only empty documents
             (run[0] + 10, run[1] + 5), (run[0] + 1050, run[1] + 40),            # begin inside the run
             (run[0] - 40, run[0] + 30), (run[0] - 5, run[1] - 1),               # end inside it
             (run[0] - 40, run[1] + 40), (run[0] - 1, run[1] + 1), (0, D)]       # cross it
    for r in docs:
        for what in ("catchwords", "topic_sums_by_doc", "topic_sums", "top_two"):
            want = check(hp, s, what, r)
            if r[0] == r[1] or r == (run[0] + 10, run[1] - 10):
                assert want == b""


# ---- 4. sparse printing ----------------------------------------------------------------------------------------------------------
def without_words(cnt, rows, offs, words):
    """the matrix without the entries of `words`"""
    keep = ~np.isin(rows, np.asarray(words, rows.dtype))
    new_offs = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[np.asarray(offs, np.int64)]
    return np.ascontiguousarray(cnt[keep]), np.ascontiguousarray(rows[keep]), new_offs


def test_few_and_no_catchwords(hp):
    """Raising r alone does not reach 1 .. 5 catchwords on this corpus: measured on the device, the count falls from 656 at r = 200 to 6 at
    r = 1483 and stays 6 up to r = 52627 (beyond every cluster's size the thresholds are the clusters' minima).  So r is raised until the
    count stops falling, and then the test edits the uploaded matrix, as the tile-edge test does: it deletes the entries of all but three of
    the remaining catchwords, and for the empty case the entries of all of them, until the stage finds 1 .. 5 and then none."""
    V, D, k, seed = 3000, 12000, 10, 2
    c, cnt, rows, offs = matrix(V, D, k, seed)
    s = stage(hp, V, D, k, c, cnt, rows, offs)
    r, n, same = s["r"], s["num_catchwords"], 0
    while n > 5 and same < 2 and r < D:                                          # raise r until at most five are left, or no fewer
        r += max(1, r // 4)
        m = hp.find_catchwords(k, r, assign=s["assign"], fetch_thresholds=False)["num_catchwords"]
        same = same + 1 if m == n else 0
        n = m
    A, few = (cnt, rows, offs), None
    for _ in range(8):
        few = stage(hp, V, D, k, c, *A, r=r)
        print("r = %d: %d catchwords in %d entries" % (r, few["num_catchwords"], A[2][-1]))
        if few["num_catchwords"] <= 5:
            break
        A = without_words(*A, np.flatnonzero(few["catch_topic"] >= 0)[3:])
    assert 1 <= few["num_catchwords"] <= 5
    for what in KINDS:
        check(hp, few, what)
        check(hp, few, what, docs=(D // 3, D - 7))
    assert check(hp, few, "catchwords")
    printed = few["catch_topic"][A[1].astype(np.int64)] >= 0
    tiles = printed[:printed.size // 1024 * 1024].reshape(-1, 1024)
    print("tiles of 1024 candidates: %d, without a printed line: %d" % (tiles.shape[0], int((tiles.sum(axis=1) == 0).sum())))
    assert printed.any() and (tiles.sum(axis=1) == 0).any()                      # some tile of 1024 candidates prints nothing

    none = few
    for _ in range(8):
        if none["num_catchwords"] == 0:
            break
        A = without_words(*A, np.flatnonzero(none["catch_topic"] >= 0))
        none = stage(hp, V, D, k, c, *A, r=r)
    assert none["num_catchwords"] == 0
    for what in KINDS:
        seen = []
        assert hp._doc_report_call(what, None, lambda mv: seen.append(bytes(mv))) == (0, 0) and seen == []
        assert hp.doc_report_text(what) == b"" == expected(none, what) and hp.doc_report_size(what) == (0, 0)


# ---- 5. pieces -------------------------------------------------------------------------------------------------------------------
def test_pieces_and_a_refusing_sink(hp, tmp_path):
    V, D, k, seed = 5000, 30000, 20, 3
    s = stage(hp, V, D, k, *matrix(V, D, k, seed))
    for what in KINDS:
        want = expected(s, what)
        parts = []
        nbytes, nlines = hp._doc_report_call(what, None, lambda mv: parts.append(bytes(mv)))
        print("doc_report %s: %d bytes in %d pieces" % (what, len(want), len(parts)))
        assert b"".join(parts) == want and (nbytes, nlines) == (len(want), want.count(b"\n"))
        assert parts and all(0 < len(p) <= CHUNK for p in parts) and all(p.endswith(b"\n") for p in parts)
        assert len(parts) >= (len(want) + CHUNK - 1) // CHUNK
        path = str(tmp_path / what)
        assert hp.write_doc_report(path, what) == (nbytes, nlines) and open(path, "rb").read() == want

        def refuse(mv):
            raise RuntimeError("no")

        with pytest.raises(RuntimeError):
            hp._doc_report_call(what, None, refuse)
    import ctypes as C
    from isle_amd.hot_path import _TEXT_SINK
    seen = []

    def refusing(ptr, n, user):
        seen.append(n)
        return 1

    cb = _TEXT_SINK(refusing)
    rc = hp._lib.isle_hip_doc_report_text(hp._h, 0, 0, D, C.cast(cb, C.c_void_p), None, None, None)
    assert rc != 0 and len(seen) == 1
    with pytest.raises(IsleHipError):
        hp._chk(rc)
    for what in KINDS:
        assert hp.doc_report_text(what) == expected(s, what)                       # the next call works


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_errors():
    from oracle import oracle as O
    V, D, k, seed = 3000, 12000, 10, 2
    c, cnt, rows, offs = matrix(V, D, k, seed)
    h = HotPath(0)
    try:
        for what in KINDS:
            with pytest.raises(IsleHipError):
                h.doc_report_text(what, (0, 0))                                     # no count matrix
        h.upload_counts(V, cnt, rows, offs)
        h.threshold(k)
        assign = c.planted()[h.get_B()["original_cols"].astype(np.int64)].astype(np.uint32)
        for what in KINDS:
            with pytest.raises(IsleHipError):
                h.doc_report_text(what)                                             # before find_catchwords
        h.find_catchwords(k, O.catchword_rank(D, k), assign=assign, fetch_thresholds=False)
        assert h.doc_report_text("catchwords", (0, 50))
        for what in KINDS[1:]:
            with pytest.raises(IsleHipError):
                h.doc_report_text(what)                                             # before construct_topic_model
        h.construct_topic_model(k, O.model_rank_threshold(D, k), D)
        for what in KINDS:
            assert h.doc_report_text(what, (10, 500))
            for bad in ((3, 2), (0, D + 1), (D + 1, D + 1)):
                seen = []
                with pytest.raises(IsleHipError):
                    h._doc_report_call(what, bad, lambda mv: seen.append(bytes(mv)))
                assert seen == []
        for kind in (4, -1):
            with pytest.raises(IsleHipError):
                h._doc_report_call(kind, (0, 10), None)
        with pytest.raises(KeyError):
            h.doc_report_text("sums")
        assert h.doc_report_text("top_two", (0, D))                                # the context is usable after the refusals
        h.upload_counts(V, cnt, rows, offs)                                        # a new count matrix voids both stages
        for what in KINDS:
            with pytest.raises(IsleHipError):
                h.doc_report_text(what, (0, 10))
    finally:
        h.close()


# ---- 7. host mirrors -------------------------------------------------------------------------------------------------------------
def test_trainer_files_and_cpp_host_loops(hp, tmp_path):
    """doc_report_main (a child process): a trainer with print_doctopic = true writes DocCatchword.tsv and DocTopicCatchwordSums.tsv
    from write_model_to_file() and TopTwoTopicsPerDoc.txt from print_top_two_topics(), and holds all four device texts to the C++ host
    loops of trainer_hip.h (exit status 0).  The files equal HotPath's texts for the same corpus under the trainer's partition."""
    from oracle import oracle as O
    from test_cli_cpu import write_tdf
    V, D, k, seed = 1500, 4000, 20, 6
    c, cnt, rows, offs = matrix(V, D, k, seed)
    tdf = str(tmp_path / "corpus.tdf")
    write_tdf(tdf, cnt, rows, offs)
    vocab = str(tmp_path / "vocab.txt")
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([os.path.join(HOST, "doc_report_main"), tdf, vocab, str(out), str(V), str(D), str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count(": equal") == 4 and "DIFFERENT" not in r.stdout
    log_dir = glob.glob(str(out / "*"))[0]
    clusters = np.loadtxt(os.path.join(log_dir, "HotPathClusters.tsv"), dtype=np.int64).reshape(-1, 2) - 1   # (topic, document of A)
    topic_of = np.full(D, -1, np.int64)
    topic_of[clusters[:, 1]] = clusters[:, 0]
    hp.upload_counts(V, cnt, rows, offs)
    hp.threshold(k)
    oc = hp.get_B()["original_cols"].astype(np.int64)
    assert (topic_of[oc] >= 0).all() and clusters.shape[0] == oc.size
    s = stage(hp, V, D, k, c, cnt, rows, offs, assign=topic_of[oc].astype(np.uint32))
    files = {"catchwords": "DocCatchword.tsv", "topic_sums": "DocTopicCatchwordSums.tsv", "topic_sums_by_doc": "DocTopicCatchwordSums_by_doc.tsv",
             "top_two": "TopTwoTopicsPerDoc.txt"}
    for what, name in files.items():
        text = open(os.path.join(log_dir, name), "rb").read()
        assert text and text == hp.doc_report_text(what) == expected(s, what), what
    diag = open(os.path.join(log_dir, "diagnosticLog.txt")).read()
    assert "Total number of catchwords: %d\n" % s["num_catchwords"] in diag
    assert "Writing document catchword weights" in open(os.path.join(log_dir, "timerLog.txt")).read()
