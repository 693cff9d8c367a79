"""The trainer's three per-document report files (include/isle_hip.h, isle_hip_doc_report_text): DocCatchword.tsv and
DocTopicCatchwordSums.tsv (ISLETrainer::output_doc_topic, src/trainer.cpp:874-991) and TopTwoTopicsPerDoc.txt
(ISLETrainer::print_top_two_topics, :1008-1040).

catchwords_text / topic_sums_text / top_two_text below are the vectorised numpy restatements the GPU tests
(tests/test_gpu_doc_report.py) take as their yardstick, built on doc_lines_text of tests/test_doc_text_cpu.py and a three-integer line
builder made from _uint_field.  They are held here, byte for byte, to a plain Python transcription of the three reference writers
(the merge walk of :946-964; the comparator of src/sparseMatrix.cpp:715-718 with the tie rule "equal (topic, value): document
ascending"; print_top_two_topics), and the three-integer line to the library's host formatter isle_hip_top_two_line_text
(isle_amd.hot_path.top_two_line_text), compiled from the functions the kernels of isle_amd/csrc/doc_report.hip compile.
No GPU."""
import functools

import numpy as np
import pytest

from isle_amd.hot_path import top_two_line_text
from test_doc_text_cpu import NUM_END, concat_float, concat_int, doc_lines_text
from test_model_text_cpu import _const, _uint_field


# ---- the vectorised restatements -----------------------------------------------------------------------------------------------
def int3_lines_text(a, b, c, block=1 << 20):
    """The lines "<a>\\t<b>\\t<c>\\n" of three integers as printed -> bytes.  ValueError for a number >= 0x7fffffff."""
    a, b, c = (np.asarray(x, np.int64).reshape(-1) for x in (a, b, c))
    assert a.shape == b.shape == c.shape
    if any(((x < 0) | (x >= NUM_END)).any() for x in (a, b, c)):
        raise ValueError("a printed number is >= 0x7fffffff")
    out = []
    for s in range(0, a.size, block):
        n = a[s:s + block].size
        parts = [_uint_field(a[s:s + block], 10), _const(n, "\t"), _uint_field(b[s:s + block], 10), _const(n, "\t"), _uint_field(c[s:s + block], 10),
                 _const(n, "\n")]
        out.append(np.hstack([p[0] for p in parts])[np.hstack([p[1] for p in parts])].tobytes())
    return b"".join(out)


def _range(offs, docs):
    offs = np.asarray(offs, np.int64)
    return offs, ((0, offs.size - 1) if docs is None else (int(docs[0]), int(docs[1])))


def catchwords_text(catch_topic, offs, rows, nv, docs=None):
    """ISLE_DOCREPORT_CATCHWORDS: every entry of documents (begin, end) of A whose word has catch_topic >= 0, in stored order."""
    offs, (b, e) = _range(offs, docs)
    doc = np.repeat(np.arange(b, e, dtype=np.int64), np.diff(offs[b:e + 1]))
    w = np.asarray(rows[offs[b]:offs[e]], np.int64)
    keep = np.asarray(catch_topic)[w] >= 0
    return doc_lines_text(doc[keep] + 1, w[keep] + 1, np.asarray(nv, np.float32)[offs[b]:offs[e]][keep])


def topic_sums_order(topic, val):
    """The order of ISLE_DOCREPORT_TOPIC_SUMS over entries given (document, topic) ascending: topic ascending, value descending, the
    earlier entry first among equal pairs.  Every value is positive and finite: its bit pattern is monotone."""
    bits = np.asarray(val, np.float32).view(np.uint32).astype(np.int64)
    return np.lexsort((-bits, np.asarray(topic, np.int64)))   # lexsort is stable: ties keep the given order


def topic_sums_text(dts_off, dts_topic, dts_val, docs=None, by_doc=False):
    """ISLE_DOCREPORT_TOPIC_SUMS (by_doc: ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC) for the CSR construct_topic_model returned."""
    offs, (b, e) = _range(dts_off, docs)
    doc = np.repeat(np.arange(b, e, dtype=np.int64), np.diff(offs[b:e + 1]))
    t = np.asarray(dts_topic[offs[b]:offs[e]], np.int64)
    v = np.asarray(dts_val[offs[b]:offs[e]], np.float32)
    if not by_doc:
        o = topic_sums_order(t, v)
        doc, t, v = doc[o], t[o], v[o]
    return doc_lines_text(doc + 1, t + 1, v)


def top_two_text(top1, top2, docs=None):
    """ISLE_DOCREPORT_TOP_TWO: documents ascending, those with both topics."""
    t1, t2 = np.asarray(top1, np.int64), np.asarray(top2, np.int64)
    b, e = (0, t1.size) if docs is None else docs
    d = np.arange(b, e, dtype=np.int64)
    keep = (t1[b:e] >= 0) & (t2[b:e] >= 0)
    return int3_lines_text(d[keep] + 1, t1[b:e][keep] + 1, t2[b:e][keep] + 1)


# ---- a plain transcription of the reference's writers ------------------------------------------------------------------------
def ref_doc_catchword(catchword_topics, offs, rows, nv):
    """src/trainer.cpp:884-885, :946-964.  catchword_topics: (word, topic) pairs in any order."""
    catchword_topics = sorted(catchword_topics, key=lambda p: p[0])
    out = []
    for doc in range(len(offs) - 1):
        w = 0
        for pos in range(offs[doc], offs[doc + 1]):
            while w != len(catchword_topics) and catchword_topics[w][0] < rows[pos]:
                w += 1
            if w == len(catchword_topics):
                continue
            if rows[pos] == catchword_topics[w][0]:
                out.append(concat_int(doc + 1) + "\t" + concat_int(catchword_topics[w][0] + 1) + "\t" + concat_float(nv[pos]) + "\n")
    return "".join(out).encode("ascii")


def ref_doc_topic_sums(doc_topic_sum):
    """src/sparseMatrix.cpp:715-718 on the (doc, topic, value) triples as :673-681 emits them ((doc, topic) ascending), then
    src/trainer.cpp:979-983.  The comparator leaves equal (topic, value) pairs unordered; the tie rule of this project: document
    ascending (a stable sort)."""
    def less(l, r):
        return l[1] < r[1] or (l[1] == r[1] and l[2] > r[2])

    ordered = sorted(doc_topic_sum, key=functools.cmp_to_key(lambda l, r: -1 if less(l, r) else (1 if less(r, l) else 0)))
    return "".join(concat_int(d + 1) + "\t" + concat_int(t + 1) + "\t" + concat_float(v) + "\n" for d, t, v in ordered).encode("ascii")


def ref_top_two(top_topic_pairs):
    """src/trainer.cpp:1011-1013, :1029-1035.  top_topic_pairs: (top1, top2, doc) of the documents that have both (:703-706)."""
    ordered = sorted(top_topic_pairs, key=lambda p: p[2])
    return "".join(concat_int(d + 1) + "\t" + concat_int(a + 1) + "\t" + concat_int(b + 1) + "\n" for a, b, d in ordered).encode("ascii")


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def draw(seed, V=60, D=90, k=7, ncatch=15, one_topic_docs=False, ties=False):
    """A small random A (CSC over documents, rows ascending, some documents empty) with normalised values, a catchword map, and the
    (document, topic) sums, top-two topics that follow from them by the reference's rules (src/sparseMatrix.cpp:661-708)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, size=D)
    lens[rng.integers(0, D, size=5)] = 0
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)
    if ties:   # few distinct values: equal (topic, value) pairs in different documents
        nv = rng.choice(np.array([0.5, 1.25, 3.0], np.float32), size=rows.size)
    else:
        nv = (rng.integers(1, 0x3f800000, size=rows.size, dtype=np.uint32).view(np.float32) * np.float32(40)).astype(np.float32)
    catch_topic = np.full(V, -1, np.int32)
    words = rng.choice(V, size=ncatch, replace=False)
    catch_topic[words] = 0 if one_topic_docs else rng.integers(0, k, size=ncatch)
    dts_off, dts_topic, dts_val = [0], [], []
    top1, top2 = np.full(D, -1, np.int32), np.full(D, -1, np.int32)
    for d in range(D):
        sums = np.zeros(k, np.float32)
        for pos in range(offs[d], offs[d + 1]):
            if catch_topic[rows[pos]] >= 0:
                sums[catch_topic[rows[pos]]] += nv[pos]
        mx = mx2 = np.float32(0)
        for t in range(k):
            if sums[t]:
                dts_topic.append(t)
                dts_val.append(sums[t])
                if sums[t] > mx:
                    mx2, top2[d] = mx, top1[d]
                    mx, top1[d] = sums[t], t
                elif sums[t] > mx2:
                    mx2, top2[d] = sums[t], t
        dts_off.append(len(dts_topic))
    return dict(offs=offs, rows=rows, nv=nv, catch_topic=catch_topic, dts_off=np.array(dts_off, np.int64), dts_topic=np.array(dts_topic, np.uint32),
                dts_val=np.array(dts_val, np.float32), top1=top1, top2=top2, D=D)


CASES = {"plain": dict(seed=1), "plain2": dict(seed=2, V=200, D=150, k=11, ncatch=60), "ties": dict(seed=3, ties=True),
         "no_catchwords": dict(seed=4, ncatch=0), "one_topic": dict(seed=5, one_topic_docs=True)}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    return request.param, draw(**CASES[request.param])


def test_inputs_are_what_they_should_be():
    c = {name: draw(**kw) for name, kw in CASES.items()}
    tie = c["ties"]
    pairs = list(zip(tie["dts_topic"].tolist(), tie["dts_val"].view(np.uint32).tolist()))
    assert len(set(pairs)) < len(pairs)                                  # equal (topic, value) pairs
    assert (c["no_catchwords"]["catch_topic"] < 0).all() and c["no_catchwords"]["dts_topic"].size == 0
    one = c["one_topic"]
    assert (one["top1"] >= 0).any() and (one["top2"] < 0).all()          # documents with only one topic: no line
    assert ((c["plain"]["top1"] >= 0) & (c["plain"]["top2"] < 0)).any() and (c["plain"]["top2"] >= 0).any()
    assert (np.diff(c["plain"]["offs"]) == 0).any()


def test_catchwords_restatement_equals_the_merge_walk(case):
    name, c = case
    ct = c["catch_topic"]
    pairs = [(int(w), int(ct[w])) for w in np.flatnonzero(ct >= 0)][::-1]
    want = ref_doc_catchword(pairs, c["offs"].tolist(), c["rows"].tolist(), c["nv"])
    assert catchwords_text(ct, c["offs"], c["rows"], c["nv"]) == want
    assert (want == b"") == (name == "no_catchwords")
    b, e = 7, c["D"] - 9
    inner = ref_doc_catchword(pairs, (c["offs"][b:e + 1] - c["offs"][b]).tolist(), c["rows"][c["offs"][b]:].tolist(), c["nv"][c["offs"][b]:])
    shifted = b"".join(b"%d\t%s" % (int(ln.split(b"\t", 1)[0]) + b, ln.split(b"\t", 1)[1]) for ln in inner.splitlines(True))
    assert catchwords_text(ct, c["offs"], c["rows"], c["nv"], docs=(b, e)) == shifted


def test_topic_sums_restatement_equals_the_comparator_with_the_tie_rule(case):
    name, c = case
    doc = np.repeat(np.arange(c["D"]), np.diff(c["dts_off"]))
    triples = list(zip(doc.tolist(), c["dts_topic"].tolist(), c["dts_val"]))
    assert topic_sums_text(c["dts_off"], c["dts_topic"], c["dts_val"]) == ref_doc_topic_sums(triples)
    by_doc = topic_sums_text(c["dts_off"], c["dts_topic"], c["dts_val"], by_doc=True)
    assert by_doc == "".join(concat_int(d + 1) + "\t" + concat_int(t + 1) + "\t" + concat_float(v) + "\n" for d, t, v in triples).encode("ascii")
    assert sorted(by_doc.splitlines()) == sorted(ref_doc_topic_sums(triples).splitlines())
    b, e = 7, c["D"] - 9
    inner = [x for x in triples if b <= x[0] < e]
    assert topic_sums_text(c["dts_off"], c["dts_topic"], c["dts_val"], docs=(b, e)) == ref_doc_topic_sums(inner)


def test_top_two_restatement_equals_print_top_two_topics(case):
    name, c = case
    pairs = [(int(a), int(b), d) for d, (a, b) in enumerate(zip(c["top1"], c["top2"])) if a >= 0 and b >= 0]
    want = ref_top_two(pairs[::-1])
    assert top_two_text(c["top1"], c["top2"]) == want
    assert (want == b"") == (name in ("no_catchwords", "one_topic"))
    b, e = 7, c["D"] - 9
    assert top_two_text(c["top1"], c["top2"], docs=(b, e)) == ref_top_two([p for p in pairs if b <= p[2] < e])


EDGES = (1, 9, 10, 0x7ffffffe)


def test_top_two_line_text_equals_the_transcription_at_the_digit_edges():
    for a in EDGES:
        for b in EDGES:
            for c in EDGES:
                want = (concat_int(a) + "\t" + concat_int(b) + "\t" + concat_int(c) + "\n").encode("ascii")
                assert top_two_line_text(a, b, c) == want == int3_lines_text([a], [b], [c])
    assert top_two_line_text(1, 9, 10) == b"1\t9\t10\n"
    for bad in ((0x7fffffff, 1, 1), (1, 0x7fffffff, 1), (1, 1, 0x7fffffff), (2 ** 40, 1, 1)):
        assert top_two_line_text(*bad) == -1
        with pytest.raises(ValueError):
            int3_lines_text(*[[x] for x in bad])
    from isle_amd._lib import load_library
    assert load_library().isle_hip_top_two_line_text(1, 1, 1, None) == -1
