"""Inference and the per-document reports on document shards (N > 1 ranks), held against the single-rank run on the whole corpus: the
corpus, the layouts, what every rank must deliver, the per-rank worker and the certificate (no GPU needed to import this module; the
worker alone opens the device; tests/rank_launch.py starts the ranks).

The rule: the ranks' outputs side by side in rank order are what one rank gives on the whole corpus, byte for byte and bit for bit.
The expected bytes of the four report kinds come from the host statements of tests/test_doc_report_cpu.py (catchwords_text,
topic_sums_text / topic_sums_order, top_two_text) applied to the plain single-rank arrays of stages_certificate.post_reference and cut
at the bounds; the inference texts from doc_lines_text (tests/test_doc_text_cpu.py, held there to hot_path.doc_line_text) applied to
the single-rank inference result.  Nothing expected comes from the sharded device path.

The corpus (corpus()): D = 2301 documents, V = 200 words, 7 topics.
  [0, 700)      drawn documents of a main and a second topic, document 0 forty times as long, document 50 empty
  [700, 1100)   400 IDENTICAL documents of cluster 3 with catchwords of the topics 3 and 5: two runs of 400 bit-equal (topic, value) pairs
  [1100, 1150)  drawn documents
  [1150, 2200)  1050 empty documents (more than IT_WIN = 1024)
  [2200, 2301)  drawn documents four times as long (the shards' mean sizes differ)
Layouts (rank q holds the documents [bounds[q], bounds[q + 1])):
  H2  2 ranks  [0, 1150, D]         an odd cut (1150 | 1151) with the run of empty documents right behind it
  E3  3 ranks  [0, 1, D, D]         a one-document shard, and an empty one beside the rest
  E4  4 ranks  [0, 0, 767, 767, D]  an empty first and an empty middle shard; the cut lies inside the identical documents
  C4  4 ranks  [0, 8, 98, 998, D]   shards that begin at the documents 8, 98 and 998: their first lines cross 9 -> 10, 99 -> 100 and
                                    999 -> 1000 printed digits; the cut at 998 lies inside the identical documents
  W1  1 rank   a communicator of one rank: the launches of a context without one; the single-rank inference result comes from here
layout_facts() states from the reference alone what the cuts must hit; tests/test_doc_shard_cases_cpu.py asserts it."""
import numpy as np

import rank_launch
import shard_cases as sc
import stages_certificate as stc
from test_doc_report_cpu import catchwords_text, top_two_text, topic_sums_order, topic_sums_text
from test_doc_text_cpu import doc_lines_text

F = np.float32
RHO = 1.1
MT_TILE, IT_WIN = 1024, 1024  # text_format.h, doc_text.h
V, TOPICS, D = 200, 7, 2301
TIES, EMPTY_RUN, LONG = (700, 1100), (1150, 2200), (2200, 2301)
LAYOUTS = ("H2", "E3", "E4", "C4", "W1")
WORLD = {"H2": 2, "E3": 3, "E4": 4, "C4": 4, "W1": 1}
KINDS = ("catchwords", "topic_sums", "topic_sums_by_doc", "top_two")
INFER_KINDS = ("entries", "top")
INNER_CHUNK = 100  # chunk_docs of the inner-range inference: splits every range longer than that
FEW = (TIES[0], TIES[0] + 1)  # L < W: rank 0 asks for the sums of one document (two sums), every other rank for none
SEED = 24  # of the drawn documents: one at which the number of sums L is no multiple of 2, 3 or 4 (layout_facts)
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# the corpus and its single-rank reference
# ---------------------------------------------------------------------------------------------------------------------------------
def corpus():
    """-> the case (stages_certificate's dict: V, cnt, rows, offs, k, topics, r, rank, B, assign, cl, nv)."""
    if "case" in _CACHE:
        return _CACHE["case"]
    rng = np.random.default_rng(SEED)
    own = lambda t: np.arange(25 * t, 25 * t + 20)  # noqa: E731
    shared = np.arange(175, 200)

    def drawn(t, scale):
        t2 = int((t + 1 + rng.integers(0, TOPICS - 1)) % TOPICS)
        d = {}
        for w in rng.choice(own(t), size=int(rng.integers(6, 12)), replace=False):
            d[int(w)] = int(rng.integers(4, 10)) * scale
        for w in rng.choice(own(t2), size=int(rng.integers(2, 5)), replace=False):
            d[int(w)] = int(rng.integers(1, 3)) * scale
        for w in rng.choice(shared, size=int(rng.integers(2, 6)), replace=False):
            d[int(w)] = int(rng.integers(1, 4)) * scale
        return d

    same = {int(w): 5 for w in own(3)[:8]}
    same.update({int(w): 1 for w in own(5)[:3]})
    docs, want = [], []
    for d in range(D):
        t = int(rng.integers(0, TOPICS))
        if d == 50 or EMPTY_RUN[0] <= d < EMPTY_RUN[1]:
            docs.append({})
            want.append(0)
        elif TIES[0] <= d < TIES[1]:
            docs.append(dict(same))
            want.append(3)
        else:
            docs.append(drawn(t, 40 if d == 0 else 4 if d >= LONG[0] else 1))  # document 0 alone moves the corpus average (layout E3)
            want.append(t)
    case = stc._csc(V, docs)
    case.update(k=TOPICS, topics=TOPICS, r=5, rank=3)
    _CACHE["case"] = stc._finish_post(case, want)
    return _CACHE["case"]


def reference():
    """The single-rank arrays of the reports: stages_certificate.post_reference on the whole corpus."""
    case = corpus()
    return stc.post_reference(case, r=case["r"], rho=RHO, rank=case["rank"])


def infer_model():
    """The host model of the inference runs, (V, 7) F-order float32: the same array in every launch (the catch model is summed over the
    ranks in fp32 and differs between layouts in its last bits, so it cannot carry a bit-for-bit statement across launches)."""
    rng = np.random.default_rng(3)
    M = (rng.random((V, TOPICS)) * 0.02 + 0.001).astype(np.float64)
    for t in range(TOPICS):
        M[25 * t:25 * t + 20, t] += 1.0 + rng.random(20)
    return np.asfortranarray((M / M.sum(axis=0)).astype(F))


def bounds(layout):
    return np.array({"H2": [0, EMPTY_RUN[0], D], "E3": [0, 1, D, D], "E4": [0, 0, 767, 767, D], "C4": [0, 8, 98, 998, D], "W1": [0, D]}[layout], np.int64)


def slice_py(L, W, q):
    """The first line of rank q's part of L lines over W ranks (stage_host.h topic_sums_slice, restated)."""
    return q * (L // W) + min(q, L % W)


def inner_range(Dq):
    """The inner range (b, e) of a shard of Dq documents that the inner-range inference covers."""
    b = min(3, Dq)
    return b, max(Dq - 2, b)


def shard_avg(case, d0, d1):
    """floor(tokens / non-empty documents) of the documents [d0, d1) alone, and the two totals"""
    offs = case["offs"]
    tokens = int(np.asarray(case["cnt"][offs[d0]:offs[d1]], np.int64).sum())
    nz = int((np.diff(offs[d0:d1 + 1]) > 0).sum())
    return tokens // max(nz, 1), tokens, nz


def sums_of(dts, ranges):
    """(document, topic, value) of the sums of the documents of `ranges` ((begin, end) in the corpus's numbering, ascending)"""
    off = dts["dts_off"]
    doc_of = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    at = np.concatenate([np.arange(off[b], off[e]) for b, e in ranges] + [np.zeros(0, np.int64)]).astype(np.int64)
    return doc_of[at], np.asarray(dts["dts_topic"], np.int64)[at], np.asarray(dts["dts_val"], F)[at]


def topic_sums_lines(dts, ranges):
    """The lines of ISLE_DOCREPORT_TOPIC_SUMS over the sums of `ranges` as ONE order: a list of the lines' bytes"""
    doc, t, v = sums_of(dts, ranges)
    o = topic_sums_order(t, v)
    return doc_lines_text(doc[o] + 1, t[o] + 1, v[o]).splitlines(True)


def cut_lines(lines, W):
    return [b"".join(lines[slice_py(len(lines), W, q):slice_py(len(lines), W, q + 1)]) for q in range(W)]


def pieces(text_of_range, bnd):
    return [text_of_range((int(bnd[q]), int(bnd[q + 1]))) for q in range(len(bnd) - 1)]


def expected_reports(layout):
    """kind -> the bytes every rank must deliver, in rank order, plus "few" and "none" (topic_sums over small ranges).  The three
    kinds without a collective are the single-rank text of the rank's documents; topic_sums is the corpus's file cut at the slices."""
    key = ("expected", layout)
    if key in _CACHE:
        return _CACHE[key]
    case, R, bnd = corpus(), reference(), bounds(layout)
    dts, W = R["dts"], WORLD[layout]
    whole = topic_sums_text(dts["dts_off"], dts["dts_topic"], dts["dts_val"])
    lines = topic_sums_lines(dts, [(0, D)])
    assert b"".join(lines) == whole
    out = {
        "catchwords": pieces(lambda r: catchwords_text(R["catch_topic"], case["offs"], case["rows"], case["nv"], docs=r), bnd),
        "topic_sums_by_doc": pieces(lambda r: topic_sums_text(dts["dts_off"], dts["dts_topic"], dts["dts_val"], docs=r, by_doc=True), bnd),
        "top_two": pieces(lambda r: top_two_text(dts["top1"], dts["top2"], docs=r), bnd),
        "topic_sums": cut_lines(lines, W),
        "few": cut_lines(topic_sums_lines(dts, few_ranges(layout)), W),
        "none": [b""] * W,
    }
    _CACHE[key] = out
    return out


def few_ranges(layout):
    """The documents (corpus numbering) whose sums the "few" call orders: FEW where a rank holds it, nothing elsewhere"""
    bnd = bounds(layout)
    return [(max(FEW[0], int(bnd[q])), min(FEW[1], int(bnd[q + 1]))) for q in range(len(bnd) - 1) if max(FEW[0], int(bnd[q])) < min(FEW[1], int(bnd[q + 1]))]


def few_local(layout, q):
    """docs of rank q's "few" call in its own numbering"""
    bnd = bounds(layout)
    b, e = max(FEW[0], int(bnd[q])), min(FEW[1], int(bnd[q + 1]))
    return (b - int(bnd[q]), e - int(bnd[q])) if b < e else (0, 0)


def none_local(layout, q):
    """docs of rank q's "none" call: what it holds of the run of empty documents (no sums anywhere)"""
    bnd = bounds(layout)
    b, e = max(EMPTY_RUN[0], int(bnd[q])), min(EMPTY_RUN[1], int(bnd[q + 1]))
    return (b - int(bnd[q]), e - int(bnd[q])) if b < e else (0, 0)


def layout_facts(layout):
    """What the cuts of a layout hit, from the reference alone."""
    case, R, bnd = corpus(), reference(), bounds(layout)
    dts, W = R["dts"], WORLD[layout]
    doc, t, v = sums_of(dts, [(0, D)])
    o = topic_sums_order(t, v)
    doc, t, bits = doc[o], t[o], v[o].view(np.uint32)
    L = len(o)
    rank_of = sc.rank_of_doc(bnd, doc)
    run_start = np.flatnonzero(np.concatenate([[True], (t[1:] != t[:-1]) | (bits[1:] != bits[:-1])]))
    run_id = np.cumsum(np.concatenate([[True], (t[1:] != t[:-1]) | (bits[1:] != bits[:-1])])) - 1
    cut_in_ties = []      # slice boundaries strictly inside a run of equal (topic, value) pairs whose documents lie on two ranks
    for q in range(1, W):
        s = slice_py(L, W, q)
        if 0 < s < L and run_id[s] == run_id[s - 1]:
            members = rank_of[run_id == run_id[s]]
            if len(set(members.tolist())) > 1:
                cut_in_ties.append(q)
    own = [int(dts["dts_off"][bnd[q + 1]] - dts["dts_off"][bnd[q]]) for q in range(W)]
    tiles = lambda n: -(-n // MT_TILE)  # noqa: E731
    cand = {"catchwords": [int(case["offs"][bnd[q + 1]] - case["offs"][bnd[q]]) for q in range(W)], "topic_sums_by_doc": own,
            "top_two": [int(bnd[q + 1] - bnd[q]) for q in range(W)]}
    avgs = [shard_avg(case, int(bnd[q]), int(bnd[q + 1])) for q in range(W)]
    nonempty = [a for a in avgs if a[2]]
    return dict(L=L, W=W, own=own, cut_in_ties=cut_in_ties, runs=len(run_start),
                slice_len=[slice_py(L, W, q + 1) - slice_py(L, W, q) for q in range(W)],
                tiles={k: [tiles(n) for n in c] for k, c in cand.items()},
                cut_inside_tile={k: [sum(c[:q + 1]) % MT_TILE != 0 for q in range(W - 1)] for k, c in cand.items()},
                avg=shard_avg(case, 0, D)[0], shard_avgs=[a[0] for a in avgs], mean_of_shard_avgs=float(np.mean([a[0] for a in nonempty])),
                few_L=sum(e - b for b, e in [(int(dts["dts_off"][b]), int(dts["dts_off"][e])) for b, e in few_ranges(layout)]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def first_difference(got, want):
    """None where the bytes are equal, else a description of the first differing line"""
    if got == want:
        return None
    g, w = got.splitlines(True), want.splitlines(True)
    for i in range(max(len(g), len(w))):
        a, b = (g[i] if i < len(g) else None), (w[i] if i < len(w) else None)
        if a != b:
            return "line %d: got %r, expected %r (%d lines against %d)" % (i + 1, a, b, len(g), len(w))
    return "equal lines, different bytes"


def certify_reports(layout, ranks):
    """The four report kinds and the two small topic_sums calls of one layout: every rank's bytes, nbytes, nlines and sink calls.
    -> {kind: "bytes equal"}; AssertionError naming the first differing line."""
    want, W = expected_reports(layout), WORLD[layout]
    assert len(ranks) == W
    out = {}
    for kind in KINDS + ("few", "none"):
        for q, res in enumerate(ranks):
            got = res["rep_" + kind].tobytes()
            diff = first_difference(got, want[kind][q])
            assert diff is None, "%s %s rank %d: %s" % (layout, kind, q, diff)
            n = [int(x) for x in res["rep_%s_n" % kind]]  # nbytes, nlines of the call; nbytes, nlines of the size query
            assert n == [len(want[kind][q]), want[kind][q].count(b"\n")] * 2, "%s %s rank %d: nbytes, nlines %s for %d bytes in %d lines" % (
                layout, kind, q, n, len(want[kind][q]), want[kind][q].count(b"\n"))
            calls = int(res["rep_%s_calls" % kind])
            assert (calls > 0) == (len(want[kind][q]) > 0), "%s %s rank %d: %d sink calls for %d bytes" % (layout, kind, q, calls, len(want[kind][q]))
        out[kind] = "bytes equal"
    return out


def certify_avg(layout, ranks, name):
    """avg_doc_sz is the corpus value, floor(tokens / non-empty documents) over all ranks' documents, on every rank"""
    case = corpus()
    want = float(int(np.asarray(case["cnt"], np.int64).sum()) // int((np.diff(case["offs"]) > 0).sum()))
    for q, res in enumerate(ranks):
        got = float(np.asarray(res[name]).ravel()[0])
        assert got == want, "%s rank %d: %s = %r, the corpus has %r" % (layout, q, name, got, want)
    return want


def infer_rows(single, d0, d1):
    """rows [d0, d1) of a single-rank inference result (dict(tt, tw, llh, off, topic, weight)), the offsets rebased"""
    off = np.asarray(single["off"], np.int64)
    o0, o1 = int(off[d0]), int(off[d1])
    return dict(tt=single["tt"][d0:d1], tw=single["tw"][d0:d1], llh=single["llh"][d0:d1], off=off[d0:d1 + 1] - o0, topic=single["topic"][o0:o1],
                weight=single["weight"][o0:o1], nc=int((np.asarray(single["llh"][d0:d1])[:, 0] != 0).sum()), ne=o1 - o0)


def infer_texts(part, first_number):
    """The two inference texts of an inference result whose row 0 is printed as first_number"""
    n = len(part["off"]) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(part["off"]))
    entries = doc_lines_text(rows + first_number, np.asarray(part["topic"], np.int64) + 1, part["weight"])
    tt, tw = np.asarray(part["tt"]).reshape(n, 5), np.asarray(part["tw"], F).reshape(n, 5)
    keep = np.cumprod(tt >= 0, axis=1).astype(bool)  # the slots in order while top_topic >= 0
    r5 = np.repeat(np.arange(n, dtype=np.int64), 5).reshape(n, 5)
    top = doc_lines_text(r5[keep] + first_number, tt[keep].astype(np.int64) + 1, tw[keep])
    return {"entries": entries, "top": top}


def certify_infer(layout, ranks, single, prefix, inner=False):
    """One inference run of a layout (prefix: "inf" host model, "ld" loaded model, "in" the inner ranges under the loaded model, "hb" B
    from the host) against the single-rank result `single` of the whole corpus: every array bit for bit, the counts, the two texts."""
    bnd = bounds(layout)
    assert len(ranks) == len(bnd) - 1
    for q, res in enumerate(ranks):
        d0, d1 = int(bnd[q]), int(bnd[q + 1])
        if inner:
            b, e = inner_range(d1 - d0)
            d0, d1 = d0 + b, d0 + e
        want = infer_rows(single, d0, d1)
        who = "%s %s rank %d" % (layout, prefix, q)
        for f in ("tt", "off", "topic"):
            assert np.array_equal(np.asarray(res["%s_%s" % (prefix, f)]).reshape(np.asarray(want[f]).shape), want[f]), "%s: %s differs" % (who, f)
        for f in ("tw", "llh", "weight"):
            got = np.asarray(res["%s_%s" % (prefix, f)], F).reshape(np.asarray(want[f]).shape)
            assert np.array_equal(_bits(got), _bits(want[f])), "%s: %s differs in its bits" % (who, f)
        assert int(res[prefix + "_nc"]) == want["nc"] and int(res[prefix + "_ne"]) == want["ne"], "%s: nconverged, nentries" % who
        if prefix in ("inf", "in"):
            texts = infer_texts(want, d0 + 1)  # base 1: the printed number of a row is its document's number in the corpus + 1
            for kind in INFER_KINDS:
                diff = first_difference(res["%s_text_%s" % (prefix, kind)].tobytes(), texts[kind])
                assert diff is None, "%s text %s: %s" % (who, kind, diff)
                n = [int(x) for x in res["%s_text_%s_n" % (prefix, kind)]]
                assert n == [len(texts[kind]), texts[kind].count(b"\n")], "%s text %s: nbytes, nlines %s" % (who, kind, n)
    return "bits equal"


def certify_sink_refusal(layout, ranks):
    """A sink that refuses on rank 1 during topic_sums: rank 1 gets the sink's error, every other rank completes with its bytes."""
    want = expected_reports(layout)["topic_sums"]
    if WORLD[layout] < 2:
        return
    assert len(want[1]) > 0
    for q, res in enumerate(ranks):
        if q == 1:
            assert str(res["refusal"]) == "RuntimeError: the sink refuses", str(res["refusal"])
        else:
            assert str(res["refusal"]) == "" and res["refusal_bytes"].tobytes() == want[q], "%s rank %d beside a refusing rank 1: %r" % (layout, q, str(res["refusal"]))


REFUSALS = {"avg_topic_model": "avg_topic_model: single-rank only", "topic_coherence": "topic_coherence: single-rank only",
            "log_combinatorial": "log_combinatorial: single-rank only", "distinct_top_five": "distinct_top_five: single-rank only",
            "top_words_avg": "model_top_words: single-rank only", "infer_avg": "infer_resident: single-rank only"}


def certify_refusals(layout, ranks):
    for res in ranks:
        for what, text in REFUSALS.items():
            assert str(res["refused_" + what]).endswith(": " + text), "%s %s: %r" % (layout, what, str(res["refused_" + what]))


# ---------------------------------------------------------------------------------------------------------------------------------
# per-rank results from the references alone (the CPU tests), right ones and ones made by a wrong rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _renumber(text, shift):
    return b"".join(b"%d\t%s" % (int(ln.split(b"\t", 1)[0]) + shift, ln.split(b"\t", 1)[1]) for ln in text.splitlines(True))


def reference_ranks(layout, wrong=None):
    """What every rank must deliver, from the reference alone.  wrong: a rule a sharded implementation could take instead:
      "local_numbers"   documents numbered from the shard's 0
      "sort_per_shard"  topic_sums sorted per shard and the shards' files concatenated
      "tie_order"       equal (topic, value) pairs of different shards in the wrong order (the later rank's first)
      "slice_drop" / "slice_repeat"   a slice rule that gives every rank floor(L / W) lines (the last L mod W lines are dropped) / ceil(L / W)
                        lines beginning at q floor(L / W) (lines repeat)
      "shard_avg"       avg_doc_sz taken over the rank's own documents"""
    case, R, bnd, W = corpus(), reference(), bounds(layout), WORLD[layout]
    dts = R["dts"]
    want = {k: list(v) for k, v in expected_reports(layout).items()}
    if wrong == "local_numbers":
        for kind in ("catchwords", "topic_sums_by_doc", "top_two"):
            want[kind] = [_renumber(t, -int(bnd[q])) for q, t in enumerate(want[kind])]
    lines = topic_sums_lines(dts, [(0, D)])
    if wrong == "sort_per_shard":
        want["topic_sums"] = [b"".join(topic_sums_lines(dts, [(int(bnd[q]), int(bnd[q + 1]))])) for q in range(W)]
    if wrong == "tie_order":
        doc, t, v = sums_of(dts, [(0, D)])
        o = np.lexsort((-sc.rank_of_doc(bnd, doc), -v.view(np.uint32).astype(np.int64), t))
        want["topic_sums"] = cut_lines(doc_lines_text(doc[o] + 1, t[o] + 1, v[o]).splitlines(True), W)
    if wrong == "slice_drop":
        want["topic_sums"] = [b"".join(lines[q * (len(lines) // W):(q + 1) * (len(lines) // W)]) for q in range(W)]
    if wrong == "slice_repeat":
        want["topic_sums"] = [b"".join(lines[q * (len(lines) // W):q * (len(lines) // W) + -(-len(lines) // W)]) for q in range(W)]
    avg = float(shard_avg(case, 0, D)[0])
    ranks = []
    for q in range(W):
        res = {}
        for kind in KINDS + ("few", "none"):
            res["rep_" + kind] = _u8(want[kind][q])
            res["rep_%s_n" % kind] = np.array([len(want[kind][q]), want[kind][q].count(b"\n")] * 2, np.int64)
            res["rep_%s_calls" % kind] = np.array(1 if want[kind][q] else 0)
        res["avg_th"] = np.array([float(shard_avg(case, int(bnd[q]), int(bnd[q + 1]))[0]) if wrong == "shard_avg" else avg], F)
        ranks.append(res)
    return ranks


def fake_single(seed=5):
    """An inference result of the corpus's shape made without a device (the CPU tests of certify_infer): random entries, empty documents
    without any"""
    rng = np.random.default_rng(seed)
    case = corpus()
    nonempty = np.diff(case["offs"]) > 0
    cnt = np.where(nonempty, rng.integers(0, 4, D), 0)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    topic = np.concatenate([np.sort(rng.choice(TOPICS, size=c, replace=False)) for c in cnt] + [np.zeros(0, np.int64)]).astype(np.uint32)
    weight = (rng.random(int(off[-1])) * 0.8 + 0.15).astype(F)
    tt, tw = np.full((D, 5), -1, np.int32), np.zeros((D, 5), F)
    for d in np.flatnonzero(cnt):
        s = slice(off[d], off[d + 1])
        o = np.argsort(-weight[s], kind="stable")
        tt[d, :len(o)], tw[d, :len(o)] = topic[s][o], weight[s][o]
    llh = np.where(nonempty[:, None], -rng.random((D, 2)) - 0.5, 0).astype(F)
    return dict(tt=tt, tw=tw, llh=llh, off=off, topic=topic, weight=weight)


def infer_ranks(layout, single, prefix, inner=False, local_numbers=False):
    """The per-rank results of one inference run cut from a single-rank result; local_numbers: the texts number rows from the shard's 0"""
    bnd = bounds(layout)
    ranks = []
    for q in range(len(bnd) - 1):
        d0, d1 = int(bnd[q]), int(bnd[q + 1])
        if inner:
            b, e = inner_range(d1 - d0)
            d0, d1 = d0 + b, d0 + e
        part = infer_rows(single, d0, d1)
        res = {"%s_%s" % (prefix, f): np.asarray(part[f]) for f in ("tt", "tw", "llh", "off", "topic", "weight")}
        res[prefix + "_nc"], res[prefix + "_ne"] = np.array(part["nc"]), np.array(part["ne"])
        for kind, text in infer_texts(part, 1 if local_numbers else d0 + 1).items():
            res["%s_text_%s" % (prefix, kind)] = _u8(text)
            res["%s_text_%s_n" % (prefix, kind)] = np.array([len(text), text.count(b"\n")], np.int64)
        ranks.append(res)
    return ranks


# ---------------------------------------------------------------------------------------------------------------------------------
# the worker: one process per rank
# ---------------------------------------------------------------------------------------------------------------------------------
def worker_main(rank, port, out, layout):
    rank_launch.run_rank(WORLD[layout], int(rank), int(port), out, lambda hp, rank, world, res: _worker(hp, layout, rank, world, res))


def _report(hp, res, name, what, docs):
    parts = []
    nb, nl = hp._doc_report_call(what, docs, lambda mv: parts.append(bytes(mv)))
    sb, sl = hp.doc_report_size(what, docs)
    res["rep_" + name], res["rep_%s_n" % name], res["rep_%s_calls" % name] = _u8(b"".join(parts)), np.array([nb, nl, sb, sl], np.int64), np.array(len(parts))


def _infer(hp, res, prefix, model, docs=None, chunk_docs=0, texts=False, base=1):
    r = hp.infer_resident(model=model, docs=docs, chunk_docs=chunk_docs)
    for f, k in (("tt", "top_topic"), ("tw", "top_weight"), ("llh", "llh"), ("off", "offs"), ("topic", "topic"), ("weight", "weight")):
        res["%s_%s" % (prefix, f)] = r[k]
    res[prefix + "_nc"], res[prefix + "_ne"], res[prefix + "_avg"] = np.array(r["nconverged"]), np.array(r["nentries"]), np.array([r["avg_doc_sz"]], F)
    if texts:
        for kind in INFER_KINDS:
            res["%s_text_%s" % (prefix, kind)] = _u8(hp.infer_text(kind, base=base))
            res["%s_text_%s_n" % (prefix, kind)] = np.array(hp.infer_text_size(kind, base=base), np.int64)


def _refused(res, name, call):
    try:
        call()
        res["refused_" + name] = np.array("")
    except Exception as e:
        res["refused_" + name] = np.array(str(e))


def _worker(hp, layout, rank, world, res):
    case, bnd = corpus(), bounds(layout)
    A = dict(vals=np.asarray(case["cnt"], np.float32), rows=case["rows"], offs=np.asarray(case["offs"], np.int64))
    cnt, rows, offs, d0 = sc.shard(A, bnd, rank)
    Dq, k = len(offs) - 1, case["topics"]
    hp.upload_counts(V, cnt, rows, offs, doc_offset=d0, docs_global=D)
    assert hp.a_doc_offset == d0
    hp.threshold(case["k"])
    res["avg_th"] = np.array([hp.avg_doc_sz()], F)  # a_avg is the thresholding's: no collective
    assign = np.asarray(case["assign"], np.uint32)[hp.doc_offset:hp.doc_offset + hp.D]
    hp.find_catchwords(k, case["r"], assign=assign, rho=RHO, fetch_thresholds=False)
    hp.construct_topic_model(k, case["rank"], Dq, fetch_sums=False)
    for kind in KINDS:
        _report(hp, res, kind, kind, None)
    _report(hp, res, "few", "topic_sums", few_local(layout, rank))
    _report(hp, res, "none", "topic_sums", none_local(layout, rank))
    # a sink that refuses on rank 1: the collectives of the call are behind every rank by then
    def consume(mv):
        if rank == 1:
            raise RuntimeError("the sink refuses")
        kept.append(bytes(mv))
    kept = []
    try:
        hp._doc_report_call("topic_sums", None, consume)
        res["refusal"] = np.array("")
    except Exception as e:
        res["refusal"] = np.array("%s: %s" % (type(e).__name__, e))
    res["refusal_bytes"] = _u8(b"".join(kept))
    # inference under the host model, under the same model loaded from its text, and on an inner range in chunks
    M = infer_model()
    _infer(hp, res, "inf", M, texts=True, base=1 + hp.a_doc_offset)
    hp.load_model_text(hp.model_text(M, "sparse"), V, k, "sparse")
    _infer(hp, res, "ld", "loaded")
    b, e = inner_range(Dq)
    _infer(hp, res, "in", "loaded", docs=(b, e), chunk_docs=INNER_CHUNK, texts=True, base=1 + hp.a_doc_offset + b)
    if world > 1:  # what this stage does not build stays refused, with its message
        _refused(res, "avg_topic_model", lambda: hp.avg_topic_model(k))
        _refused(res, "topic_coherence", lambda: hp.topic_coherence(np.arange(2 * k, dtype=np.uint32).reshape(k, 2)))
        _refused(res, "log_combinatorial", hp.log_combinatorial)
        _refused(res, "distinct_top_five", hp.distinct_top_five_sets)
        _refused(res, "top_words_avg", lambda: hp.model_top_words(3, model="avg"))
        _refused(res, "infer_avg", lambda: hp.infer_resident(model="avg"))
    # B from the host beside a new A: the corpus totals behind avg_doc_sz are summed over the ranks inside the inference call
    hp.upload_csc(V, cnt, rows, offs, doc_offset=d0, docs_global=D)
    hp.upload_counts(V, cnt, rows, offs, doc_offset=d0, docs_global=D)
    _infer(hp, res, "hb", M)
    if layout == DOMAIN_LAYOUT:
        _worker_domain(hp, rank, res)


# ---- the writers' domain applies to the number in the corpus: a two-document shard whose second document prints 0x7fffffff --------------
DOMAIN_LAYOUT, DOMAIN_OFFSET = "H2", 0x7ffffffd


def domain_case():
    """Two ranks of two one-word documents each ({word 0: 5}, {word 1: 5}; clusters 0, 1; two topics, r = 1: both words are catchwords,
    every normalised value is avg = 5).  Rank 1 uploads its shard with doc_offset = 0x7ffffffd: its document 0 prints 0x7ffffffe, the
    last number the writers take, its document 1 would print 0x7fffffff.  B and A come from the host, the partition is passed."""
    return dict(V=4, cnt=np.full(2, 5, F), rows=np.array([0, 1], np.uint32), offs=np.array([0, 1, 2], np.int64), assign=np.array([0, 1], np.uint32), topics=2, r=1)


def _worker_domain(hp, rank, res):
    c = domain_case()
    d0 = DOMAIN_OFFSET if rank == 1 else 0
    hp.upload_csc(c["V"], c["cnt"], c["rows"], c["offs"], doc_offset=d0, docs_global=DOMAIN_OFFSET + 2)
    hp.upload_counts(c["V"], c["cnt"], c["rows"], c["offs"], doc_offset=d0, docs_global=DOMAIN_OFFSET + 2)
    hp.find_catchwords(c["topics"], c["r"], assign=c["assign"], rho=RHO, fetch_thresholds=False)  # collective
    res["dom_first"] = _u8(hp.doc_report_text("catchwords", docs=(0, 1)))
    try:
        res["dom_all"], res["dom_refused"] = _u8(hp.doc_report_text("catchwords")), np.array("")
    except Exception as e:
        res["dom_all"], res["dom_refused"] = _u8(b""), np.array(str(e))


def certify_domain(ranks):
    """rank 0 prints its two documents as 1 and 2; rank 1 prints document 0 as 2147483646 and is refused for document 1, by both names"""
    five = np.full(2, 5, F)
    assert ranks[0]["dom_all"].tobytes() == doc_lines_text([1, 2], [1, 2], five) and str(ranks[0]["dom_refused"]) == ""
    assert ranks[0]["dom_first"].tobytes() == doc_lines_text([1], [1], five[:1])
    assert ranks[1]["dom_first"].tobytes() == doc_lines_text([DOMAIN_OFFSET + 1], [1], five[:1]) == b"2147483646\t1\t5.000000\n"
    msg = str(ranks[1]["dom_refused"])
    assert "doc_report_text(catchwords): the line of document 1 (document %d of the corpus), word 1 (0-based)" % (DOMAIN_OFFSET + 1) in msg, msg
    assert "outside the writers' domain" in msg and ranks[1]["dom_all"].size == 0


def launch(layout, tmp, timeout=rank_launch.LAUNCH_TIMEOUT_S):
    """rank_launch.launch of the layout's ranks"""
    return rank_launch.launch("docs %s" % layout, "docs_%s" % layout, WORLD[layout], tmp, rank_launch.module_command("doc_shard_cases", layout), timeout=timeout)
