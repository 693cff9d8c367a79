"""Catchwords, the topic model and the edge pairs on column-sharded documents (N > 1 ranks), held against the plain reference of the
single-rank stage: layouts, the per-rank worker and the certificate (no GPU needed to import this module; the worker alone opens the
device; tests/rank_launch.py starts the ranks).

The cases are the downstream cases of stages_certificate (p_arms_case, p_select_case, p_dts_case(k) for k in DTS_K) and their reference
is post_reference(case): what one rank computes on the whole corpus.  Layouts give the document bounds (rank r holds the documents
[bounds[r], bounds[r + 1]) of A, D of any parity):

  H    2 ranks  [0, ceil(D / 2), D]
  E3   3 ranks  [0, 1, D, D]                a one-document shard and an empty last shard
  E4   4 ranks  [0, 0, D // 3, D // 3, D]   an empty first and an empty middle shard
  S<n> 4 ranks  p_select_case only: the three segments of n values (n = 255, 256, 257, 1000; kinds equal, run, top16) each cut in the
                middle, so that every one of them lies on two ranks.  Three cuts are what four ranks of contiguous documents give: the
                twelve segments take the four layouts S255, S256, S257, S1000, and every segment is cut in one of them.
  W1   1 rank   a communicator of one rank: the launches of a context without one
  C2   2 ranks  chunk_case only (below): more segments than one all-reduce of bins takes, every one of them cut 1 + 1

select_layout_facts states, from the reference alone, what makes the S layouts test the histogram select and not the one-workgroup
one: both parts of every cut segment hold values, a rank r whose r-th largest value lies on the first part and one whose value lies on
the second, and values that share their top 16 bits on both parts (passes three and four see bins only the sum resolves).

The worker runs as one fresh process per rank on one GPU over the host-staged transport and writes every array it fetched to an .npz
per rank.  certify_post takes those per-rank arrays; tests/test_post_shard_cases_cpu.py feeds it arrays made from the references alone
(reference_ranks), right ones and ones made by a wrong rule, so no statement rests on what the device returns.

The model's bound is certify_model's, unchanged: (m + max m + V + C) u' |ref| holds for any tree of the m additions of an entry, and
partial sums per rank followed by N - 1 additions of partials is such a tree (a rank that contributes nothing adds an exact zero): no
margin for N."""
import numpy as np

import rank_launch
import shard_cases as sc
import stages_certificate as stc

F = np.float32
RHO = 1.1
TOP_WORDS = 5
EDGE_MAX, EDGE_MIN_DOCS = 10, 1

SELECT_CUT_LENGTHS = (255, 256, 257, 1000)
GENERAL_LAYOUTS = ("H", "E3", "E4")
SELECT_LAYOUTS = tuple("S%d" % n for n in SELECT_CUT_LENGTHS)
WORLD = dict({"H": 2, "E3": 3, "E4": 4, "W1": 1, "C2": 2}, **{l: 4 for l in SELECT_LAYOUTS})
CASE_NAMES = ("arms", "select") + tuple("dts%d" % k for k in stc.DTS_K)


def case_of(name):
    if name == "arms":
        return stc.p_arms_case()
    if name == "select":
        return stc.p_select_case()
    return stc.p_dts_case(int(name[3:]))


def cases_of(layout):
    if layout == "C2":
        return ("chunk",)
    return ("select",) if layout in SELECT_LAYOUTS else CASE_NAMES


# ---- more slots than a chunk: the second chunk of the bins' all-reduce (the first slot of a chunk is not slot 0) ----------------------------
CHUNK_SLOTS = 65536  # stage_host.h SELECT_CHUNK_SLOTS: 64 MiB of bins per all-reduce (stated here, checked by test_post_select_rule_cpu.py)
CHUNK_V, CHUNK_W, CHUNK_SKIP = 33000, 500, 110
_CHUNK = {}


def chunk_case():
    """Two topics, r = 1, V = 33 000 words: 66 000 (word, topic) pairs.  Every word stands in two documents of either topic (documents of 500
    consecutive words, counts 1 .. 49), but for the words w with w % 110 == 7, which topic 1 holds once: 65 700 pairs have more than r
    values, 300 have S > r >= n (threshold 0).  The documents come in two repetitions, one on either rank of [0, D / 2, D]: every segment has
    one value on each rank, and its largest is on rank 0 for some pairs and on rank 1 for others.  B is uploaded beside A with A's columns
    (no thresholding ran: avg_doc_sz is formed in the catchword call, from totals summed over the ranks).  Its reference is the thresholds
    and the catch topics alone (V exceeds the size condition of certify_model).  -> dict(V, cnt, rows, offs, nv, cl, assign, topics, r, thr,
    catch_topic, nslots)."""
    if not _CHUNK:
        rng = np.random.default_rng(77)
        rows, cnt, lens, want = [], [], [], []
        for rep in (0, 1):
            for t in (0, 1):
                for b in range(CHUNK_V // CHUNK_W):
                    w = np.arange(b * CHUNK_W, (b + 1) * CHUNK_W)
                    if rep == 1 and t == 1:
                        w = w[w % CHUNK_SKIP != 7]
                    rows.append(w.astype(np.uint32))
                    cnt.append(rng.integers(1, 50, len(w)).astype(F))
                    lens.append(len(w))
                    want.append(t)
        rows, cnt = np.concatenate(rows), np.concatenate(cnt)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        avg = stc.corpus_avg(cnt, offs)[0]
        nv = stc.ref_normalize(cnt, offs, avg)
        cl = np.asarray(want, np.int32)
        thr, arms = stc.ref_catch_thresholds(CHUNK_V, rows, offs, nv, cl, 2, 1)
        _CHUNK.update(V=CHUNK_V, cnt=cnt, rows=rows, offs=offs, nv=nv, cl=cl, assign=cl.astype(np.uint32), topics=2, r=1, thr=thr, arms=arms,
                      catch_topic=stc.ref_find_catchwords(thr, RHO), nslots=int(arms["n == r + 1"] + arms["n > r + 1"]))
    return _CHUNK


def certify_chunk(case, ranks):
    thr = sc.same_on_all_ranks(ranks, key("chunk", 1, "thr"))
    bad = np.argwhere(_bits(thr) != _bits(case["thr"]))
    assert bad.size == 0, "chunk: %d thresholds differ, first (word %d, topic %d): %r vs %r" % (
        len(bad), bad[0][0], bad[0][1], thr[tuple(bad[0])], case["thr"][tuple(bad[0])])
    ct = sc.same_on_all_ranks(ranks, key("chunk", 1, "ct"))
    assert np.array_equal(ct, case["catch_topic"])
    assert int(sc.same_on_all_ranks(ranks, key("chunk", 1, "nc")).ravel()[0]) == int((case["catch_topic"] >= 0).sum())


def runs_of(name):
    """(r, rank) of every run of a case: p_select_case takes r = rank over select_ranks() (r == n - 1, n, n + 1 at every length)."""
    if name == "select":
        return [(r, r) for r in stc.select_ranks()]
    case = case_of(name)
    return [(case["r"], case.get("rank", 1))]


def num_docs(case):
    return len(case["offs"]) - 1


def segment_starts(case):
    """first document of every segment of p_select_case, in the order of case["segs"]"""
    return np.concatenate([[0], np.cumsum([s["n"] for s in case["segs"]])])[:-1]


def bounds(layout, case):
    D = num_docs(case)
    if layout == "H":
        return np.array([0, (D + 1) // 2, D], np.int64)
    if layout == "E3":
        return np.array([0, 1, D, D], np.int64)
    if layout == "E4":
        return np.array([0, 0, D // 3, D // 3, D], np.int64)
    if layout == "W1":
        return np.array([0, D], np.int64)
    assert layout in SELECT_LAYOUTS and "segs" in case
    n = int(layout[1:])
    starts = segment_starts(case)
    cuts = [int(starts[i]) + n // 2 for i, s in enumerate(case["segs"]) if s["n"] == n]  # n // 2: inside the middle run of kind "run"
    assert len(cuts) == 3 and cuts == sorted(cuts)
    return np.array([0] + cuts + [D], np.int64)


def segment_values(case, seg):
    """(values float32, documents) of a segment of p_select_case: the normalised counts of its word over the documents of its cluster"""
    doc_of = np.repeat(np.arange(num_docs(case)), np.diff(case["offs"]))
    at = np.flatnonzero((np.asarray(case["rows"], np.int64) == seg["word"]) & (case["cl"][doc_of] == seg["topic"]))
    return np.asarray(case["nv"], F)[at], doc_of[at]


def select_layout_facts(case, bnd):
    """Per segment of p_select_case that the bounds cut: dict(seg, parts (values per rank, non-empty ones), first (ranks r of select_ranks()
    whose r-th largest value lies on the first part only), second (... on the second part only), shared16 (the values on each part that
    carry the segment's most frequent top 16 bits), per_part_differs (ranks r at which selecting within one part alone gives another value
    than selecting from the whole))."""
    out = []
    for seg in case["segs"]:
        v, d = segment_values(case, seg)
        rk = sc.rank_of_doc(bnd, d)
        parts = [v[rk == q] for q in np.unique(rk)]
        if len(parts) < 2:
            continue
        n = len(v)
        desc = np.sort(v)[::-1]
        first, second, differs = [], [], []
        for r in stc.select_ranks():
            if r > n:
                continue
            x = desc[r - 1]
            on = [bool((p == x).any()) for p in parts]
            if on == [True, False]:
                first.append(r)
            if on == [False, True]:
                second.append(r)
            alone = [np.sort(p)[::-1][r - 1] if r <= len(p) else None for p in parts]
            if all(a is None or a != x for a in alone):
                differs.append(r)
        top = v.view(np.uint32) >> 16
        vals, cnt = np.unique(top, return_counts=True)
        common = vals[np.argmax(cnt)]
        out.append(dict(seg=seg, parts=[len(p) for p in parts], first=first, second=second,
                        shared16=[int(((p.view(np.uint32) >> 16) == common).sum()) for p in parts], per_part_differs=differs))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
def key(name, r, what):
    return "%s_r%d_%s" % (name, r, what)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def concat_docs(ranks, kk, bnd):
    """The per-document outputs of the ranks side by side: top1 / top2 and the (document, topic) sums with the offsets rebased.  Every
    rank's arrays have the lengths of its own shard and offsets that begin at 0."""
    t1, t2, off, topic, val, base = [], [], [], [], [], 0
    for q, res in enumerate(ranks):
        Dq = int(bnd[q + 1] - bnd[q])
        o = np.asarray(res[kk("dts_off")], np.int64)
        assert len(o) == Dq + 1 and o[0] == 0, "rank %d: %d offsets beginning at %d for %d documents" % (q, len(o), o[0] if len(o) else -1, Dq)
        assert len(res[kk("top1")]) == Dq and len(res[kk("top2")]) == Dq
        n = int(np.asarray(res[kk("nsums")]).ravel()[0])
        assert n == o[-1] == len(res[kk("dts_topic")]) == len(res[kk("dts_val")]), "rank %d: num_sums %d, last offset %d" % (q, n, o[-1])
        t1.append(res[kk("top1")])
        t2.append(res[kk("top2")])
        off.append(o[:-1] + base)
        topic.append(res[kk("dts_topic")])
        val.append(res[kk("dts_val")])
        base += n
    return dict(top1=np.concatenate(t1), top2=np.concatenate(t2), dts_off=np.concatenate(off + [[base]]).astype(np.int64),
                dts_topic=np.concatenate(topic), dts_val=np.concatenate(val).astype(np.float32), nsums=base)


def certify_post(case, name, r, rank, bnd, ranks):
    """One run (r, rank) of one case on one layout.  -> dict(model_ratio)."""
    R = stc.post_reference(case, r=r, rho=RHO, rank=rank)
    V, k = case["V"], case["topics"]
    kk = lambda what: key(name, r, what)  # noqa: E731
    assert len(ranks) == len(bnd) - 1
    # replicated, bit for bit the reference's
    thr = sc.same_on_all_ranks(ranks, kk("thr"))
    assert thr.shape == R["thr"].shape
    bad = np.argwhere(_bits(thr) != _bits(R["thr"]))
    assert bad.size == 0, "%s r=%d: %d thresholds differ, first (word %d, topic %d): %r vs %r" % (
        name, r, len(bad), bad[0][0], bad[0][1], thr[tuple(bad[0])], R["thr"][tuple(bad[0])])
    ct = sc.same_on_all_ranks(ranks, kk("ct"))
    assert np.array_equal(ct, R["catch_topic"]), "%s r=%d: catch topics differ at words %s" % (name, r, np.flatnonzero(ct != R["catch_topic"])[:10])
    assert int(sc.same_on_all_ranks(ranks, kk("nc")).ravel()[0]) == int((R["catch_topic"] >= 0).sum())
    mthr = sc.same_on_all_ranks(ranks, kk("mthr"))
    assert np.array_equal(_bits(mthr), _bits(R["mthr"])), "%s r=%d: rank thresholds %s vs %s" % (name, r, mthr, R["mthr"])
    # the shards' own, side by side
    got, dts = concat_docs(ranks, kk, bnd), R["dts"]
    assert got["nsums"] == len(dts["dts_val"]), "%s r=%d: %d sums over the ranks, %d in the reference" % (name, r, got["nsums"], len(dts["dts_val"]))
    assert np.array_equal(got["dts_off"], dts["dts_off"]) and np.array_equal(got["dts_topic"], dts["dts_topic"]), "%s r=%d: document-topic sums misplaced" % (name, r)
    bad = np.flatnonzero(_bits(got["dts_val"]) != _bits(dts["dts_val"]))
    assert bad.size == 0, "%s r=%d: %d document-topic sums differ in their bits" % (name, r, bad.size)
    assert np.array_equal(got["top1"], dts["top1"]) and np.array_equal(got["top2"], dts["top2"]), "%s r=%d: top topics differ" % (name, r)
    # the model: replicated, the reference's NaN pattern, within the single-rank bound
    model = sc.same_on_all_ranks(ranks, kk("model"))
    res = stc.certify_model(model, R["model64"], R["m"], V)
    # edge pairs: replicated, the selection over all documents
    pairs = sc.same_on_all_ranks(ranks, kk("pairs"))
    from isle_amd import hot_path
    want = hot_path.select_edge_pairs(dts["top1"], dts["top2"], EDGE_MAX, EDGE_MIN_DOCS)
    assert pairs.shape == want.shape and np.array_equal(pairs, want), "%s r=%d: edge pairs\n%s\nexpected\n%s" % (name, r, pairs, want)
    sc.same_on_all_ranks(ranks, kk("pinfo"))
    ep = stc.edge_pairs(k, case.get("empty_topic"))
    stc.certify_edge(sc.same_on_all_ranks(ranks, kk("edge")), model, ep)
    sc.same_on_all_ranks(ranks, kk("tw"))
    return dict(model_ratio=res["max_ratio"])


# ---------------------------------------------------------------------------------------------------------------------------------
# per-rank arrays from the references alone (the CPU tests), right ones and ones made by a wrong rule
# ---------------------------------------------------------------------------------------------------------------------------------
def model32_from_shards(case, R, bnd, leave_out=None):
    """The model as N ranks form it, in float32: every shard's contributions summed (in document order), the partial sums added rank after
    rank, the columns normalised.  leave_out: a rank whose partial sums are left out (a wrong rule)."""
    V, k = case["V"], case["topics"]
    rows, offs, nv = np.asarray(case["rows"], np.int64), case["offs"], np.asarray(case["nv"], F)
    parts = [np.zeros((V, k), F, order="F") for _ in range(len(bnd) - 1)]
    for t, d in R["contribs"]:
        q = int(sc.rank_of_doc(bnd, d))
        s = slice(offs[d], offs[d + 1])
        parts[q][rows[s], t] = parts[q][rows[s], t] + nv[s]
    M = np.zeros((V, k), F, order="F")
    for q, P in enumerate(parts):
        if q != leave_out:
            M = (M + P).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(k):
            tot = F(0)
            for w in range(V):
                tot = F(tot + abs(M[w, t]))
            M[:, t] = M[:, t] * F(1.0 / np.float64(tot))
    return np.asfortranarray(M)


def reference_ranks(case, name, r, rank, bnd, thr=None, rebase=True, leave_out=None):
    """What every rank must hold, from post_reference alone: the replicated results as they are, the per-document results cut at the
    bounds.  thr: thresholds to hand out instead (a wrong rule); rebase=False: a shard's offsets keep the corpus's numbering (a wrong rule);
    leave_out: model32_from_shards."""
    R = stc.post_reference(case, r=r, rho=RHO, rank=rank)
    from isle_amd import hot_path
    dts, k = R["dts"], case["topics"]
    model = model32_from_shards(case, R, bnd, leave_out)
    ep = stc.edge_pairs(k, case.get("empty_topic"))
    a, b = stc.edge_coefficients(0.7)
    with np.errstate(invalid="ignore"):
        edge = np.asfortranarray(np.stack([(a * model[:, p] + b * model[:, q]).astype(F) for p, q in ep], axis=1))
    shared = {"thr": R["thr"] if thr is None else thr, "ct": R["catch_topic"], "nc": np.array([int((R["catch_topic"] >= 0).sum())]), "mthr": R["mthr"],
              "model": model, "pairs": hot_path.select_edge_pairs(dts["top1"], dts["top2"], EDGE_MAX, EDGE_MIN_DOCS), "pinfo": np.zeros(2, np.int64),
              "edge": edge, "tw": hot_path.top_words(model, TOP_WORDS)}
    ranks = []
    for q in range(len(bnd) - 1):
        d0, d1 = int(bnd[q]), int(bnd[q + 1])
        o0, o1 = int(dts["dts_off"][d0]), int(dts["dts_off"][d1])
        own = {"top1": dts["top1"][d0:d1], "top2": dts["top2"][d0:d1], "dts_off": dts["dts_off"][d0:d1 + 1] - (o0 if rebase else 0),
               "dts_topic": dts["dts_topic"][o0:o1], "dts_val": dts["dts_val"][o0:o1], "nsums": np.array([o1 - o0])}
        ranks.append({key(name, r, w): np.asarray(v) for w, v in list(shared.items()) + list(own.items())})
    return ranks


# ---------------------------------------------------------------------------------------------------------------------------------
# the worker: one process per rank
# ---------------------------------------------------------------------------------------------------------------------------------
def worker_main(rank, port, out, layout):
    def body(hp, rank, world, res):
        for name in cases_of(layout):
            if name == "chunk":
                _worker_chunk(hp, rank, res)
            else:
                _worker_case(hp, name, bounds(layout, case_of(name)), rank, res)
        if world > 1:  # what this stage does not build stays refused, with its message
            try:
                hp.avg_topic_model(2)
                res["avg_refused"] = np.array("")
            except Exception as e:
                res["avg_refused"] = np.array(str(e))
    rank_launch.run_rank(WORLD[layout], int(rank), int(port), out, body)


def _worker_chunk(hp, rank, res):
    case = chunk_case()
    D = num_docs(case)
    A = dict(vals=case["cnt"], rows=case["rows"], offs=case["offs"])
    cnt, rows, offs, d0 = sc.shard(A, np.array([0, D // 2, D], np.int64), rank)
    hp.upload_csc(case["V"], cnt, rows, offs, doc_offset=d0, docs_global=D)  # B with A's columns, from the host
    hp.upload_counts(case["V"], cnt, rows, offs, doc_offset=d0, docs_global=D)
    fc = hp.find_catchwords(case["topics"], case["r"], assign=case["assign"][d0:d0 + len(offs) - 1], rho=RHO)
    res[key("chunk", 1, "thr")], res[key("chunk", 1, "ct")], res[key("chunk", 1, "nc")] = fc["thresholds"], fc["catch_topic"], np.array([fc["num_catchwords"]])


def _worker_case(hp, name, bnd, rank, res):
    case = case_of(name)
    A = dict(vals=np.asarray(case["cnt"], np.float32), rows=case["rows"], offs=np.asarray(case["offs"], np.int64))
    cnt, rows, offs, d0 = sc.shard(A, bnd, rank)
    D_own, k = len(offs) - 1, case["topics"]
    hp.upload_counts(case["V"], cnt, rows, offs, doc_offset=d0, docs_global=num_docs(case))
    hp.threshold(case["k"])
    assign = np.asarray(case["assign"], np.uint32)[hp.doc_offset:hp.doc_offset + hp.D]  # of the columns of B this rank kept
    for r, rk in runs_of(name):
        fc = hp.find_catchwords(k, r, assign=assign, rho=RHO)
        tm = hp.construct_topic_model(k, rk, D_own)
        pairs, info = hp.select_edge_pairs(EDGE_MAX, EDGE_MIN_DOCS)
        got = {"thr": fc["thresholds"], "ct": fc["catch_topic"], "nc": np.array([fc["num_catchwords"]]), "model": tm["model"], "mthr": tm["model_threshold"],
               "top1": tm["top1"], "top2": tm["top2"], "nsums": np.array([tm["num_sums"]]), "dts_off": tm["dts_off"], "dts_topic": tm["dts_topic"],
               "dts_val": tm["dts_val"], "pairs": pairs, "pinfo": np.array([info["candidates"], -1 if info["threshold"] is None else info["threshold"]], np.int64),
               "edge": hp.edge_topics(stc.edge_pairs(k, case.get("empty_topic"))), "tw": hp.model_top_words(TOP_WORDS)}
        for what, v in got.items():
            res[key(name, r, what)] = v


def launch(layout, tmp, timeout=rank_launch.LAUNCH_TIMEOUT_S):
    """rank_launch.launch of the layout's ranks"""
    return rank_launch.launch("post %s" % layout, "post_%s" % layout, WORLD[layout], tmp, rank_launch.module_command("post_shard_cases", layout), timeout=timeout)
