"""The rule of isle_hip_similar_docs in numpy, a cutter of rows into rank shares, and the case table (a plain module, importable without
torch and without a GPU).  A row is a document's (topic, weight) entries, topics ascending strictly, its document doc_base + row; a query is
the same kind of list.  Row r is a candidate of query q when a topic is STORED in both (whatever the weights) and doc != exclude[q]; the score
is DOT, COSINE or BHATTACHARYYA as include/isle_hip.h states them; per query the candidates go by (ord(score bits) descending, document
ascending) and the first n are the result.  Nothing here reads isle_amd/csrc/simdocs_host.h: the table is what
tests/test_simdocs_rule_cpu.py holds the header's host statement to, and what the GPU tests hold the kernels to, bit for bit.

The arithmetic: np.float32 / np.float64 operations in the order stated, one IEEE operation each, so numpy's bits are the rule's.  rule()
walks the topics in ascending order and updates every (row, query) pair that stores the topic by ONE elementwise operation per topic: each
pair's sum is accumulated sequentially, common topics ascending, and no reduction is vectorised.  rule_scalar() is the same with scalars, pair by pair,
for the small cases.  Weights stay >= 2^-60 or are exactly 0, so that no fp32 product is subnormal: what subnormal products do is not
certified."""
import numpy as np

from topdocs_rule import f2b, ord_bits

DOT, COSINE, BHATTACHARYYA = 0, 1, 2
MEASURES = {"dot": DOT, "cosine": COSINE, "bhattacharyya": BHATTACHARYYA}
MAX_QUERIES = 64
NO_DOC = 0xFFFFFFFF
U32, F32, F64 = np.uint32, np.float32, np.float64


def qp_of(Q):
    p = 1
    while p < Q:
        p *= 2
    return p


def csr(lists):
    """lists: per row (or query) a list of (topic, weight), topics ascending -> off int64, topic uint32, weight float32"""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in lists])
    flat = [x for r in lists for x in r]
    return off, np.array([x[0] for x in flat], U32), np.array([x[1] for x in flat], F32)


class Case:
    """name, num_topics, n, doc_base; rows (off, topic, weight); queries (q_off, q_topic, q_weight) or query_rows (then the queries are those
    rows and exclude defaults to their documents); exclude uint32 (Q,) or None; aim: what the case aims at; exact: every partial sum of DOT is
    exactly representable (tests/test_simdocs_rule_cpu.py holds DOT to fractions there); forms: the table forms the GPU test runs it under"""

    def __init__(self, name, num_topics, n, doc_base, rows, queries=None, query_rows=None, exclude=None, aim="", exact=False, forms=("lds", "global")):
        self.name, self.num_topics, self.n, self.doc_base, self.aim, self.exact, self.forms = name, int(num_topics), int(n), int(doc_base), aim, exact, forms
        self.off, self.topic, self.weight = (np.ascontiguousarray(rows[0], np.int64), np.ascontiguousarray(rows[1], U32), np.ascontiguousarray(rows[2], F32))
        self.query_rows = None if query_rows is None else np.ascontiguousarray(query_rows, np.uint64)
        self.given_exclude = None if exclude is None else np.ascontiguousarray(exclude, U32)
        if query_rows is not None:
            lists = [list(zip(self.topic[self.off[r]:self.off[r + 1]].tolist(), self.weight[self.off[r]:self.off[r + 1]].tolist())) for r in query_rows]
            queries = csr(lists)
        self.q_off, self.q_topic, self.q_weight = (np.ascontiguousarray(queries[0], np.int64), np.ascontiguousarray(queries[1], U32),
                                                   np.ascontiguousarray(queries[2], F32))
        assert self.off[0] == 0 and self.off[-1] == self.topic.size == self.weight.size and self.q_off[-1] == self.q_topic.size
        assert 1 <= self.Q <= MAX_QUERIES

    @property
    def rows(self):
        return self.off.size - 1

    @property
    def Q(self):
        return self.q_off.size - 1

    @property
    def exclude(self):
        """the excluded documents the rule works with"""
        if self.given_exclude is not None:
            return self.given_exclude
        if self.query_rows is not None:
            return (self.doc_base + self.query_rows).astype(U32)
        return np.full(self.Q, NO_DOC, U32)

    def queries_arg(self):
        return self.query_rows if self.query_rows is not None else (self.q_off, self.q_topic, self.q_weight)

    def source_arg(self):
        return (self.off, self.topic, self.weight)


def _scores(case, measure):
    """-> hit bool (rows, Q), score float32 (rows, Q)"""
    R, Q, T = case.rows, case.Q, case.num_topics
    s = np.zeros((R, Q), F64)
    nr = np.zeros(R, F64)
    nq = np.zeros(Q, F64)
    hit = np.zeros((R, Q), bool)
    row_of = np.repeat(np.arange(R), np.diff(case.off))
    q_of = np.repeat(np.arange(Q), np.diff(case.q_off))
    order_r = np.argsort(case.topic, kind="stable")
    order_q = np.argsort(case.q_topic, kind="stable")
    rt, qt = case.topic[order_r], case.q_topic[order_q]
    rb, qb = np.searchsorted(rt, np.arange(T + 1)), np.searchsorted(qt, np.arange(T + 1))
    with np.errstate(all="ignore"):
        for t in range(T):  # ascending: every pair meets its common topics in ascending order, one elementwise update per topic
            er, eq = order_r[rb[t]:rb[t + 1]], order_q[qb[t]:qb[t + 1]]
            a, b = case.weight[er], case.q_weight[eq]
            if er.size:
                nr[row_of[er]] = nr[row_of[er]] + a.astype(F64) * a.astype(F64)  # (a topic occurs once in a row: no index repeats)
            if eq.size:
                nq[q_of[eq]] = nq[q_of[eq]] + b.astype(F64) * b.astype(F64)
            if er.size and eq.size:
                ix = np.ix_(row_of[er], q_of[eq])
                if measure == BHATTACHARYYA:
                    term = np.sqrt((a[:, None] * b[None, :]).astype(F32)).astype(F64)  # product and root in fp32
                else:
                    term = a.astype(F64)[:, None] * b.astype(F64)[None, :]  # exact
                s[ix] = s[ix] + term
                hit[ix] = True
        num = s.astype(F32)
        if measure == COSINE:
            den = (np.sqrt(nr.astype(F32))[:, None] * np.sqrt(nq.astype(F32))[None, :]).astype(F32)
            score = np.where(den == 0, F32(0), num / np.where(den == 0, F32(1), den)).astype(F32)
        else:
            score = num
    return hit, score


def select(hit, score, doc, exclude, n):
    """the result from the (rows, Q) candidates and scores: the tie-ruled top n per query"""
    Q = hit.shape[1]
    docs = np.full((Q, n), NO_DOC, U32)
    bits_out = np.zeros((Q, n), U32)
    counts = np.zeros(Q, U32)
    cand = np.zeros(Q, np.uint64)
    for q in range(Q):
        ok = hit[:, q] & ((exclude[q] == NO_DOC) | (doc != exclude[q]))
        idx = np.nonzero(ok)[0]
        bits = score[idx, q].view(U32)
        o = ord_bits(bits).astype(np.int64)
        order = np.lexsort((doc[idx].astype(np.int64), -o))
        m = min(n, idx.size)
        docs[q, :m] = doc[idx[order[:m]]]
        bits_out[q, :m] = bits[order[:m]]
        counts[q] = m
        cand[q] = idx.size
    return dict(docs=docs, scores=bits_out, counts=counts, candidates=cand)


def rule(case, measure):
    """-> dict(docs uint32 (Q, n), scores (bits) uint32 (Q, n), counts uint32 (Q,), candidates uint64 (Q,))"""
    hit, score = _scores(case, measure)
    doc = (case.doc_base + np.arange(case.rows, dtype=np.int64)).astype(U32)
    return select(hit, score, doc, case.exclude, case.n)


def score_scalar(measure, row, query):
    """row, query: lists of (topic, np.float32), ascending -> None (no common topic) or the np.float32 score, scalar by scalar"""
    s, nr, nq, common = F64(0), F64(0), F64(0), False
    qd = dict(query)
    with np.errstate(all="ignore"):
        for _, b in query:
            nq = nq + F64(b) * F64(b)
        for t, a in row:
            nr = nr + F64(a) * F64(a)
            if t in qd:
                common = True
                b = qd[t]
                s = s + (F64(np.sqrt(F32(F32(a) * F32(b)))) if measure == BHATTACHARYYA else F64(a) * F64(b))
        if not common:
            return None
        if measure != COSINE:
            return F32(s)
        den = F32(np.sqrt(F32(nr)) * np.sqrt(F32(nq)))
        return F32(0) if den == 0 else F32(F32(s) / den)


def rule_scalar(case, measure):
    R, Q = case.rows, case.Q
    hit = np.zeros((R, Q), bool)
    score = np.zeros((R, Q), F32)
    rows = [list(zip(case.topic[case.off[r]:case.off[r + 1]].tolist(), case.weight[case.off[r]:case.off[r + 1]])) for r in range(R)]
    qs = [list(zip(case.q_topic[case.q_off[q]:case.q_off[q + 1]].tolist(), case.q_weight[case.q_off[q]:case.q_off[q + 1]])) for q in range(Q)]
    for r in range(R):
        for q in range(Q):
            v = score_scalar(measure, rows[r], qs[q])
            if v is not None:
                hit[r, q], score[r, q] = True, v
    doc = (case.doc_base + np.arange(R, dtype=np.int64)).astype(U32)
    return select(hit, score, doc, case.exclude, case.n)


def cuts(case, world):
    """row bounds of `world` shares: two halves; three shares with an empty one in the middle — and, where the case begins with empty rows,
    the first share holds exactly those (rows and no entries)"""
    R = case.rows
    if world == 1:
        return [0, R]
    if world == 2:
        return [0, R // 2, R]
    lead = int(np.argmax(np.diff(case.off) > 0)) if case.topic.size else 0
    a = lead if lead > 0 else R // 3
    return [0, a, a, R]


def share(case, bounds, q):
    """-> (doc_base, (off, topic, weight)) of rows [bounds[q], bounds[q + 1]), offsets from 0"""
    b, e = bounds[q], bounds[q + 1]
    lo, hi = int(case.off[b]), int(case.off[e])
    return case.doc_base + b, (case.off[b:e + 1] - lo, case.topic[lo:hi], case.weight[lo:hi])


def merged(case, measure, bounds):
    """the rule on every share, the shares' lists merged by the key: what W ranks with exact local lists arrive at"""
    parts = []
    for q in range(len(bounds) - 1):
        base, rows = share(case, bounds, q)
        part = Case("share", case.num_topics, case.n, base, rows, (case.q_off, case.q_topic, case.q_weight), exclude=case.exclude)
        parts.append(rule(part, measure))
    Q, n = case.Q, case.n
    out = dict(docs=np.full((Q, n), NO_DOC, U32), scores=np.zeros((Q, n), U32), counts=np.zeros(Q, U32), candidates=np.zeros(Q, np.uint64))
    for q in range(Q):
        d = np.concatenate([p["docs"][q, :p["counts"][q]] for p in parts])
        b = np.concatenate([p["scores"][q, :p["counts"][q]] for p in parts])
        order = np.lexsort((d.astype(np.int64), -ord_bits(b).astype(np.int64)))
        total = sum(int(p["candidates"][q]) for p in parts)
        m = min(n, total)
        out["docs"][q, :m], out["scores"][q, :m], out["counts"][q], out["candidates"][q] = d[order[:m]], b[order[:m]], m, total
    return out


# ---- builders -----------------------------------------------------------------------------------------------------------------------------------
def grid_lists(seed, T, count, maxlen, zero=0.1, lead=0):
    """`count` lists behind `lead` empty ones: random subsets of at most maxlen topics, weights k / 8 (k = 1 .. 39), exactly 0 with probability `zero`"""
    rng = np.random.default_rng(seed)
    out = [[] for _ in range(lead)]
    for _ in range(count):
        m = int(rng.integers(0, min(T, maxlen) + 1))
        tp = np.sort(rng.choice(T, m, replace=False))
        w = np.where(rng.random(m) < zero, 0.0, rng.integers(1, 40, m) / 8.0).astype(F32)
        out.append(list(zip(tp.tolist(), w.tolist())))
    return out


def float_lists(seed, T, count, maxlen):
    """random weights in [2^-20, 4): inexact sums, normal products"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = int(rng.integers(0, min(T, maxlen) + 1))
        tp = np.sort(rng.choice(T, m, replace=False))
        w = (rng.random(m) * 4 + 2.0 ** -20).astype(F32)
        out.append(list(zip(tp.tolist(), w.tolist())))
    return out


def length_lists(seed, T, lengths):
    rng = np.random.default_rng(seed)
    out = []
    for m in lengths:
        tp = np.sort(rng.choice(T, m, replace=False))
        w = (rng.random(m) * 2 + 2.0 ** -10).astype(F32)
        out.append(list(zip(tp.tolist(), w.tolist())))
    return out


def _sharing(rows, queries, q):
    """the rows that store a topic of query q"""
    mine = set(queries[1][queries[0][q]:queries[0][q + 1]].tolist())
    return [r for r in range(rows[0].size - 1) if mine & set(rows[1][rows[0][r]:rows[0][r + 1]].tolist())]


def _cases():
    out = []
    # every Qp, the padded lanes, the last partial group of a wave
    for Q in (1, 2, 3, 5, 33, 64):
        G = 64 // qp_of(Q)
        for R in sorted({1, G - 1, G, G + 1} - {0}):
            out.append(Case("q%d_rows%d" % (Q, R), 7, 5, 100, csr(grid_lists(1000 * Q + R, 7, R, 4)), csr(grid_lists(77 + Q, 7, Q, 3, lead=0)),
                            aim="lanes", exact=True))
    big5 = csr(float_lists(5, 12, 4000, 6))
    out.append(Case("q5_rows4000", 12, 10, 1000, big5, csr(float_lists(6, 12, 5, 5)), aim="many_rows"))
    out.append(Case("q5_rows4000_n256", 12, 256, 1000, big5, csr(float_lists(6, 12, 5, 5)), aim="n256"))
    out.append(Case("q64_rows4000", 12, 10, 0, csr(grid_lists(8, 12, 4000, 6)), csr(grid_lists(9, 12, 64, 5)), aim="many_rows", exact=True))
    # the group's hand-off of a row's entries at the wave width, and the two homes either side of the threshold
    lengths = [0, 1, 63, 64, 65, 200, 3, 0, 64, 129]
    for Q, T, forms in ((3, 256, ("lds", "global")), (64, 256, ("lds", "global", "auto")), (64, 257, ("lds", "global", "auto")), (5, 200, ("lds", "global"))):
        out.append(Case("lengths_q%d_T%d" % (Q, T), T, 8, 3, csr(length_lists(T + Q, T, lengths)), csr(length_lists(Q, T, [min(T, 10 + 3 * q) for q in range(Q)])),
                        aim="lengths", forms=forms))
    out.append(Case("global_T1024_q64", 1024, 10, 0, csr(length_lists(1, 1024, [200, 0, 1, 65, 700] * 20)),
                    csr(length_lists(2, 1024, [1 + 16 * q for q in range(64)])), aim="global"))
    # structure decides who is a candidate
    z = [[(0, 0.0), (2, 1.5)], [(1, 2.0)], [(0, 3.0)], [], [(3, 1.0)], [(0, 0.0)], [(2, 0.0), (3, 0.0)], [(0, -0.0), (1, 1.0)]]
    zq = [[(0, 2.0)], [(0, 0.0), (1, 1.0)], [(2, 0.0), (3, 0.0)], [(4, 1.0)], []]
    out.append(Case("zero_weights", 5, 8, 10, csr(z), csr(zq), aim="zeros", exact=True))
    out.append(Case("fewer_than_n", 5, 20, 10, csr(z), csr(zq[:2]), aim="fewer", exact=True))
    out.append(Case("no_match", 6, 5, 0, csr(grid_lists(3, 5, 70, 3)), csr([[(5, 1.0)], [], [(5, 2.0)]]), aim="no_match", exact=True))
    out.append(Case("no_rows", 4, 5, 11, csr([]), csr([[(0, 1.0)], [(1, 1.0)]]), aim="no_rows", exact=True))
    out.append(Case("rows_without_entries", 4, 5, 11, csr([[], [], [], [], []]), csr([[(0, 1.0)], [(1, 1.0)]]), aim="no_entries", exact=True))
    # bit-equal scores across many documents: the smaller document first; the last document is 0xfffffff0
    tie = [[] for _ in range(3)] + [([(0, 0.5)] if r % 3 else [(0, 0.5), (1, 0.25 * (r % 7))]) + [(2, 1.0)] for r in range(700)]
    tq = [[(0, 2.0), (2, 1.0)], [(1, 1.0)], [(0, 2.0), (2, 1.0)]]
    for n in (5, 256):
        out.append(Case("ties_n%d" % n, 3, n, 0xFFFFFFF1 - 703, csr(tie), csr(tq), aim="tie", exact=True))
    out.append(Case("ties_low_docs", 3, 40, 0x10000 - 300, csr(tie), csr(tq), aim="tie", exact=True))
    # excluded documents
    ex_rows = csr(grid_lists(21, 6, 90, 4, zero=0.0))
    ex_q = csr(grid_lists(22, 6, 4, 4, zero=0.0))
    hit0, hit3 = (_sharing(ex_rows, ex_q, q) for q in (0, 3))  # a candidate in the first half of the rows, one in the second
    out.append(Case("exclude_hits_and_misses", 6, 10, 500, ex_rows, ex_q, exclude=[500 + hit0[0], 7, NO_DOC, 500 + hit3[-1]], aim="exclude", exact=True))
    out.append(Case("query_rows_default", 6, 10, 500, ex_rows, query_rows=[17, 0, 89, 17, 33], aim="query_rows", exact=True))
    out.append(Case("query_rows_exclude_given", 6, 10, 500, ex_rows, query_rows=[17, 0, 89], exclude=[NO_DOC, 500, 3], aim="query_rows", exact=True))
    # the selection's tile of 1024 pairs
    for pairs in (1023, 1024, 1025, 2048, 3072):
        rng = np.random.default_rng(pairs)
        rows = [[(0, float(rng.integers(1, 40) / 8.0)), (1, 1.0)] for _ in range(pairs)]
        out.append(Case("pairs_%d" % pairs, 2, 32, 0, csr(rows), csr([[(0, 1.0)]]), aim="tile", exact=True))
    # a row of zeros under COSINE: den == 0 gives score 0
    out.append(Case("zero_norm", 3, 6, 0, csr([[(0, 0.0), (1, 0.0)], [(0, 1.0)], [(1, 0.0)], [(0, 0.0), (2, 5.0)]]), csr([[(0, 1.0), (1, 1.0)], [(0, 0.0)]]),
                    aim="zero_norm", exact=True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SHARDED = ["ties_n5", "ties_low_docs", "no_match", "exclude_hits_and_misses", "rows_without_entries", "lengths_q5_T200"]


class Refusal:
    """a call through the caller's CSR that ISLE_E_ARG answers, and a piece of the text it gives.  kw: what differs from the good call
    (source rows, queries, n, measure, exclude ... as HotPath.similar_docs takes them)"""

    def __init__(self, name, text, **kw):
        self.name, self.text, self.kw = name, text, kw


def _bad_rows(value, where=1201):
    rows = [[(0, 1.0), (2, 1.0)] for _ in range(1200)]  # entries 0 .. 2399
    flat = csr(rows)
    w = flat[2].copy()
    w.view(U32)[where] = f2b([value])[0] if not isinstance(value, int) else value
    w.view(U32)[2201] = w.view(U32)[where]  # a later one: the first is named
    return flat[0], flat[1], w


GOOD_ROWS = csr([[(0, 1.0), (2, 1.0)] for _ in range(1200)])
GOOD_QUERIES = csr([[(0, 1.0)], [(1, 2.0), (2, 1.0)]])


def _refusals():
    def q(lists):
        return csr(lists)

    nan_q = q([[(0, 1.0)], [(1, float("nan"))]])
    return [
        Refusal("row_weight_nan", "entry 1201 (row 600) has weight", source=_bad_rows(float("nan"))),
        Refusal("row_weight_inf", "entry 1201 (row 600) has weight inf", source=_bad_rows(float("inf"))),
        Refusal("row_weight_negative", "entry 1201 (row 600) has weight -0.5", source=_bad_rows(-0.5)),
        Refusal("row_weight_2_31", "entry 1201 (row 600) has weight 2.14748e+09", source=_bad_rows(2.0 ** 31)),
        Refusal("query_weight_nan", "entry 1 (query 1) has weight", queries=nan_q),
        Refusal("query_weight_negative", "entry 1 (query 1) has weight -1", queries=q([[(0, 1.0)], [(1, -1.0)]])),
        Refusal("query_topic_out_of_range", "query entry 2 (query 1) has topic 3 >= num_topics 3", queries=q([[(0, 1.0)], [(1, 1.0), (3, 1.0)]])),
        Refusal("query_topics_descend", "query entry 2 (query 1), topic 1: the topics of a query must ascend strictly", queries=q([[(0, 1.0)], [(2, 1.0), (1, 1.0)]])),
        Refusal("query_topic_repeats", "query entry 1 (query 0), topic 0: the topics of a query must ascend strictly", queries=q([[(0, 1.0), (0, 1.0)]])),
        Refusal("no_queries", "num_queries = 0 not in [1, 64]", queries=q([])),
        Refusal("65_queries", "num_queries = 65 not in [1, 64]", queries=q([[(0, 1.0)]] * 65)),
        Refusal("n_0", "n = 0 not in [1, 256]", n=0),
        Refusal("n_257", "n = 257 not in [1, 256]", n=257),
        Refusal("unknown_measure", "unknown measure 3", measure=3),
        Refusal("query_row_beyond", "query_rows[1] = 1200 is not below the 1200 rows", queries=np.array([5, 1200], np.uint64)),
        Refusal("doc_base_too_large", "doc_base %d + 1200 rows exceed 4294967281" % (0xFFFFFFF1 - 1199), doc_base=0xFFFFFFF1 - 1199),
        Refusal("row_topic_out_of_range", "entry 1201 (row 600) has topic 3 >= num_topics 3",
                source=(GOOD_ROWS[0], np.where(np.arange(2400) == 1201, 3, GOOD_ROWS[1]).astype(U32), GOOD_ROWS[2])),
    ]


REFUSALS = _refusals()
