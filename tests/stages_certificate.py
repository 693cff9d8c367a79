"""Plain restatement of the two stages around the hot path, and the fp64 certificates of the topic model and the edge topics (no GPU,
no oracle library; numpy only).

Upstream (threshold.hip): normalize_docs, compute_thresholds and threshold_and_copy of the reference, src/sparseMatrix.cpp:136-167,
:357-485, :1285-1361.  Downstream (post.hip): rth_highest_element(_using_CSR) :491-568, find_catchwords :573-595,
construct_topic_model :597-838, construct_edge_topics_v2 src/trainer.cpp:1116-1167.  Everything here uses lists and sorts, as the
reference does: no histograms, no radix passes, no wave merges.  Selections, indices and ordered sums are compared bit for bit; only
the topic model (fp32 atomics on the device, any order) and the edge topics carry a bound.

u = 2^-24, u' = u / (1 - u).  A product of n factors (1 + d_i)^(+-1), |d_i| <= u, differs from 1 by at most gamma(n) = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).

certify_model: |got[w, t] - ref[w, t]| <= (m[w, t] + max_w m[., t] + V + C_MODEL) u' |ref[w, t]| + 2^-126, C_MODEL = 2.
  ref is the fp64 model from the fp32 normalised values nv >= 0; which documents enter which column is decided by exact comparisons
  (the fp32 sums and thresholds are bit-equal to the plain reference, asserted separately), so both sides add the same terms.
  1. Entry (w, t) is the sum of m = m[w, t] terms nv >= 0 (src/sparseMatrix.cpp:810-820), m - 1 additions in any order or tree:
     S^ = S (1 + th), |th| <= gamma(m - 1).  All terms are like-signed, so the bound is relative whatever the order of the atomics.
  2. The column sum (FPasum, :829) adds the V entries, V - 1 additions in any tree, on top of the entries' own errors, the largest of
     which is gamma(max_w m[., t] - 1): T^ = T (1 + th), |th| <= gamma(max_w m - 1 + V - 1).
  3. a = float(1.0 / double(T^)) (:830): the double reciprocal is within 2^-53, the cast to float is one rounding.
  4. got = fl(S^ a): one rounding.
  Roundings: (m - 1) + (max_w m - 1 + V - 1) + 1 + 1 = m + max_w m + V - 1; one more unit covers the 2^-53 of the reciprocal and the
  rounding of the fp64 reference itself (V + m additions of 2^-53 each, asserted far below u): n = m + max_w m + V.
  Size condition, asserted: n <= 5790, for which gamma(n) <= (n + 2) u (n^2 + 2 n <= 2 / u = 2^25); (n + 2) u <= (n + C_MODEL) u'.
  The floor 2^-126 makes the statement hold whether subnormal results are kept or flushed.  A topic that receives no document has
  T = 0, a = inf and 0 * inf = NaN in every entry: the NaN pattern must match exactly.

certify_edge: Edge[w] = fma(b, q[w], fl(a p[w])), a = float32(ratio), b = float32(1.0 - double(a)) (src/trainer.cpp:1153-1159: two
  FPaxpy into a zeroed column; the first is one rounded product, the second one fused multiply-add).  With p, q, a, b >= 0:
  got = (b q + a p (1 + d1)) (1 + d2), so |got - (a p + b q)| <= (a p u + (a p + b q)(u + u^2)) <= (2 u + u^2) ref <= 2 u' ref.
  Bound: 2 u' |ref| + 2^-126; where ref is NaN (a NaN topic vector) got must be NaN.
"""
from collections import Counter

import numpy as np

F = np.float32
U_F32 = 2.0 ** -24
U_PRIME = U_F32 / (1.0 - U_F32)
TINY = 2.0 ** -126
C_MODEL = 2
GAMMA_N_MAX = 5790  # largest n with gamma(n) <= (n + 2) u
W0_C, EPS1_C = 1.0, 1.0 / 60.0  # include/hyperparams.h:8-9
RULES = ("device", "assoc", "fp64", "banker")
MI355X_CUS = 256  # T-stride is sized against this


# ---------------------------------------------------------------------------------------------------------------------------------
# upstream: thresholding
# ---------------------------------------------------------------------------------------------------------------------------------
def _doc_sums(cnt, offs):
    cnt = np.asarray(cnt)
    assert cnt.dtype == np.float32 and np.all(cnt == np.floor(cnt)) and np.all(cnt > 0), "counts are positive integers"
    cs = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    sums = cs[offs[1:]] - cs[offs[:-1]]
    assert sums.size == 0 or sums.max() < 2 ** 24, "a document sum of 2^24 or more is not exact in fp32"
    return sums


def corpus_avg(cnt, offs):
    """-> (avg as float32, tokens, nz_docs)   src/sparseMatrix.cpp:92-99: an integer division."""
    tokens = int(np.asarray(cnt).astype(np.int64).sum())
    nz = int((np.diff(offs) > 0).sum())
    return F(tokens // max(nz, 1)), tokens, nz


def quantise(avg, cnt, sums_e, rule="device"):
    """Rounded normalised value of every entry (:157 then std::round, :381 / :1344).  sums_e: the document sum per entry."""
    avg = F(avg)
    c = np.asarray(cnt, F)
    s = np.asarray(sums_e).astype(F)
    if rule == "device" or rule == "banker":
        x = avg * (c / s)  # float32 quotient, float32 product
        assert x.dtype == np.float32
        q = np.rint(x) if rule == "banker" else np.floor(x.astype(np.float64) + 0.5)
    elif rule == "assoc":
        x = (avg * c) / s
        assert x.dtype == np.float32
        q = np.floor(x.astype(np.float64) + 0.5)
    else:
        assert rule == "fp64"
        q = np.floor(float(avg) * c.astype(np.float64) / s.astype(np.float64) + 0.5)
    return q.astype(np.int64)


def threshold_counts(nz_docs, k):
    """count_gr, count_eq of src/sparseMatrix.cpp:370-373: float32 operands, double arithmetic, 0 -> 1."""
    count_gr = int(W0_C * float(F(nz_docs)) / (2.0 * float(F(k))))
    count_eq = int(np.ceil(3.0 * EPS1_C * W0_C * float(F(nz_docs)) / float(F(k))))
    return max(count_gr, 1), max(count_eq, 1)


def zeta_walk(f, count_gr, count_eq):
    """f: one word's descending list of positive rounded values.  The loop of src/sparseMatrix.cpp:389-480, FPTYPE branch.
    -> (zeta, entries at or above it as the reference counts them, trace)."""
    n = len(f)
    tr = dict(size=n, arm=None, first=None, eq=None, descents=[])
    if n == 0:  # :476-479
        tr["arm"] = "absent"
        return 1.0, 0, tr
    if count_gr > n:  # :395-412, FEW_SAMPLES_THRESHOLD_DROP off
        tr["arm"] = "few"
        return 1.0, n, tr
    neg = -np.asarray(f, np.int64)  # ascending, so that searchsorted stands for lower_/upper_bound under std::greater
    assert np.all(np.diff(neg) >= 0) and f[-1] >= 1
    zeta = int(f[count_gr - 1])  # :445
    tr["first"] = zeta
    while True:
        cur = int(np.searchsorted(neg, -zeta, "left"))
        nxt = int(np.searchsorted(neg, -zeta, "right"))
        assert cur != n and cur != nxt and zeta > 0
        if nxt - cur < count_eq:  # :453-457
            tr["arm"], tr["eq"] = ("accept_first" if not tr["descents"] else "accept_after_descent"), nxt - cur
            return float(zeta), nxt, tr
        if nxt == n or zeta == 1:  # :459-468, BAD_THRESHOLD_DROP off
            tr["arm"], tr["eq"] = ("one" if zeta == 1 else "end"), nxt - cur
            return 1.0, n, tr
        tr["descents"].append((zeta, int(f[nxt]), nxt - cur))
        zeta = int(f[nxt])  # :470


def ref_threshold(V, cnt, rows, offs, k, doc_base=0, rule="device"):
    """A -> B as the reference builds it.  -> dict(avg, tokens, nz_docs, count_gr, count_eq, q, zetas, keep, D, nnz, offs, rows, vals,
    original_cols, entries_above, weight, trace (per word))."""
    cnt = np.asarray(cnt, F)
    rows = np.asarray(rows, np.int64)
    offs = np.asarray(offs, np.int64)
    D = offs.shape[0] - 1
    assert rule in RULES
    avg, tokens, nz = corpus_avg(cnt, offs)
    sums = _doc_sums(cnt, offs)
    lens = np.diff(offs)
    doc_of = np.repeat(np.arange(D), lens)
    q = quantise(avg, cnt, sums[doc_of], rule)
    assert q.size == 0 or q.max() <= int(avg)  # :380
    count_gr, count_eq = threshold_counts(nz, k)
    # :289-354 the descending list of positive values of every word
    pos = q > 0
    order = np.lexsort((-q[pos], rows[pos]))
    rw, qv = rows[pos][order], q[pos][order]
    start = np.searchsorted(rw, np.arange(V + 1), "left")
    zetas = np.ones(V, F)
    trace = []
    new_nnzs = 0
    for w in range(V):
        z, add, tr = zeta_walk(qv[start[w]:start[w + 1]], count_gr, count_eq)
        zetas[w] = z
        new_nnzs += add
        trace.append(tr)
    keep = q.astype(np.float64) >= zetas[rows].astype(np.float64)  # :1348
    kept = np.bincount(doc_of[keep], minlength=D) if D else np.zeros(0, np.int64)
    assert int(keep.sum()) == new_nnzs, "compute_thresholds' count and threshold_and_copy's disagree"
    cols = np.flatnonzero(kept > 0)  # :1355-1359
    boffs = np.concatenate([[0], np.cumsum(kept[cols])]).astype(np.int64)
    weight = np.bincount(doc_of[keep], weights=zetas[rows[keep]].astype(np.float64), minlength=D).astype(F) if D else np.zeros(0, F)
    return dict(avg=float(avg), tokens=tokens, nz_docs=nz, count_gr=count_gr, count_eq=count_eq, q=q, zetas=zetas, keep=keep, V=V, D=int(cols.size),
                nnz=int(keep.sum()), offs=boffs, rows=rows[keep].astype(np.uint32), vals=np.sqrt(zetas[rows[keep]]).astype(F),  # :1349
                original_cols=(cols + doc_base).astype(np.uint64), entries_above=new_nnzs, weight=weight, trace=trace, kept=kept)


B_FIELDS = ("zetas", "offs", "rows", "vals", "original_cols")


def assert_same_B(got, want, what=""):
    """Bit for bit: zetas, offs, rows, vals, original_cols, D, nnz."""
    assert got["D"] == want["D"] and got["nnz"] == want["nnz"], "%s: B is %d x %d entries, the reference has %d x %d" % (
        what, got["D"], got["nnz"], want["D"], want["nnz"])
    for f in B_FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, "%s: %s has shape %s, the reference %s" % (what, f, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), np.asarray(b, F).view(np.uint32)
        bad = np.flatnonzero(a.astype(np.int64) != b.astype(np.int64))
        assert bad.size == 0, "%s: %s differs at %d places, first at %d: %r vs %r" % (what, f, bad.size, bad[0], got[f][bad[0]], want[f][bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------------
# downstream: catchwords, document-topic sums, topic model, edge topics
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_normalize(cnt, offs, avg):
    """nv = avg * (count / doc_sum) in float32   src/sparseMatrix.cpp:157."""
    cnt = np.asarray(cnt, F)
    sums = _doc_sums(cnt, offs)
    nv = F(avg) * (cnt / sums[np.repeat(np.arange(len(sums)), np.diff(offs))].astype(F))
    assert nv.dtype == np.float32
    return nv


def cluster_of_docs(D, original_cols, assign, doc_base=0):
    """src/trainer.cpp:572-575: the cluster of every document of A, -1 for the documents thresholding dropped."""
    cl = np.full(D, -1, np.int32)
    cl[np.asarray(original_cols, np.int64) - doc_base] = np.asarray(assign, np.int32)
    return cl


def ref_catch_thresholds(V, rows, offs, nv, cluster_of, k, r):
    """src/sparseMatrix.cpp:539-566 (and :496-500 for an empty cluster).  -> (thr (V, k) F-order, Counter of the arms populated)."""
    rows = np.asarray(rows, np.int64)
    D = len(offs) - 1
    cl = np.asarray(cluster_of, np.int64)
    sizes = np.bincount(cl[cl >= 0], minlength=k)
    doc_of = np.repeat(np.arange(D), np.diff(offs))
    lists = {}
    for i in np.flatnonzero(cl[doc_of] >= 0):
        lists.setdefault((int(rows[i]), int(cl[doc_of[i]])), []).append(nv[i])
    thr = np.zeros((V, k), F, order="F")
    arms = Counter()
    arms["empty cluster"] = int((sizes == 0).sum())
    for (w, t), f in lists.items():
        n, S = len(f), int(sizes[t])
        if n == r:
            arms["n == r"] += 1
        if n > r:
            arms["n == r + 1" if n == r + 1 else "n > r + 1"] += 1
            thr[w, t] = sorted(f, reverse=True)[r - 1]
        elif r >= S:
            if n == S:
                arms["S == r, n == S" if S == r else "S < r, n == S"] += 1
                thr[w, t] = min(f)
            else:
                arms["n < S <= r"] += 1
        else:
            arms["S > r >= n"] += 1
    return thr, arms


def ref_find_catchwords(thr, rho, strict=True):
    """src/sparseMatrix.cpp:573-595: topic t takes word w when thr[w, t] > rho * thr[w, o] (a double product) for every o != t; with one
    topic the loop never sets the flag.  -> catch_topic int32[V], -1 where none.  strict=False (>=) exists for the CPU tests only."""
    thr = np.asarray(thr)
    assert thr.dtype == np.float32
    V, k = thr.shape
    t64 = thr.astype(np.float64)
    ct = np.full(V, -1, np.int32)
    for t in range(k):
        if k == 1:
            break
        lhs, rhs = t64[:, t][:, None], float(rho) * np.delete(t64, t, axis=1)
        ok = np.all(lhs > rhs if strict else lhs >= rhs, axis=1)
        assert not strict or not np.any(ok & (ct >= 0)), "a word qualified twice"
        ct[ok & (ct < 0)] = t
    return ct


def ref_doc_topic_sums(rows, offs, nv, catch_topic, k, order="entry"):
    """src/sparseMatrix.cpp:656-708: float32 sums of the catchword entries, one at a time in entry order; the non-zero sums in topic
    order; the two heaviest topics by the strict-compare scan, reported when both exist.  order="reversed": for the CPU tests only."""
    rows = np.asarray(rows, np.int64)
    D = len(offs) - 1
    ct_e = np.asarray(catch_topic)[rows]
    dts_off, topic, val = [0], [], []
    top1, top2 = np.full(D, -1, np.int32), np.full(D, -1, np.int32)
    for d in range(D):
        idx = np.arange(offs[d], offs[d + 1])
        idx = idx[ct_e[idx] >= 0]
        if order == "reversed":
            idx = idx[::-1]
        acc = {}
        for i in idx:
            t = int(ct_e[i])
            acc[t] = F(acc.get(t, F(0)) + nv[i])
        mx = mx2 = F(0)
        t1 = t2 = -1
        for t in sorted(acc):
            v = acc[t]
            if v == 0:
                continue
            topic.append(t)
            val.append(v)
            if v > mx:
                mx2, t2, mx, t1 = mx, t1, v, t
            elif v > mx2:
                mx2, t2 = v, t
        dts_off.append(len(topic))
        if t1 >= 0 and t2 >= 0:
            top1[d], top2[d] = t1, t2
    return dict(dts_off=np.array(dts_off, np.int64), dts_topic=np.array(topic, np.uint32), dts_val=np.array(val, F), top1=top1, top2=top2)


def ref_model_thresholds(dts_topic, dts_val, k, rank):
    """src/sparseMatrix.cpp:722-753: the rank-th largest sum of a topic that has at least `rank` sums, else 0."""
    out = np.zeros(k, F)
    for t in range(k):
        v = np.sort(dts_val[dts_topic == t])[::-1]
        if rank >= 1 and len(v) >= rank:
            out[t] = v[rank - 1]
    return out


def model_contributions(offs, cluster_of, dts, mthr, strict=True, skip_doc=None):
    """(topic, document) pairs that src/sparseMatrix.cpp:807-821 adds: a sum strictly above its topic's threshold, and the document's own
    cluster (a document can be added twice to one column)."""
    out = []
    for d in range(len(offs) - 1):
        if d == skip_doc:
            continue
        for j in range(dts["dts_off"][d], dts["dts_off"][d + 1]):
            t = int(dts["dts_topic"][j])
            if (dts["dts_val"][j] > mthr[t]) if strict else (dts["dts_val"][j] >= mthr[t]):
                out.append((t, d))
        if cluster_of[d] >= 0:
            out.append((int(cluster_of[d]), d))
    return out


def ref_model64(V, rows, offs, nv, contribs, k):
    """-> (model (V, k) F-order float64, L1-normalised, NaN where the column is empty; m (V, k): terms per entry)."""
    rows = np.asarray(rows, np.int64)
    M = np.zeros((V, k), np.float64, order="F")
    m = np.zeros((V, k), np.int64, order="F")
    nv64 = np.asarray(nv, np.float64)
    for t, d in contribs:
        s = slice(offs[d], offs[d + 1])
        M[rows[s], t] += nv64[s]
        m[rows[s], t] += 1
    tot = M.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        M = np.where(tot[None, :] > 0, M / tot[None, :], np.nan)
    return np.asfortranarray(M), m


def emulate_model32(V, rows, offs, nv, contribs, k, rng):
    """The model in float32 with the contributions and the column sum taken in a random order (stands for the atomics)."""
    rows = np.asarray(rows, np.int64)
    M = np.zeros((V, k), F, order="F")
    for i in rng.permutation(len(contribs)):
        t, d = contribs[i]
        s = slice(offs[d], offs[d + 1])
        M[rows[s], t] = M[rows[s], t] + np.asarray(nv, F)[s]
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(k):
            tot = F(0)
            for w in rng.permutation(V):
                tot = F(tot + abs(M[w, t]))
            M[:, t] = M[:, t] * F(1.0 / np.float64(tot))
    return M


def certify_model(got, ref64, m, V):
    """See the module docstring.  -> dict(max_ratio)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape == m.shape and got.shape[0] == V
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern: %d entries differ" % int((np.isnan(got) != nan).sum())
    n = m + m.max(0)[None, :] + V
    assert int(n.max()) <= GAMMA_N_MAX, "size condition: n = %d" % int(n.max())
    assert int(n.max()) * 2.0 ** -53 <= 2.0 ** -12 * U_F32  # the fp64 reference's own rounding
    ok = ~nan
    bound = (n + C_MODEL) * U_PRIME * np.abs(np.where(ok, ref64, 0.0)) + TINY
    err = np.abs(np.where(ok, got.astype(np.float64) - np.where(ok, ref64, 0.0), 0.0))
    ratio = err / bound
    if (ratio > 1.0).any():
        w, t = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%d model entries outside the bound; worst (word %d, topic %d): %r vs fp64 %r, error / bound %.4g (m = %d)" % (
            int((ratio > 1).sum()), w, t, float(got[w, t]), float(ref64[w, t]), ratio[w, t], m[w, t]))
    return dict(max_ratio=float(ratio.max()), rel_max=float(((n + C_MODEL) * U_PRIME).max()))


def edge_coefficients(primary_ratio):
    a = F(primary_ratio)
    return a, F(1.0 - float(a))


def certify_edge(got, model32, pairs, primary_ratio=0.7):
    """See the module docstring.  -> dict(max_ratio)."""
    got = np.asarray(got)
    model32 = np.asarray(model32)
    assert got.dtype == np.float32 and model32.dtype == np.float32
    a, b = edge_coefficients(primary_ratio)
    worst = 0.0
    for e, (p, q) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        ref = float(a) * model32[:, p].astype(np.float64) + float(b) * model32[:, q].astype(np.float64)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got[:, e]), nan), "edge topic %d: NaN pattern" % e
        assert np.all(ref[~nan] >= 0)
        err = np.abs(got[:, e].astype(np.float64)[~nan] - ref[~nan])
        ratio = err / (2.0 * U_PRIME * ref[~nan] + TINY)
        assert not (ratio > 1.0).any(), "edge topic %d (%d, %d): error / bound %.4g" % (e, p, q, ratio.max())
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    return dict(max_ratio=worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs.  Every builder returns a dict with V, cnt, rows, offs, k (the num_topics thresholding runs with) and its own design notes.
# ---------------------------------------------------------------------------------------------------------------------------------
def _csc(V, docs):
    """docs: one {word: count} per document."""
    offs, rows, cnt = [0], [], []
    for d in docs:
        ws = sorted(d)
        assert not ws or (0 <= ws[0] and ws[-1] < V)
        rows += ws
        cnt += [d[w] for w in ws]
        offs.append(len(rows))
    assert all(c >= 1 and c == int(c) for c in cnt)
    return dict(V=V, cnt=np.array(cnt, F), rows=np.array(rows, np.uint32), offs=np.array(offs, np.int64))


def _pad_to_avg(docs, word, avg, nz_target):
    """Appends one-word filler documents so that there are nz_target non-empty documents holding avg * nz_target tokens."""
    nz = sum(1 for d in docs if d)
    tokens = sum(sum(d.values()) for d in docs)
    nfill, need = nz_target - nz, avg * nz_target - tokens
    assert nfill >= 1 and need >= nfill, (nfill, need)
    base = need // nfill
    fill = [base] * nfill
    fill[-1] += need - base * nfill
    assert max(fill) < 2 ** 24
    docs += [{word: c} for c in fill]


_CACHE = {}


def _cached(fn):
    def wrap(*a):
        key = (fn.__name__,) + a
        if key not in _CACHE:
            _CACHE[key] = fn(*a)
        return _CACHE[key]
    wrap.__name__ = fn.__name__
    return wrap


# ---- T-round ---------------------------------------------------------------------------------------------------------------------
# 9, 11 and 13 have exact x.5 ties; a search over sums below 40 avg finds order-sensitive triples for 11 but none for 9 and 13 (13 * (15 / 26) is
# 7.5 exactly in float32 as well), so 19 and 23, which have them, are added.
ROUND_AVGS = (9, 11, 13, 19, 23)


def search_triples(avg):
    """Small (cnt, sum) whose rounded value under the device rule differs from another rule.  -> list of dict(cnt, sum, q (per rule),
    tie (device value is exactly x.5))."""
    out = []
    for s in range(2, 6 * avg + 1):
        c = np.arange(1, s, dtype=np.int64)
        se = np.full(c.shape, s)
        q = {r: quantise(avg, c.astype(F), se, r) for r in RULES}
        x = (F(avg) * (c.astype(F) / se.astype(F))).astype(np.float64)
        tie = (x - np.floor(x)) == 0.5
        for i in np.flatnonzero((q["device"] != q["assoc"]) | (q["device"] != q["fp64"]) | (q["device"] != q["banker"]) | tie):
            out.append(dict(cnt=int(c[i]), sum=s, q={r: int(q[r][i]) for r in RULES}, tie=bool(tie[i])))
    return out


@_cached
def t_round_case(avg):
    """nz_docs = 480, k = 4: count_gr = 60, count_eq = 6.  Per probe word: 58 one-word documents (value avg), three pin documents at the
    value Z = the larger of the probe's two candidate values, and the probe document.  The word's list is 58 x avg, then three or four
    Z: freqs[59] = Z with 3 or 4 < 6 equal values, so zeta = Z whichever way the probe rounds, and the probe survives iff it rounds to Z."""
    k, nz = 4, 480
    chosen = []
    found = search_triples(avg)

    def usable(t):
        z = max(t["q"].values())
        return 2 <= z <= avg - 1 and min(t["q"].values()) == z - 1

    for want in ("banker", "assoc", "fp64"):
        got = [t for t in found if usable(t) and t["q"][want] != t["q"]["device"] and t not in chosen]
        chosen += got[:2]
    chosen += [t for t in found if t["tie"] and 2 <= t["q"]["device"] <= avg - 1 and t not in chosen][:1]  # a tie whatever the parity
    assert len(chosen) <= 7
    P = len(chosen)
    f_word, g_word = P, P + 1
    docs, probes = [], []
    for j, t in enumerate(chosen):
        Z = max(max(t["q"].values()), t["q"]["device"])
        docs += [{j: 1} for _ in range(58)]
        docs += [{j: Z, f_word: avg - Z} for _ in range(3)]
        probes.append(dict(word=j, doc=len(docs), Z=Z, **t))
        docs.append({j: t["cnt"], f_word: t["sum"] - t["cnt"]})
        docs.append({})  # an empty document behind every probe
    _pad_to_avg(docs, g_word, avg, nz)
    case = _csc(P + 2, docs)
    case.update(k=k, avg=avg, probes=probes)
    return case


# ---- T-zeta ----------------------------------------------------------------------------------------------------------------------
ZETA_WORDS = {  # word -> (value, how many) lists; count_gr = 30, count_eq = 3, avg = 12
    1: [(3, 29)],                                  # size < count_gr
    2: [(5, 29), (4, 1)],                          # size == count_gr; first zeta 4 accepted
    3: [(6, 29), (5, 1), (2, 10)],                 # first zeta accepted, one equal value
    4: [(6, 28), (5, 2), (2, 10)],                 # #eq == count_eq - 1: accepts
    5: [(6, 28), (5, 3), (4, 1)],                  # #eq == count_eq: descends one bin, accepts 4
    6: [(9, 28), (8, 3), (5, 2)],                  # descends over the empty bins 7 and 6, accepts 5
    7: [(6, 28), (5, 3), (3, 3)],                  # descends to the last present value and ends there: 1
    8: [(6, 28), (2, 3), (1, 4)],                  # reaches zeta == 1 with #eq >= count_eq: 1
    9: [(12, 31), (4, 2)],                         # first zeta is avg itself (one-word documents), the largest bin in use
}
ZETA_EXPECT = {0: ("absent", 1), 1: ("few", 1), 2: ("accept_first", 4), 3: ("accept_first", 5), 4: ("accept_first", 5), 5: ("accept_after_descent", 4),
               6: ("accept_after_descent", 5), 7: ("end", 1), 8: ("one", 1), 9: ("accept_after_descent", 4)}


@_cached
def t_zeta_case():
    avg, k, nz, f_word = 12, 8, 480, 10
    items = sorted(((v, w) for w, spec in ZETA_WORDS.items() for v, n in spec for _ in range(n)), reverse=True)
    docs, used = [], []
    for v, w in items:  # first fit: every document sums to avg, so that the rounded value of an entry is its count
        for i, d in enumerate(docs):
            if w not in d and used[i] + v <= avg:
                d[w] = v
                used[i] += v
                break
        else:
            docs.append({w: v})
            used.append(v)
    for d, u in zip(docs, used):
        if u < avg:
            d[f_word] = avg - u
    assert len(docs) < nz
    docs += [{f_word: avg} for _ in range(nz - len(docs))]
    case = _csc(12, docs)  # words 0 and 11 never occur
    case.update(k=k, avg=avg)
    return case


# ---- T-lanes ---------------------------------------------------------------------------------------------------------------------
LANE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 200)
LANE_PATTERNS = ("all", "none", "first", "last", "alternating")


def lane_mask(n, pattern):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": i % 64 == 0, "last": (i % 64 == 63) | (i == n - 1),
            "alternating": i % 2 == 0}[pattern]


# T-sampled: sample_rate 0.5 on the T-lanes corpus.  A document's key is u^(1 / weight), and the 750 documents that pin the drop words
# weigh 1900 against at most 200 for a lane document, so most seeds keep no lane document at all.  With this seed the CPU port keeps the
# documents (128, all), (129, all) and (128, alternating); test_stages_certificate_cpu.py asserts it.
SAMPLED_RATE, SAMPLED_SEED = 0.5, 11
SAMPLED_LANES_KEPT = {(128, "all"), (129, "all"), (128, "alternating")}


@_cached
def t_lanes_case():
    """avg = 2000, nz_docs = 900, k = 30: count_gr = 15, count_eq = 2.  Pattern p, position i: word 400 p + 2 i is a `keep` word (it occurs
    in at most eight documents: size < count_gr, zeta 1), word 400 p + 2 i + 1 a `drop` word: it stands with value 100 in fourteen documents
    and with value 95 in one, so freqs[14] = 95 with one equal value: zeta 95, above the value of any entry of a document of 63 or more
    equal counts (at most 32).  A one-entry document has value avg and survives whatever its word."""
    avg, k, nz = 2000, 30, 900
    F_word, G_word, V = 2000, 2001, 2002
    docs, lanes = [], []
    for p, pat in enumerate(LANE_PATTERNS):
        for n in LANE_SIZES:
            mask = lane_mask(n, pat)
            lanes.append(dict(doc=len(docs), n=n, pattern=pat, mask=mask))
            docs.append({400 * p + 2 * i + (0 if mask[i] else 1): 1 for i in range(n)})
            docs.append({})
    drop = [400 * p + 2 * i + 1 for p in range(5) for i in range(200)]
    for g in range(0, len(drop), 20):
        grp = drop[g:g + 20]
        docs += [{w: 1 for w in grp} for _ in range(14)]
        d = {w: 19 for w in grp}
        d[F_word] = 20
        docs.append(d)
    _pad_to_avg(docs, G_word, avg, nz)
    case = _csc(V, docs)
    case.update(k=k, avg=avg, lanes=lanes)
    return case


# ---- T-scan ----------------------------------------------------------------------------------------------------------------------
SCAN_D = (4095, 4096, 4097, 8193)


@_cached
def t_scan_case(D):
    """Every document sums to 40 = avg.  Words 0 and 1 stand with the values 21..39, seven times each, in two-word documents, and with
    the value 20 in the documents {0: 20, 1: 20}; k is the smallest for which both zetas exceed 20, so that those documents are dropped
    whole.  Every third document is empty or such a document, in turn; the others have one to three entries."""
    rng = np.random.default_rng(D)
    high = [{w: v, 2: 40 - v} for w in (0, 1) for v in range(21, 40) for _ in range(7)]
    docs = []
    for d in range(D):
        if d % 3 == 2:
            docs.append({} if (d // 3) % 2 == 0 else {0: 20, 1: 20})
        elif high and d % 2 == 0:
            docs.append(high.pop())
        else:
            n = int(rng.integers(1, 4))
            ws = rng.choice(np.arange(3, 11), size=n, replace=False)
            cuts = np.sort(rng.choice(np.arange(1, 40), size=n - 1, replace=False)) if n > 1 else np.zeros(0, np.int64)
            parts = np.diff(np.concatenate([[0], cuts, [40]]))
            docs.append({int(w): int(c) for w, c in zip(ws, parts)})
    assert not high
    case = _csc(11, docs)
    for k in range(1, 400):
        z = ref_threshold(11, case["cnt"], case["rows"], case["offs"], k)["zetas"]
        if z[0] > 20 and z[1] > 20:
            break
    else:
        raise AssertionError("no k drops the {0: 20, 1: 20} documents")
    case.update(k=k, avg=40, doc_offset=1000 if D == 4097 else 0)
    return case


# ---- T-stride --------------------------------------------------------------------------------------------------------------------
@_cached
def t_stride_case():
    """70 000 documents of about nine entries: more documents than num_cus * 32 * 4 waves and more entries than num_cus * 8 * 256 threads
    at 256 compute units, so that every grid-stride loop of threshold.hip takes at least two trips."""
    rng = np.random.default_rng(70000)
    D, V, W = 70000, 600, 12
    ids = np.sort(rng.integers(0, V, size=(D, W)), axis=1)
    n = rng.integers(6, W + 1, size=D)
    n[::50] = 0
    take = (np.arange(W)[None, :] < n[:, None]) & np.concatenate([np.ones((D, 1), bool), ids[:, 1:] > ids[:, :-1]], axis=1)
    offs = np.concatenate([[0], np.cumsum(take.sum(1))]).astype(np.int64)
    rows = ids[take].astype(np.uint32)
    cnt = rng.integers(1, 61, size=rows.shape[0]).astype(F)  # values spread over many bins: some zetas end above 1
    return dict(V=V, cnt=cnt, rows=rows, offs=offs, k=40)


def threshold_cases():
    """name -> builder call, for every thresholding case both test files run."""
    out = {"round-%d" % a: (t_round_case, a) for a in ROUND_AVGS}
    out["zeta"] = (t_zeta_case,)
    out["lanes"] = (t_lanes_case,)
    out.update({"scan-%d" % D: (t_scan_case, D) for D in SCAN_D})
    out["stride"] = (t_stride_case,)
    return out


def build(spec):
    return spec[0](*spec[1:])


# ---- downstream cases ------------------------------------------------------------------------------------------------------------
def _finish_post(case, want_cluster):
    """Thresholds the corpus with the plain reference and maps the wanted cluster of every document of A to B's columns."""
    B = ref_threshold(case["V"], case["cnt"], case["rows"], case["offs"], case["k"])
    oc = B["original_cols"].astype(np.int64)
    want = np.asarray(want_cluster, np.int32)
    D = len(case["offs"]) - 1
    assign = want[oc]
    assert np.all(assign >= 0), "a document that B keeps has no cluster"
    case.update(B=B, assign=assign.astype(np.uint32), cl=cluster_of_docs(D, oc, assign), nv=ref_normalize(case["cnt"], case["offs"], B["avg"]),
                want_cluster=want)
    return case


CATCH_K = (1, 2, 63, 64, 65, 130)
CATCH_RHOS = (1.1, 1.5, 2.0)
CATCH_SUM = 8192  # = avg: a count c in a document of this sum has the normalised value c exactly


def _ulp_above(rho, c2_first):
    """(c2, c1, S1): float32(c1 / S1) is the float32 next above rho * float32(c2 / 8192), which is itself a float32."""
    for c2 in range(c2_first, c2_first + 400, 2):
        x2 = F(c2) / F(CATCH_SUM)
        tgt = float(rho) * float(x2)
        if float(F(tgt)) != tgt or tgt >= 0.9:
            continue
        t = np.nextafter(F(tgt), F(np.inf))
        S1 = np.arange(1024, 15000)
        c1 = np.rint(float(t) * S1)
        hit = np.flatnonzero(((c1.astype(F) / S1.astype(F)) == t) & (c1 < S1))
        if hit.size:
            return c2, int(c1[hit[0]]), int(S1[hit[0]])
    raise AssertionError("no fraction one ulp above rho * m2")


@_cached
def p_catch_case(k):
    """One document per cluster and r = 1: thr[w, t] is the normalised value of word w in document t (the arm r >= S, n == S).  Documents
    sum to 8192 = avg, so thr[w, t] is the count itself; the two `ulp` rows use a document of another sum (and one that makes up for it)."""
    S0 = CATCH_SUM
    special = {4: None, 6: None, 7: None, 8: None} if k >= 63 else {}
    plain = [t for t in range(k) if t not in special]
    rows_spec = []
    for T in sorted({0, 63, 64, k - 1} & set(plain)):
        rows_spec.append(("max@%d" % T, {**{t: 1 for t in plain}, T: 8}))
    if k > 65:
        rows_spec.append(("tie(t,t+64)", {**{t: 1 for t in plain}, 1: 8, 65: 8}))
    if k >= 4:
        rows_spec.append(("tie(t,t+1)", {**{t: 1 for t in plain}, 2: 8, 3: 8}))
    elif k == 2:
        rows_spec.append(("tie(t,t+1)", {0: 8, 1: 8}))
    rows_spec.append(("zero", {}))
    rows_spec.append(("single@last", {k - 1: 5}))
    rows_spec.append(("single@0", {0: 5}))
    if k >= 2:
        rows_spec.append(("eq1.5", {k - 1: 3, 0: 2}))
        rows_spec.append(("eq2.0", {0: 4, k - 1: 2}))
    sums = {t: S0 for t in range(k)}
    if special:
        c2a, c1a, S1a = _ulp_above(1.5, 2731)
        c2b, c1b, S1b = _ulp_above(2.0, 1365)
        rows_spec.append(("ulp1.5", {4: c1a, 5: c2a}))
        rows_spec.append(("ulp2.0", {7: c1b, 5: c2b}))
        sums.update({4: S1a, 6: 2 * S0 - S1a, 7: S1b, 8: 2 * S0 - S1b})
    pad = len(rows_spec)
    docs = []
    for t in range(k):
        d = {w: spec[t] for w, (_, spec) in enumerate(rows_spec) if t in spec}
        rest = sums[t] - sum(d.values())
        assert rest >= 0
        if rest:
            d[pad] = rest
        docs.append(d)
    case = _csc(pad + 1, docs)
    case.update(k=1, topics=k, r=1, names=[n for n, _ in rows_spec], spec=[s for _, s in rows_spec], avg=S0)
    return _finish_post(case, np.arange(k))


@_cached
def p_arms_case():
    """k = 5 clusters, r = 3: cluster 0 has six documents and the one-word fillers (S > r), cluster 1 three (S == r), cluster 2 two (S < r), cluster 3 none, cluster 4
    five.  Three documents of 100 equal counts round to 0 everywhere (avg = 40): thresholding drops them and they belong to no cluster,
    although they hold every probe word."""
    docs, want = [], []

    def add(t, d):
        docs.append(d)
        want.append(t)

    c0 = [dict() for _ in range(6)]
    for w, members in ((0, range(5)), (1, range(3)), (2, range(4)), (8, range(6))):  # n = 5 > r + 1; n == r; n == r + 1; in all six
        for j in members:
            c0[j][w] = 2 + ((j + w) % 4)
    c1 = [{3: 2 + j, 5: 4 - j} for j in range(3)]   # word 3: n == S == r -> minimum
    del c1[2][5]                                    # word 5: n = 2 < S = 3 <= r -> 0
    c2 = [{4: 3 + j, 6: 2} for j in range(2)]       # word 4: S < r, n == S -> minimum
    del c2[1][6]                                    # word 6: n = 1 < S = 2 <= r -> 0
    c4 = [{7: 1 + j, 0: 1} for j in range(5)]       # word 7: n = 5 > r + 1; word 0 again in cluster 4
    for t, group in ((0, c0), (1, c1), (2, c2), (4, c4)):
        for d in group:
            d[9] = 40 - sum(d.values())             # every document sums to avg = 40
            assert d[9] >= 1
            add(t, d)
    for _ in range(3):
        add(-1, {w: 1 for w in range(100)})         # rounds to 0 everywhere: dropped from B
    while 40 * (len(docs) + 1) - sum(sum(d.values()) for d in docs) < 1:
        add(0, {9: 1})                              # one-word documents of cluster 0 until one more can bring avg to 40
    add(0, {9: 40 * (len(docs) + 1) - sum(sum(d.values()) for d in docs)})
    case = _csc(100, docs)
    case.update(k=1, topics=5, r=3, rank=2)
    return _finish_post(case, want)


SELECT_LENGTHS = (2, 255, 256, 257, 1000)
SELECT_KINDS = ("equal", "run", "top16")


def select_ranks():
    out = {1}
    for n in SELECT_LENGTHS:
        out |= {max(n // 2, 1), n - 1, n, n + 1}
    return sorted(out)


@_cached
def p_select_case():
    """One topic per (length, kind); its documents hold the topic's word and a filler.  equal: one value.  run: distinct values with runs of
    equal ones over the top two, the middle five and the bottom three ranks.  top16: count 30 000 in sums 60 000 .. 60 100 (up to 101
    distinct quotients in [0.4991, 0.5], which share sign, exponent and the seven leading mantissa bits)."""
    docs, want, segs = [], [], []
    pad = len(SELECT_LENGTHS) * len(SELECT_KINDS)
    for li, n in enumerate(SELECT_LENGTHS):
        for ki, kind in enumerate(SELECT_KINDS):
            t = w = li * len(SELECT_KINDS) + ki
            segs.append(dict(topic=t, word=w, n=n, kind=kind))
            for j in range(n):
                if kind == "equal":
                    c, s = 30000, 60000
                elif kind == "run":
                    jj = j
                    if j < 2:
                        jj = 0
                    elif abs(j - n // 2) <= 2:
                        jj = n // 2
                    elif j >= n - 3:
                        jj = n - 3
                    c, s = 40000 - 20 * jj, 60000
                else:
                    c, s = 30000, 60000 + (j * 37) % 101
                docs.append({w: c, pad: s - c})
                want.append(t)
    case = _csc(pad + 1, docs)
    case.update(k=1, topics=pad, segs=segs, r=1, rank=1)
    return _finish_post(case, want)


DTS_K = (65, 130)
DTS_V = 256


def dts_topics(k):
    return [0, 1, 63, 64] + ([65, 127, 128, k - 1] if k > 65 else [])


def dts_word(i, catch):
    """The word at position i of a test document: 2 i is a catchword, 2 i + 1 a plain word; positions 127 and 128 have catchwords only."""
    if i >= 127:
        assert catch
        return 254 if i == 127 else 255
    return 2 * i + (0 if catch else 1)


def dts_catch_topic(w, k):
    """The designed catch topic of word w (-1: plain).  Catchword number j belongs to the topic dts_topics(k)[j % len]."""
    if w == 255:
        j = 128
    elif w % 2 == 0:
        j = w // 2
    else:
        return -1
    tl = dts_topics(k)
    return tl[j % len(tl)]


@_cached
def p_dts_case(k):
    """r = 1.  Every catchword stands alone (value avg) in two documents of its topic's cluster, every plain word in two documents of
    cluster 0 and two of cluster 1 (a tied maximum: no catchword).  The test documents have 64, 65 and 129 entries of small values
    (below avg / 1.1), with catchwords at the positions 0, 63, 64 and 128 among others.  Topic 10 (among others) has no document: a NaN column."""
    rng = np.random.default_rng(k)
    docs, want, notes = [], [], {}

    def add(t, d, note=None):
        if note:
            notes[note] = len(docs)
        docs.append(d)
        want.append(t)

    for w in range(DTS_V):
        t = dts_catch_topic(w, k)
        for tt in ([t, t] if t >= 0 else [0, 0, 1, 1]):
            add(tt, {w: 60})
    tl = dts_topics(k)

    def doc(n, catch_positions, counts=None):
        cp = set(catch_positions) | {i for i in (127, 128) if i < n}
        return {dts_word(i, i in cp): int(counts[i]) if counts is not None else int(rng.integers(1, 6)) for i in range(n)}

    add(2, doc(64, []), "no catchword")
    add(3, doc(64, [0, 63]), "boundaries 0, 63")
    add(tl[0], doc(65, [0, 63, 64]), "boundaries 0, 63, 64")
    add(tl[1], doc(129, [0, 63, 64]), "boundaries 0, 63, 64, 128")
    L = len(tl)
    add(5, doc(64, [0, L, 2 * L]), "one topic only")                      # three catchwords of topic tl[0]
    add(6, doc(65, [1, 2], counts=np.full(65, 3)), "two equal sums")       # one catchword each of tl[1] and tl[2], equal counts
    add(tl[3], doc(65, [3, 3 + L, 3 + 2 * L, 5]), "both routes")           # three catchwords of its own cluster's topic
    for s in range(200):  # three or more catchwords of one topic whose float32 sum depends on the order
        r2 = np.random.default_rng(1000 * k + s)
        counts = r2.integers(1, 40, size=65)
        d = doc(65, [2, 2 + L, 2 + 2 * L, 2 + 3 * L], counts=counts)
        tot = sum(d.values())
        v = [F(70) * (F(d[dts_word(2 + j * L, True)]) / F(tot)) for j in range(4)]  # avg is set to 70 below
        fwd = F(F(F(v[0] + v[1]) + v[2]) + v[3])
        rev = F(F(F(v[3] + v[2]) + v[1]) + v[0])
        if fwd != rev:
            add(7, d, "order-sensitive")
            break
    for j in range(12):  # more sums per topic, so that the rank thresholds have something to select from
        n = (64, 65, 129)[j % 3]
        add(tl[j % L], doc(n, list(rng.choice(min(n, 127), size=6, replace=False))))
    tokens = sum(sum(d.values()) for d in docs)
    nz = len(docs)
    need = 70 * (nz + 4) - tokens
    assert need >= 4
    for j in range(4):  # one-word documents of the plain word 1, cluster 0: bring avg to 70
        add(0, {1: need // 4 + (need % 4 if j == 3 else 0)})
    case = _csc(DTS_V, docs)
    # rank: past the two one-word documents of every catchword of the `both routes` topic (sums of avg), eighth among the test documents
    rank = 2 * sum(1 for w in range(DTS_V) if dts_catch_topic(w, k) == tl[3]) + 8
    case.update(k=1, topics=k, r=1, rank=rank, notes=notes, empty_topic=10)
    assert 10 not in tl and 10 not in want
    return _finish_post(case, want)


def edge_pairs(k, empty_topic=None):
    p = [(0, 0), (0, 1), (k - 1, 0), (1, k - 1), (k - 1, k - 1)]
    if empty_topic is not None:
        p.append((0, empty_topic))
    return np.array(p, np.int64)


def post_reference(case, r=None, rho=1.1, rank=None):
    """The plain reference of the whole downstream stage on a case (cached per argument set)."""
    r = case["r"] if r is None else r
    rank = case.get("rank", 1) if rank is None else rank
    key = ("post", id(case), r, rho, rank)
    if key not in _CACHE:
        k = case["topics"]
        thr, arms = ref_catch_thresholds(case["V"], case["rows"], case["offs"], case["nv"], case["cl"], k, r)
        ct = ref_find_catchwords(thr, rho)
        dts = ref_doc_topic_sums(case["rows"], case["offs"], case["nv"], ct, k)
        mthr = ref_model_thresholds(dts["dts_topic"], dts["dts_val"], k, rank)
        contribs = model_contributions(case["offs"], case["cl"], dts, mthr)
        model64, m = ref_model64(case["V"], case["rows"], case["offs"], case["nv"], contribs, k)
        _CACHE[key] = dict(thr=thr, arms=arms, catch_topic=ct, dts=dts, mthr=mthr, contribs=contribs, model64=model64, m=m)
    return _CACHE[key]
