"""Plain rules, references and the case table for the corpus and model diagnostics (coherence.hip, corpus_stats.hip, avg_model.hip).
No GPU, no library: numpy and fractions only (the corpora that reach avg_topic_model reuse the builders of stages_certificate.py).

Every case aims at a constant of a kernel.  The constants are read out of the .hip sources below, so a case keeps its aim only as long as
test_diag_cases_cpu.py's reach assertions hold; a changed constant fails there instead of silently un-aiming a case.

u = 2^-24, u' = u / (1 - u) (fp32); v = 2^-53 (fp64); gamma64(n) = n v / (1 - n v) (Higham, Accuracy and Stability of Numerical Algorithms,
Lemma 3.1: a product of n factors (1 + d_i)^(+-1), |d_i| <= v, differs from 1 by at most gamma64(n)).

The average model (k_avg_model).  nv = avg * (count / doc_sum) in fp32 as post_normalize_k forms it.  With vmin = m 2^ex (frexp) every
value is a multiple of 2^(ex - 24), so q = nv 2^e, e = 24 - ex, is an integer; the device adds the two 32-bit halves of q with integer
atomics, hence S[w, t] = sum of q over the entries (w, d) of the documents d of cluster t and N[t] = sum_w S[w, t] are exact integers
whatever the order of arrival.
  bit-exact rule.  When N[t] < 2^53, am_value's hi 2^32 + lo is an exact integer in double, every partial sum of the norm reduction is an
    integer below 2^53 and therefore exact, and the result is the correctly rounded quotient cast once:
    m[w, t] = float32(float64(S) / float64(N)), to the bit.
  derived bound, for any N.  am_value makes at most three roundings (two conversions, one addition): s^ = S (1 + th3).  The norm adds V
    such values in a fixed tree, at most V - 1 additions on any path: N^ = N (1 + th(V + 2)).  The quotient is one rounding and the cast
    to float one fp32 rounding (or an absolute error below 2^-126 where the result is subnormal):
    m = (S / N) (1 + th64(3 + V + 2 + 1)) (1 + d32), so |m - S / N| <= (u + gamma64(V + 6) (1 + u)) S / N <= (u' + (V + 8) v) S / N + 2^-126
    for every V with (V + 6) v < 2^-20.  S / N is evaluated as a Fraction.
  An empty cluster has N = 0 and S = 0: 0 / 0 = NaN in every entry of the column.

Diversity (dv_mean_k, dv_dist_k) of a model with k' finite columns, reference in Fraction: abar_w = (1 / k') sum_t x[w, t],
dist_t = sum_w (x[w, t] - abar_w)^2.
  1. abar^_w: k' - 1 additions and one division of exactly converted floats: abar^_w = abar_w + eps_w, |eps_w| <= gamma64(k') |abar|_w,
     |abar|_w = (1 / k') sum_t |x[w, t]|.  With d_w = (k' + 1) v |abar|_w: |eps_w| <= rho d_w, rho = gamma64(k') / ((k' + 1) v) <= k' / (k' + 1) (1 + 2 k' v).
  2. One subtraction, one product: fl((x - abar^)^2) = (x - abar^)^2 (1 + th3).  The sum of V non-negative terms in a tree with at most V - 1
     additions on any path: dist^ = E (1 + th(V + 2)), E = sum_w (x_w - abar^_w)^2.
  3. sqrt(E) <= sqrt(dist) + ||eps||_2 and >= sqrt(dist) - ||eps||_2, so |E - dist| <= 2 sqrt(dist) ||eps|| + ||eps||^2.
  Together |dist^ - dist| <= gamma64(V + 2) dist + (1 + gamma64(V + 2)) (2 sqrt(dist) rho ||d|| + rho^2 ||d||^2)
                          <= gamma64(V + 3) dist + 2 sqrt(dist) ||d||_2 + ||d||_2^2,
  because (1 + gamma64(V + 2)) rho <= 1 whenever gamma64(V + 2) <= 1 / (2 k') (asserted: V <= 300, k' <= 8).  k' = 1: the division by 1 and the
  subtraction x - x are exact, so dist is 0 exactly.  k' = 0: 0 / 0, the average is NaN.  The average over the finite topics is formed on
  the host from the returned distances in ascending t, so it is a fixed function of them.

Edge top words: the column is fma(b, q, fl(a p)) entry for entry in fp32, a = float32(ratio), b = float32(1.0 - double(a)), rounded here
from the exact rational; hot_path.top_words is applied to it.
"""
import math
import os
import re
from fractions import Fraction

import numpy as np

import stages_certificate as sc
from stages_certificate import F

U32 = 2.0 ** -24
U_PRIME = U32 / (1.0 - U32)
V64 = 2.0 ** -53
TINY = 2.0 ** -126
WAVE = 64
MS = (2, 3, 5, 10, 20, 50, 100, 200, 500)
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "isle_amd", "csrc")


def gamma64(n):
    return n * V64 / (1.0 - n * V64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' constants, from their sources
# ---------------------------------------------------------------------------------------------------------------------------------
def _constants(file, names):
    with open(os.path.join(_CSRC, file)) as f:
        src = f.read()
    out = {}
    for name in names:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, "%s: no constexpr %s" % (file, name)
        expr = re.sub(r"(?<=\d)(ull|ul|u)\b", "", m.group(1).strip())
        assert re.fullmatch(r"[0-9\s*+\-()]+", expr), "%s: %s = %r is not plain integer arithmetic" % (file, name, expr)
        out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


COH = _constants("coherence.hip", ("CT", "HCAP", "COH_LDS", "COH_BITMAP_MAX_V"))
CS = _constants("corpus_stats.hip", ("LF_LDS_MAX", "CT"))
AM = _constants("avg_model.hip", ("AT",))
EXPECTED_CONSTANTS = dict(COH=dict(CT=1024, HCAP=256, COH_LDS=160 * 1024 - 512, COH_BITMAP_MAX_V=131072), CS=dict(LF_LDS_MAX=16384, CT=256),
                          AM=dict(AT=256))
AW = AM["AT"] // WAVE  # waves of tw_select_k: a wave's id range is ceil(V / AW)


def coh_uses_table(V):
    return V > COH["COH_BITMAP_MAX_V"]


def coh_tile(V):
    """Counters per pass of k_coherence_counts: what is left of the LDS after the bitmap, its prefix counts and the waves' hit lists."""
    nwords = 0 if coh_uses_table(V) else (V + 31) // 32
    return (COH["COH_LDS"] - (2 * nwords + (COH["CT"] // WAVE) * COH["HCAP"]) * 4) // 4


_CACHE = {}


def _cached(fn):
    def wrap(*a):
        key = (fn.__name__,) + a
        if key not in _CACHE:
            _CACHE[key] = fn(*a)
        return _CACHE[key]
    wrap.__name__ = fn.__name__
    return wrap


def build(spec):
    return spec[0](*spec[1:])


def csc_of_sets(V, docs):
    """Count matrix with count 1 from one collection of word ids per document (rows ascending within a document)."""
    offs, rows = [0], []
    for w in docs:
        w = np.unique(np.asarray(w, np.int64))
        assert w.size == 0 or (w[0] >= 0 and w[-1] < V)
        rows.append(w)
        offs.append(offs[-1] + w.size)
    rows = np.concatenate(rows).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    return dict(V=V, cnt=np.ones(rows.size, F), rows=rows, offs=np.array(offs, np.int64))


def csc_of_counts(V, docs):
    """Count matrix from one list of (word, count) per document, words ascending."""
    offs, rows, cnt = [0], [], []
    for d in docs:
        ws = [w for w, _ in d]
        assert ws == sorted(set(ws)) and (not ws or ws[-1] < V)
        rows += ws
        cnt += [c for _, c in d]
        offs.append(len(rows))
    return dict(V=V, cnt=np.array(cnt, F), rows=np.array(rows, np.uint32), offs=np.array(offs, np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# coherence
# ---------------------------------------------------------------------------------------------------------------------------------
def coh_plan(tw):
    """The counter space of k_coherence_counts: U (distinct words ascending), the distinct pairs of local ids sorted by (lo, hi) as a CSR
    keyed by lo.  -> dict(U, loc (n, M), pairs (nP, 2), part_off, nU, nP, N)."""
    tw = np.asarray(tw, np.int64)
    n, M = tw.shape
    U = np.unique(tw)
    loc = np.searchsorted(U, tw)
    keys = set()
    for i in range(1, M):
        for j in range(i):
            a, b = loc[:, i], loc[:, j]
            keys.update((np.minimum(a, b) * (1 << 32) + np.maximum(a, b)).tolist())
    keys = np.array(sorted(keys), np.int64)
    pairs = np.stack([keys >> 32, keys & 0xffffffff], axis=1) if keys.size else np.zeros((0, 2), np.int64)
    part_off = np.searchsorted(pairs[:, 0], np.arange(U.size + 1), "left")
    return dict(U=U, loc=loc, pairs=pairs, part_off=part_off, nU=int(U.size), nP=int(len(pairs)), N=int(U.size + len(pairs)))


def coh_hits(case):
    """Per document: the positions (entry index within the document) of the entries that are top words, and their local ids."""
    U = np.unique(np.asarray(case["tw"], np.int64))
    rows, offs = case["rows"].astype(np.int64), case["offs"]
    out = []
    for d in range(len(offs) - 1):
        r = rows[offs[d]:offs[d + 1]]
        at = np.searchsorted(U, r)
        hit = (at < U.size) & (U[np.minimum(at, U.size - 1)] == r)
        out.append((np.flatnonzero(hit), at[hit]))
    return out


COH_RULES = ("plain", "within-batch", "drop-beyond-hcap")


def coh_reference(case, rule="plain", eps=1e-5):
    """Set intersection per document, then the fp64 sum in the stated order (i ascending, then j ascending) with math.log.
    -> (coherence float64 (n,), doc_freq uint64 (n, M), co_doc_freq uint64 (n, M (M - 1) / 2)).
    Wrong rules: `within-batch` counts a pair only when both entries lie in the same 64-entry batch of the document (the compaction offset
    h forgotten between batches); `drop-beyond-hcap` counts pairs among a document's first HCAP hits only."""
    assert rule in COH_RULES
    tw = np.asarray(case["tw"], np.int64)
    n, M = tw.shape
    U = np.unique(tw)
    loc = np.searchsorted(U, tw)
    hits = coh_hits(case)
    D = len(hits)
    P = np.zeros((D, U.size), np.float32)
    groups = []  # the sets within which pairs are counted
    for d, (pos, ids) in enumerate(hits):
        P[d, ids] = 1
        if rule == "plain":
            groups.append(ids)
        elif rule == "within-batch":
            for b in np.unique(pos // WAVE):
                groups.append(ids[pos // WAVE == b])
        else:
            groups.append(ids[:COH["HCAP"]])
    Q = np.zeros((len(groups), U.size), np.float32)
    for g, ids in enumerate(groups):
        Q[g, ids] = 1
    df = P.sum(axis=0).astype(np.uint64)[loc]
    Qt = Q[:, loc]                                                        # (groups, n, M)
    G = np.matmul(Qt.transpose(1, 2, 0), Qt.transpose(1, 0, 2))            # (n, M, M): counts below 2^24, exact in fp32
    ii = np.array([i for i in range(1, M) for j in range(i)], np.int64)
    jj = np.array([j for i in range(1, M) for j in range(i)], np.int64)
    co = G[:, ii, jj].astype(np.uint64) if ii.size else np.zeros((n, 0), np.uint64)
    coh = np.empty(n, np.float64)
    for t in range(n):
        s, undefined = 0.0, False
        for p in range(ii.size):
            dij, dj = int(co[t, p]), int(df[t, jj[p]])
            if dj == 0:
                undefined = True
                continue
            s += math.log(float(dij) + eps) - math.log(float(dj))
        coh[t] = math.nan if undefined else s
    return coh, df, co


COH_HITS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 300)
COH_NU = 320


@_cached
def coh_hits_case(V):
    """Two documents per hit count h of COH_HITS: the first h and the last h of 320 top words spread over the vocabulary (the last is word
    V - 1), each with 36 other words in between, and an empty document.  Ten topics of 32 words, topic t = U[t::10], so that the words of a
    topic are spread over every 64-entry batch of a document."""
    U = np.unique(np.linspace(3, V - 1, COH_NU).astype(np.int64))
    assert U.size == COH_NU and U[-1] == V - 1
    inU = set(U.tolist())
    miss = [int(w) + 1 for w in U[::9] if int(w) + 1 not in inU and int(w) + 1 < V]
    docs, want = [], []
    for h in COH_HITS:
        for part in (U[:h], U[U.size - h:]):
            docs.append(np.concatenate([part, miss]))
            want.append(h)
    docs.append([])
    want.append(0)
    case = csc_of_sets(V, docs)
    case.update(tw=np.stack([U[t::10] for t in range(10)]).astype(np.uint32), want_hits=want, nmiss=len(miss))
    return case


# (V, topics, M, shared words): N = nU + nP against coh_tile(V)
COH_TILE_SPECS = {
    "tile-exact": (4864, 69, 32, 0),      # N == tile: one full pass
    "tile-plus-1": (4896, 69, 32, 1),     # N == tile + 1: a second pass of one counter
    "cut-at-nU": (34592, 17287, 2, 0),    # nU == tile: the second pass starts exactly at the first pair counter
    "words-only": (40000, 1200, 32, 0),   # nU > tile: a pass of word counters only, then a mixed one, then pairs
}


@_cached
def coh_tile_case(name):
    V, T, M, shared = COH_TILE_SPECS[name]
    rng = np.random.default_rng(len(name) * 1000 + T)
    tw = rng.permutation(V)[:T * M].reshape(T, M).astype(np.int64)
    for s in range(shared):
        tw[s + 1, 0] = tw[0, 0]          # one distinct word fewer, the pairs stay distinct
    D = 200
    docs = []
    if M == 2:
        for d in range(D):               # about 90 whole topics per document, overlapping with the neighbours
            t0 = (d * 86) % T
            ts = (t0 + np.arange(90)) % T
            docs.append(np.concatenate([tw[ts].ravel(), tw[rng.integers(0, T, 20), 0]]))
    else:
        per = max(T // D, 1)
        for d in range(D):               # some whole topics, half of another, a few stray top words
            ts = (d * per + np.arange(12 if d % 40 == 0 else min(per, 6))) % T   # every 40th: more hits than a wave's list holds
            half = tw[(7 * d + 3) % T, ::2]
            docs.append(np.concatenate([tw[ts].ravel(), half, tw[rng.integers(0, T, 8), rng.integers(0, M, 8)]]))
    case = csc_of_sets(V, docs)
    case.update(tw=tw.astype(np.uint32))
    return case


def coherence_cases():
    out = {"hits-%d" % V: (coh_hits_case, V) for V in (2000, 131072, 131073)}
    out.update({"bitmap-tail-%d" % (V % 32): (coh_hits_case, V) for V in (1985, 2015)})
    out.update({name: (coh_tile_case, name) for name in COH_TILE_SPECS})
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# log-combinatorial
# ---------------------------------------------------------------------------------------------------------------------------------
def log_fact(nmax):
    """src/sparseMatrix.cpp:1032-1034: log_fact[i + 1] = (float)((double)log_fact[i] + log(i + 1))."""
    lf = np.zeros(nmax + 1, F)
    x = 0.0
    for i in range(nmax):
        x = float(F(x + math.log(i + 1)))
        lf[i + 1] = x
    return lf


def doc_words(case):
    ci = case["cnt"].astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(ci)])
    return cs[case["offs"][1:]] - cs[case["offs"][:-1]]


LC_RULES = ("plain", "clamp-index")


def log_comb_reference(case, rule="plain"):
    """The element-wise fp32 walk, one document after the other.  `clamp-index`: every table index clamped at LF_LDS_MAX - 1 (a table that
    stayed in LDS one entry too long)."""
    assert rule in LC_RULES
    N = doc_words(case)
    lf = log_fact(int(N.max()) if N.size else 0)
    top = CS["LF_LDS_MAX"] - 1 if rule == "clamp-index" else len(lf) - 1
    ci, offs = case["cnt"].astype(np.int64), case["offs"]
    out = np.zeros(len(N), F)
    for d in range(len(N)):
        acc = F(0)
        for c in ci[offs[d]:offs[d + 1]]:
            acc = F(acc - lf[min(int(c), top)])
        out[d] = F(acc + lf[min(int(N[d]), top)])
    return out


def _pseudo_counts(n, seed, hi=9):
    return (np.random.default_rng(seed).integers(1, hi + 1, n)).tolist()


@_cached
def lc_case(name):
    small = [[(1, 2), (4, 3)], [(0, 1)], [], [(2, 5), (3, 1), (7, 2)]]
    if name == "lds-last":      # nlf == LF_LDS_MAX: the last table read from LDS, T[N_d] its last entry
        docs = [[(0, 16383)], [(1, 16000), (2, 383)], [(0, 16382), (5, 1)]] + small
    elif name == "hbm-first":   # nlf == LF_LDS_MAX + 1: the first table read from HBM
        docs = [[(0, 16384)], [(0, 16383), (1, 1)], [(0, 8192), (3, 8192)]] + small
    elif name == "wave-sum":    # documents of 0, 1, 63, 64, 65 entries: the wave sum of cs_doc_words_k
        docs = [[(w, c) for w, c in enumerate(_pseudo_counts(n, n))] for n in (0, 1, 63, 64, 65, 0, 64)]
    else:
        assert name == "refuse"  # one entry of count 2^31: N_d is above the reference's int index
        docs = [[(0, 2 ** 31)], [(1, 3), (2, 4)]]
    return csc_of_counts(70, docs)


def log_comb_cases():
    return {name: (lc_case, name) for name in ("lds-last", "hbm-first", "wave-sum")}


# ---------------------------------------------------------------------------------------------------------------------------------
# distinct top-five sets
# ---------------------------------------------------------------------------------------------------------------------------------
def normalised(case):
    avg, _, _ = sc.corpus_avg(case["cnt"], case["offs"])
    return sc.ref_normalize(case["cnt"], case["offs"], avg)


def lane_top5(vals, keep=5, pop_all=False):
    """cs_top5_k's own scheme on one document's values (uint32 bit patterns): a descending top `keep` per lane (lane = entry index mod 64),
    then five rounds of a wave-wide maximum whose lowest holder pops its head.  keep = 5 and pop_all = False is the kernel; keep = 4 and
    pop_all = True (every holder pops) are the wrong rules."""
    lanes = [sorted((int(v) for v in vals[l::WAVE]), reverse=True)[:keep] for l in range(WAVE)]
    lanes = [a + [0] * (5 - len(a)) for a in lanes]
    out = []
    for _ in range(5):
        m = max(a[0] for a in lanes)
        holders = [l for l in range(WAVE) if lanes[l][0] == m]
        for l in (holders if pop_all else holders[:1]):
            lanes[l] = lanes[l][1:] + [0]
        out.append(m)
    return out


T5_RULES = ("plain", "lanes", "lane-top-4", "pop-all-holders", "last-run-1")


def top5_reference(case, rule="plain"):
    """Every qualifying document's values sorted descending, the first five; the tuples lexsorted; the run lengths of equal tuples; the
    counts by test_corpus_stats_cpu.literal (applied by the caller: run ids are returned).
    -> dict(tuples float32 (n, 5), runs list, run_ids list)."""
    assert rule in T5_RULES
    nv = normalised(case).view(np.uint32)
    offs = case["offs"]
    T = []
    for d in range(len(offs) - 1):
        v = nv[offs[d]:offs[d + 1]]
        if v.size < 5:
            continue
        if rule in ("plain", "last-run-1"):
            T.append(np.sort(v)[::-1][:5].tolist())
        else:
            T.append(lane_top5(v, keep=4 if rule == "lane-top-4" else 5, pop_all=rule == "pop-all-holders"))
    T = np.array(T, np.uint32).reshape(-1, 5)
    T = T[np.lexsort((T[:, 4], T[:, 3], T[:, 2], T[:, 1], T[:, 0]))]      # positive floats: the bit patterns order as the values
    run_ids = np.concatenate([[0], np.cumsum(np.any(T[1:] != T[:-1], axis=1))]).tolist() if len(T) else []
    runs = np.bincount(run_ids).tolist() if len(T) else []
    if rule == "last-run-1" and runs:
        runs[-1] = 1
    return dict(tuples=T.view(F), runs=runs, run_ids=run_ids)


T5_LENGTHS = (4, 5, 63, 64, 65, 320, 321)
T5_ONE_LANE = 37


@_cached
def t5_lanes_case():
    """Documents of 4 .. 321 entries with small counts (many ties), and three planted ones: the five largest values in one lane; five equal
    maxima in five lanes; six equal maxima in two lanes."""
    docs, plant = [], {}
    for n in T5_LENGTHS:
        docs.append([(w, c) for w, c in enumerate(_pseudo_counts(n, 100 + n, 50))])
    c = _pseudo_counts(330, 7, 50)
    pos = [T5_ONE_LANE + WAVE * j for j in range(5)]
    for j, p in enumerate(pos):
        c[p] = 200 + j
    plant["one-lane"] = (len(docs), pos)
    docs.append(list(enumerate(c)))
    c = _pseudo_counts(200, 8, 50)
    pos = [3, 68, 133, 198, 199]
    for p in pos:
        c[p] = 90
    plant["five-equal"] = (len(docs), pos)
    docs.append(list(enumerate(c)))
    c = _pseudo_counts(200, 9, 50)
    pos = [10, 74, 138, 11, 75, 139]
    for p in pos:
        c[p] = 90
    plant["six-in-two"] = (len(docs), pos)
    docs.append(list(enumerate(c)))
    case = csc_of_counts(400, docs)
    case.update(plant=plant)
    return case


T5_RUN_SPECS = {  # qualifying documents -> (first position of the long run or None, its length)
    255: (None, 0), 256: (None, 0), 257: (None, 0), 300: (250, 11),
}


@_cached
def t5_runs_case(n):
    """n qualifying documents of five entries; type i has the counts (i + 10, 1, 1, 1, 1), so the tuples ascend with i.  Every type once,
    except: the long run of T5_RUN_SPECS, and the last type three times (a run that ends at the last sorted position)."""
    at, length = T5_RUN_SPECS[n]
    mult, total = [], 0
    while total < n - 3:
        m = length if at is not None and total == at else 1
        mult.append(m)
        total += m
    assert total == n - 3
    mult.append(3)
    docs = []
    for i, m in enumerate(mult):
        docs += [[(0, i + 10), (1, 1), (2, 1), (3, 1), (4, 1)]] * m
    docs += [[(0, 3), (1, 2)], []] * 2                                      # not qualifying
    order = np.random.default_rng(n).permutation(len(docs))
    case = csc_of_counts(8, [docs[i] for i in order])
    case.update(mult=mult)
    return case


def top_five_cases():
    out = {"lanes": (t5_lanes_case,)}
    out.update({"runs-%d" % n: (t5_runs_case, n) for n in T5_RUN_SPECS})
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the average model
# ---------------------------------------------------------------------------------------------------------------------------------
def _avg_case(V, docs, want, topics, exact, avg=None, fill_word=None, nz=None, fill_cluster=0):
    if avg is not None:
        before = len(docs)
        sc._pad_to_avg(docs, fill_word, avg, nz)
        want = list(want) + [fill_cluster] * (len(docs) - before)
    case = sc._csc(V, docs)
    case.update(k=1, topics=topics, r=1, exact=exact)
    return sc._finish_post(case, want)


@_cached
def avg_case(name):
    """Hand-built corpora through stages_certificate's builders (thresholded by the plain reference, every kept document with a known
    cluster).  A single-word document has the normalised value avg whatever its count; a count c in a document of sum S has avg c / S."""
    if name == "hi-half":
        # avg = 64: values from 64 / 3000 to 64, vmax / vmin = 3000 in [2^9, 2^12]; e = 29, so every value >= 8 has q >= 2^32
        docs, want = [], []
        for d in ({5: 7, 9: 3, 100: 54}, ):
            docs.append(d), want.append(1)                                  # a cluster of one document
        for n, big in ((63, 38), (64, 67), (65, 33)):                       # documents of 63, 64, 65 entries, sums 100, 130, 97
            d = {w: 1 for w in range(n)}
            d[n // 2] = big
            docs.append(d), want.append(2)
        for d in ({0: 1, 1: 1023}, {2: 3, 3: 1500, 4: 33}, {7: 1, 8: 2999}, {0: 11, 3: 13, 8: 17, 60: 1}):
            docs.append(d), want.append(4)
        for d in ({0: 5, 1: 2, 61: 30}, {1: 9, 62: 1, 63: 20, 64: 7}, {0: 21, 64: 100}):
            docs.append(d), want.append(0)
        for _ in range(2):                                                  # 129 equal counts round to 0 everywhere: outside B
            docs.append({w: 1 for w in range(129)}), want.append(-1)
        return _avg_case(200, docs, want, topics=5, exact=True, avg=64, fill_word=199, nz=150)      # cluster 3 stays empty
    if name == "beyond-2^53":
        # avg = 2^15; one document holds the count 3 in a sum S just below 2^23, so vmin = 2^15 fl(3 / S) and e = 30; 280 single-word
        # documents of word 0 (value 2^15, q = 2^45) bring the total of column 0 above 2^53, and vmin's odd q makes it unrepresentable
        c = 3
        S = next(S for S in range(2 ** 23 - 1, 2 ** 23 - 200, -2) if int(math.ldexp(math.frexp(float(F(c) / F(S)))[0], 24)) & 1)
        docs = [{0: 1 + i % 7} for i in range(280)] + [{0: c, 1: S - c}]
        want = [0] * 281
        return _avg_case(4, docs, want, topics=2, exact=False, avg=2 ** 15, fill_word=2, nz=340, fill_cluster=1)
    if name == "one-topic":
        docs = [{0: 3, 1: 5}, {2: 8}, {0: 1, 3: 2, 4: 5}, {1: 1, 2: 1, 3: 1}]
        return _avg_case(5, docs, [0] * 4, topics=1, exact=True, avg=8, fill_word=4, nz=9)
    assert name == "one-word"
    docs = [{0: c} for c in (1, 5, 9, 2, 2, 7)]
    return _avg_case(1, docs, [0] * 6, topics=2, exact=True)


AVG_CASES = ("hi-half", "beyond-2^53", "one-topic", "one-word")


def avg_scale(nv):
    """-> e of k_avg_model: vmin = m 2^ex, e = 24 - ex."""
    _, ex = math.frexp(float(nv.min()))
    return 24 - ex


AVG_RULES = ("exact", "drop-hi")


def avg_reference(case, rule="exact"):
    """Exact integer sums.  -> dict(e, q (python ints), n_hi (entries with q >= 2^32), S (V x k python ints), N (k), exact (every N < 2^53),
    sizes (documents per cluster), model (float32 (V, k): the bit-exact expectation; meaningful where exact)).
    `drop-hi`: the high 32 bits of every q are lost."""
    assert rule in AVG_RULES
    V, k, nv, cl, offs = case["V"], case["topics"], case["nv"], case["cl"], case["offs"]
    rows = case["rows"].astype(np.int64)
    e = avg_scale(nv)
    q = [int(math.ldexp(float(x), e)) for x in nv]
    assert all(math.ldexp(float(x), e) == qi for x, qi in zip(nv, q)) and min(q) >= 2 ** 23 and max(q) < 2 ** 64
    S = [[0] * k for _ in range(V)]
    for d in range(len(offs) - 1):
        if cl[d] < 0:
            continue
        for i in range(offs[d], offs[d + 1]):
            S[rows[i]][cl[d]] += q[i] & 0xffffffff if rule == "drop-hi" else q[i]
    N = [sum(S[w][t] for w in range(V)) for t in range(k)]
    model = np.full((V, k), np.nan, F)
    for t in range(k):
        if N[t]:
            model[:, t] = (np.array([np.float64(S[w][t]) for w in range(V)]) / np.float64(N[t])).astype(F)
    return dict(e=e, q=q, n_hi=sum(1 for x in q if x >= 2 ** 32), S=S, N=N, exact=all(n < 2 ** 53 for n in N),
                sizes=np.bincount(cl[cl >= 0], minlength=k), model=model)


def avg_fp32_in_document_order(case):
    """The wrong rule of an fp32 accumulator: nv added per (word, topic) in document order, the norm in word order, one fp32 quotient."""
    V, k, nv, cl, offs = case["V"], case["topics"], case["nv"], case["cl"], case["offs"]
    rows = case["rows"].astype(np.int64)
    S = np.zeros((V, k), F)
    for d in range(len(offs) - 1):
        if cl[d] >= 0:
            for i in range(offs[d], offs[d + 1]):
                S[rows[i], cl[d]] = F(S[rows[i], cl[d]] + nv[i])
    out = np.full((V, k), np.nan, F)
    for t in range(k):
        n = F(0)
        for w in range(V):
            n = F(n + S[w, t])
        if n > 0:
            out[:, t] = S[:, t] / n
    return out


def avg_bound_ratio(M, ref, V):
    """max over the entries of non-empty clusters of |m - S / N| / ((u' + (V + 8) v) S / N + 2^-126), with S / N as a Fraction."""
    rel = Fraction(U_PRIME) + (V + 8) * Fraction(V64)
    worst = 0.0
    for t, n in enumerate(ref["N"]):
        if n == 0:
            continue
        for w in range(V):
            m = float(M[w, t])
            assert math.isfinite(m), "entry (%d, %d) of a non-empty cluster is %r" % (w, t, m)
            x = Fraction(ref["S"][w][t], n)
            worst = max(worst, float(abs(Fraction(m) - x) / (rel * x + Fraction(TINY))))
    return worst


def certify_avg(M, case, ref):
    """-> dict(mode, ratio).  The NaN pattern exactly; bit equality where every total is below 2^53 (and the bound as well: the two
    statements are consistent), else the derived bound."""
    M = np.asarray(M)
    assert M.dtype == np.float32 and M.shape == (case["V"], case["topics"])
    empty = np.array([n == 0 for n in ref["N"]])
    assert np.array_equal(np.isnan(M), np.broadcast_to(empty, M.shape)), "NaN exactly in the columns of empty clusters"
    ratio = avg_bound_ratio(M, ref, case["V"])
    assert ratio <= 1.0, "error / bound %.4g" % ratio
    if ref["exact"]:
        bad = np.argwhere(M.view(np.uint32)[:, ~empty] != ref["model"].view(np.uint32)[:, ~empty])
        assert bad.size == 0, "%d entries differ from float32(S / N) in their bits, first %s" % (len(bad), bad[0])
    return dict(mode="bits" if ref["exact"] else "bound", ratio=ratio)


# ---------------------------------------------------------------------------------------------------------------------------------
# top words
# ---------------------------------------------------------------------------------------------------------------------------------
def round_f32(x):
    """A Fraction rounded to float32, to nearest, ties to even, subnormals kept."""
    if x == 0:
        return F(0.0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(a, quantum)
    n = int(n)
    if rem * 2 > quantum or (rem * 2 == quantum and n & 1):
        n += 1
    out = s * float(n * quantum)
    assert abs(out) < 2.0 ** 128
    return F(out)


def edge_columns(M, pairs, ratio):
    """fma(b, M[w, q], fl(a M[w, p])) entry for entry, for finite models.  -> float32 (V, n_edge)."""
    a, b = sc.edge_coefficients(ratio)
    M = np.asarray(M, F)
    out = np.empty((M.shape[0], len(pairs)), F)
    for e, (p, q) in enumerate(pairs):
        y = (a * M[:, p]).astype(F)
        for w in range(M.shape[0]):
            out[w, e] = round_f32(Fraction(float(b)) * Fraction(float(M[w, q])) + Fraction(float(y[w])))
    return out


def top_words_highest_id(M, n):
    """The wrong rule: among equal weights the higher id first."""
    W = np.where(np.isnan(M), -np.inf, M)
    out = np.empty((M.shape[1], n), np.uint32)
    for t in range(M.shape[1]):
        out[t] = np.lexsort((-np.arange(M.shape[0]), -W[:, t]))[:n]
    return out


TW_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)


@_cached
def tw_size_case(V):
    rng = np.random.default_rng(V)
    M = np.empty((V, 6), F)
    M[:, 0] = rng.random(V, dtype=F)
    M[:, 1] = rng.integers(0, 4, V).astype(F) / 4
    M[:, 2] = 0.25
    M[:, 3] = np.arange(V, 0, -1, dtype=F) / V
    M[:, 4] = np.arange(1, V + 1, dtype=F) / V
    M[:, 5] = rng.random(V, dtype=F)
    M[::3, 5] = np.nan
    return dict(M=M, ns=sorted({1, min(V, 32)}))


@_cached
def tw_ties_case():
    """V = 1024: a wave's range is 256 ids.  Column 0: five words of 0.9 and four of 0.5 at ids 254 .. 257 (n = 8 needs three of them: two of
    wave 0's range and one of wave 1's).  Column 1: 40 words of 0.5 in wave 0's range and two of 0.9 (n = 5 needs three of the 40).
    Column 2: every word 0.25.  Column 3: ties in the ranges of waves 2 and 3 only."""
    V = 1024
    rng = np.random.default_rng(1024)
    M = (rng.random((V, 4), dtype=F) * F(0.4)).astype(F)
    M[[10, 300, 600, 900, 1023], 0] = 0.9
    M[254:258, 0] = 0.5
    M[0:80:2, 1] = 0.5
    M[[500, 700], 1] = 0.9
    M[:, 2] = 0.25
    M[[600, 800, 801], 3] = 0.5
    M[5, 3] = 0.9
    return dict(M=M, ns=[1, 3, 5, 8, 32])


@_cached
def tw_keys_case():
    """tw_key's special values, V = 70 (ranges of 18 ids, the last one shorter)."""
    V = 70
    rng = np.random.default_rng(70)
    nnan = np.array([0xffc00000], np.uint32).view(F)[0]
    M = np.empty((V, 6), F)
    M[:, 0] = np.nan                                   # fewer than n non-NaN entries
    M[[3, 40, 41, 69], 0] = [0.5, 0.25, 0.25, 1.0]
    M[:, 1] = np.where(np.arange(V) % 2 == 0, F(-0.0), F(0.0))   # -0 and +0 mixed, negatives below them
    M[10:20, 1] = -1.0
    M[:, 2] = 0.0                                      # subnormals around zero
    M[[7, 8, 30, 31, 50], 2] = [1e-40, -1e-40, 1e-45, -1e-45, 2.0 ** -126]
    M[:, 3] = rng.random(V, dtype=F)                   # infinities and both NaNs among finite weights
    M[[2, 20], 3] = np.inf
    M[[4, 33], 3] = -np.inf
    M[5, 3] = np.nan
    M[6, 3] = nnan
    M[:, 4] = -np.inf                                  # -inf and NaN share the lowest key
    M[1::2, 4] = np.nan
    M[9, 4] = nnan
    M[:, 5] = -rng.random(V, dtype=F)                  # all negative
    return dict(M=M, ns=[1, 32])


EDGE_PAIRS = ((0, 1), (1, 0), (2, 3), (0, 0), (3, 1))
EDGE_RATIOS = (0.7, 1.0)
EDGE_TIE_WORDS = (17, 90)


@_cached
def tw_edge_case():
    """A 4-column model of 130 words.  Words 17 and 90 hold different entries in columns 0 and 1 but the same edge weight for the pair (0, 1)
    under both ratios, the largest of the column: under 1.0 the edge is column 0 itself (equal there, different in column 1), under 0.7 word
    90's column-1 entry is searched so that the fused multiply-add rounds to word 17's weight."""
    V = 130
    rng = np.random.default_rng(130)
    M = (rng.random((V, 4), dtype=F) * F(0.2)).astype(F)
    lo, hi = EDGE_TIE_WORDS
    M[lo, 0], M[lo, 1] = 0.5, 0.25
    return dict(M=M, ns=[1, 10, 32], V=V, lo=lo, hi=hi)


def edge_model(ratio):
    """The model of the edge case for one ratio (the searched entry depends on the ratio)."""
    key = ("edge_model", ratio)
    if key in _CACHE:
        return _CACHE[key]
    base = tw_edge_case()
    M = base["M"].copy()
    lo, hi = base["lo"], base["hi"]
    a, b = sc.edge_coefficients(ratio)
    target = edge_columns(M[[lo]], [(0, 1)], ratio)[0, 0]
    if float(b) == 0.0:
        M[hi, 0], M[hi, 1] = M[lo, 0], 0.125
    else:
        M[hi, 0] = 0.375
        y = F(a * M[hi, 0])
        q = F((float(target) - float(y)) / float(b))
        found = None
        for step in range(-64, 65):
            cand = q
            for _ in range(abs(step)):
                cand = np.nextafter(cand, F(np.inf) if step > 0 else F(-np.inf))
            if round_f32(Fraction(float(b)) * Fraction(float(cand)) + Fraction(float(y))) == target:
                found = cand
                break
        assert found is not None, "no column-1 entry makes the fma tie"
        M[hi, 1] = found
    _CACHE[key] = M
    return M


def top_words_cases():
    out = {"size-%d" % V: (tw_size_case, V) for V in TW_SIZES}
    out["ties"] = (tw_ties_case,)
    out["keys"] = (tw_keys_case,)
    return out


def tie_ranges(col, n):
    """-> (K weight, r ties needed, the wave range of every id whose weight equals the n-th largest), NaN as -inf."""
    w = np.where(np.isnan(col), -np.inf, col).astype(np.float64)
    K = np.sort(w)[::-1][n - 1]
    per = -(-len(col) // AW)
    ids = np.flatnonzero(w == K)
    return K, n - int((w > K).sum()), (ids // per).tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# diversity
# ---------------------------------------------------------------------------------------------------------------------------------
INF_TOKEN = b"9" * 45   # the loader accumulates the digits in fp32: forty-five nines overflow to +inf


def _sixtyfourths(V, k, seed):
    return (np.random.default_rng(seed).integers(0, 4 * 64, (V, k)).astype(F) / F(64)).astype(F)


@_cached
def div_case(name):
    """Models of multiples of 1 / 64 (six decimals print them exactly), loaded as dense text."""
    if name == "no-finite-topic":
        M = _sixtyfourths(6, 2, 1)
        M[2, 0] = np.nan
        M[5, 1] = np.nan
    elif name == "one-finite-topic":
        M = _sixtyfourths(6, 3, 2)
        M[0, 0] = np.nan
        M[3, 2] = np.inf
    elif name == "one-inf":
        M = _sixtyfourths(10, 4, 3)
        M[9, 1] = np.inf
    else:
        V = int(name.split("-")[1])
        M = _sixtyfourths(V, 5, V)
    return dict(M=M, V=M.shape[0], k=M.shape[1])


DIV_CASES = ("no-finite-topic", "one-finite-topic", "one-inf", "block-255", "block-256", "block-257")


def dense_text(M):
    def tok(x):
        if np.isnan(x):
            return b"nan"
        if np.isinf(x):
            assert x > 0
            return INF_TOKEN
        s = b"%.6f" % float(x)
        assert float(s) == float(x)
        return s
    return b"".join(b"\t".join(tok(x) for x in M[:, t]) + b"\t\n" for t in range(M.shape[1]))


def diversity_reference(M):
    """In Fraction.  -> dict(finite (k,) bool, kp, dist (k floats, NaN where not finite: the nearest doubles), bound (k floats), exact (k Fractions or None))."""
    M = np.asarray(M)
    V, k = M.shape
    fin = np.isfinite(M).all(axis=0)
    kp = int(fin.sum())
    assert V <= 300 and kp <= 8 and gamma64(V + 2) <= 1.0 / (2 * max(kp, 1))
    dist, bound, exact = np.full(k, np.nan), np.full(k, np.nan), [None] * k
    if kp:
        X = [[Fraction(float(M[w, t])) for t in range(k) if fin[t]] for w in range(V)]
        abar = [sum(r) / kp for r in X]
        aabs = [sum(abs(x) for x in r) / kp for r in X]
        d2 = sum(((kp + 1) * Fraction(V64) * a) ** 2 for a in aabs)
        dn = math.sqrt(float(d2)) * (1 + 4 * V64)                      # rounded up
        col = 0
        for t in range(k):
            if not fin[t]:
                continue
            ex = sum((X[w][col] - abar[w]) ** 2 for w in range(V))
            col += 1
            exact[t] = ex
            dist[t] = float(ex)
            bound[t] = gamma64(V + 3) * float(ex) + 2 * math.sqrt(float(ex)) * (1 + 4 * V64) * dn + dn * dn
    return dict(finite=fin, kp=kp, dist=dist, bound=bound, exact=exact)


def certify_diversity(got, ref):
    """-> the largest error / bound (0 where both are 0)."""
    fin, kp = ref["finite"], ref["kp"]
    dist = np.asarray(got["dist"], np.float64)
    assert np.array_equal(np.isnan(dist), ~fin), "NaN exactly for the topics with a non-finite entry"
    worst = 0.0
    for t in np.flatnonzero(fin):
        err = abs(Fraction(float(dist[t])) - ref["exact"][t])
        if kp == 1:
            assert dist[t] == 0.0, "one finite topic is its own mean"
        if err:
            assert ref["bound"][t] > 0 and float(err) <= ref["bound"][t], "topic %d: error %.4g, bound %.4g" % (t, float(err), ref["bound"][t])
            worst = max(worst, float(err) / ref["bound"][t])
    if kp == 0:
        assert math.isnan(got["avg"])
    else:
        s = 0.0
        for t in np.flatnonzero(fin):
            s += float(dist[t])
        assert got["avg"] == s / kp, "the average is the host's sum of the returned distances in ascending t over k'"
    return worst
