"""The rule of isle_hip_score_docs (include/isle_hip.h; isle_amd/csrc/score_host.h) stated in numpy, with an exact reference per document in
mpmath, the table of cases the CPU and the GPU tests share, and the table of refusals with the texts they must carry.

A document d has a weight row (t_0 < t_1 < .., th_j) and entries (w, c); M is the model, V x k.
  th'_j   (double)th_j, with normalise (double)th_j / s_d, s_d = ((0.0 + th_0) + th_1) + ..; a row with s_d == 0 has no weights
  z       fma((double)M[w,t_j], th'_j, z) over j ascending from 0.0 (without normalise the product is exact: z + M th' is the same bits)
  class   z NaN, infinite or negative: unscored; else z < floor: scored at floor, counted in floored; else z == 0: unscored; else scored
  term    c log(z) ("log") or c z ("prob"), the product rounded once
  sums    lane i of 64 adds the terms of the entries i, i + 64, .. from 0.0; then p[i] = p[i] + p[i + s], s = 32 .. 1; p[0]
rule(..., wrong=...) computes a deliberately different rule, for the CPU test that shows the comparison of bits tells them apart."""
import math

import mpmath
import numpy as np

LANES = 64
LOG, PROB = 0, 1
FLOOR = 2.0 ** -40
# (measure, normalise, floor): what every case is run with
MODES = ((PROB, 0, 0.0), (PROB, 0, FLOOR), (LOG, 0, 0.0), (LOG, 1, FLOOR), (PROB, 1, 0.0))
WRONG = ("z_fp32", "descending", "sequential", "log_fp32", "no_normalise")
K_LOG_ULP = 4  # the device log's error: no accuracy table of the HIP math API is at hand; OpenCL's full-profile ceiling of 3 ulp for double log, + 1


class Case:
    def __init__(self, name, model, weights, entries):
        """model: (V, k) fp32; weights: (offs, topic, weight); entries: (counts, words, offs)"""
        self.name = name
        self.model = np.asfortranarray(model, np.float32)
        self.V, self.k = self.model.shape
        self.woff = np.ascontiguousarray(weights[0], np.int64)
        self.wtopic = np.ascontiguousarray(weights[1], np.uint32)
        self.wweight = np.ascontiguousarray(weights[2], np.float32)
        self.cnt = np.ascontiguousarray(entries[0], np.float32)
        self.word = np.ascontiguousarray(entries[1], np.uint32)
        self.off = np.ascontiguousarray(entries[2], np.int64)
        self.rows = self.off.size - 1
        assert self.woff.size - 1 == self.rows and self.woff[-1] == self.wtopic.size == self.wweight.size and self.off[-1] == self.cnt.size == self.word.size

    def weights_arg(self):
        return (self.woff, self.wtopic, self.wweight)

    def entries_arg(self):
        return (self.cnt, self.word, self.off)


def d2b(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def fma(a, b, c):
    """one fused multiply-add of doubles, exactly: the integers behind the three values, one correctly rounded division"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c  # (NaN and infinities go the same way fused and unfused)
    (n1, d1), (n2, d2), (n3, d3) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    num = n1 * n2 * d3 + n3 * d1 * d2
    if num == 0:
        return a * b + c  # (the sign of a zero result: every product and sum here is of values >= +0.0 or exact)
    return num / (d1 * d2 * d3)  # int / int is correctly rounded


def row_sum(w):
    s = np.float64(0.0)
    for x in w.astype(np.float64):
        s = s + x
    return float(s)


_Z = {}


def products(c, normalise, wrong=None):
    """z of every entry, in entry order (computed once per case and setting, and left unchanged)"""
    key = (id(c), bool(normalise), wrong if wrong in ("z_fp32", "descending", "no_normalise") else None)
    if key not in _Z:
        _Z[key] = (c, _products(c, normalise, wrong))  # (the case is kept alive with its products: the key is its id)
        _Z[key][1].setflags(write=False)
    return _Z[key][1]


def _products(c, normalise, wrong):
    z = np.zeros(c.cnt.size, np.float64)
    use_norm = bool(normalise) and wrong != "no_normalise"
    with np.errstate(all="ignore"):
        for r in range(c.rows):
            eb, ee = int(c.off[r]), int(c.off[r + 1])
            wb, we = int(c.woff[r]), int(c.woff[r + 1])
            if eb == ee:
                continue
            tp, w = c.wtopic[wb:we], c.wweight[wb:we]
            s = row_sum(w)
            if use_norm and s == 0.0:
                continue
            th = w.astype(np.float64) / np.float64(s) if use_norm else w.astype(np.float64)
            order = range(tp.size - 1, -1, -1) if wrong == "descending" else range(tp.size)
            words = c.word[eb:ee]
            if wrong == "z_fp32":
                acc = np.zeros(ee - eb, np.float32)
                for j in order:
                    acc = acc + c.model[words, tp[j]] * np.float32(th[j])
                z[eb:ee] = acc.astype(np.float64)
            elif not use_norm:
                acc = np.zeros(ee - eb, np.float64)
                for j in order:
                    acc = acc + c.model[words, tp[j]].astype(np.float64) * th[j]  # (an exact product: the same bits as the fused step)
                z[eb:ee] = acc
            else:
                cols = [c.model[words, tp[j]].astype(np.float64).tolist() for j in order]
                ths = [float(th[j]) for j in order]
                for i in range(ee - eb):
                    a = 0.0
                    for col, t in zip(cols, ths):
                        a = fma(col[i], t, a)
                    z[eb + i] = a
    return z


def classes(z, floor):
    """-> (at, scored mask, floored mask)"""
    with np.errstate(invalid="ignore"):
        dom = np.isfinite(z) & (z >= 0.0)
        floored = dom & (z < floor)
        scored = floored | (dom & ~floored & (z != 0.0))
    at = np.where(floored, np.float64(floor), np.where(scored, z, 0.0))
    return at, scored, floored


def fold(v, sequential=False):
    """the sum of one document's values in the stated order"""
    if sequential:
        s = np.float64(0.0)
        for x in v:
            s = s + x
        return s
    n = v.size
    pad = np.zeros(((n + LANES - 1) // LANES) * LANES, np.float64)
    pad[:n] = v
    p = np.zeros(LANES, np.float64)
    for row in pad.reshape(-1, LANES):
        p = p + row
    s = LANES // 2
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def rule(c, measure, normalise, floor, wrong=None):
    """-> dict(z, score, tokens, unscored_tokens as the bits of doubles (uint64); unscored_entries, floored uint32)"""
    z = products(c, normalise, wrong)
    at, scored, floored = classes(z, floor)
    cd = c.cnt.astype(np.float64)
    with np.errstate(all="ignore"):
        if measure == LOG:
            lg = np.log(np.where(scored, at, 1.0))
            if wrong == "log_fp32":
                lg = lg.astype(np.float32).astype(np.float64)
            term = np.where(scored, cd * lg, 0.0)
        else:
            term = np.where(scored, cd * at, 0.0)
    tok = np.where(scored, cd, 0.0)
    utok = np.where(scored, 0.0, cd)
    n = c.rows
    score, tokens, ut = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.float64)
    ue, fl = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    seq = wrong == "sequential"
    for r in range(n):
        sl = slice(int(c.off[r]), int(c.off[r + 1]))
        score[r], tokens[r], ut[r] = fold(term[sl], seq), fold(tok[sl], seq), fold(utok[sl], seq)
        ue[r], fl[r] = int((~scored[sl]).sum()), int(floored[sl].sum())
    return dict(z=d2b(z), score=d2b(score), tokens=d2b(tokens), unscored_tokens=d2b(ut), unscored_entries=ue, floored=fl)


FIELDS_EXACT = ("z", "tokens", "unscored_tokens", "unscored_entries", "floored")  # equal bit for bit in every mode; score too for PROB without normalise


def exact_log(c, z, floor):
    """per document the exact sum of c ln(z) over the scored entries (z: the rule's doubles, taken exactly) and the sum of c |ln z|, in
    mpmath at 200 bits; and the document's bound g / (1 - g) sum c |ln z|, g = (2 K + 1 + ceil(n / 64) + 6) 2^-53"""
    at, scored, _ = classes(z, floor)
    out = []
    with mpmath.workprec(200):
        for r in range(c.rows):
            ex, ab = mpmath.mpf(0), mpmath.mpf(0)
            for e in range(int(c.off[r]), int(c.off[r + 1])):
                if scored[e]:
                    t = mpmath.mpf(float(c.cnt[e])) * mpmath.log(mpmath.mpf(float(at[e])))
                    ex += t
                    ab += abs(t)
            n = int(c.off[r + 1] - c.off[r])
            g = mpmath.mpf(2 * K_LOG_ULP + 1 + (n + LANES - 1) // LANES + 6) * mpmath.mpf(2) ** -53
            out.append((ex, ab, g / (1 - g) * ab))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def _model(rs, V, k, zero_rows=()):
    m = (rs.random_sample((V, k)) ** 4).astype(np.float32) * np.float32(0.01) + np.float32(1e-7)
    m[rs.random_sample((V, k)) < 0.1] = 0.0
    for w in zero_rows:
        m[w, :] = 0.0
    return m


def _rows(rs, k, lengths, zero_rows=()):
    """weight rows of the given lengths: topics ascending strictly, weights of mixed magnitude"""
    off, tp, wt = [0], [], []
    for i, n in enumerate(lengths):
        t = np.sort(rs.choice(k, n, replace=False)) if n else np.zeros(0, np.int64)
        w = (rs.random_sample(n) ** 3).astype(np.float32) * np.float32(10.0 ** rs.randint(-3, 3))
        if i in zero_rows:
            w[:] = 0.0
        tp.extend(t.tolist())
        wt.extend(w.tolist())
        off.append(len(tp))
    return np.array(off, np.int64), np.array(tp, np.uint32), np.array(wt, np.float32)


def _entries(rs, V, lengths, words_of=None):
    """documents of the given lengths: words ascending within a document where V allows, else drawn with repeats (a caller's CSC may hold them)"""
    off, wd, ct = [0], [], []
    for n in lengths:
        w = np.sort(rs.choice(V, n, replace=False)) if n <= V else np.sort(rs.randint(0, V, n))
        wd.extend(w.tolist())
        ct.extend((rs.randint(1, 40, n) * (10.0 ** rs.randint(0, 4, n))).tolist())  # counts of mixed magnitude: the order of a sum shows
        off.append(len(wd))
    return np.array(ct, np.float32), np.array(wd, np.uint32), np.array(off, np.int64)


def _case(name, seed, V, k, doc_lengths, row_lengths, zero_model_rows=(), zero_weight_rows=(), nan_col=None):
    rs = np.random.RandomState(seed)
    m = _model(rs, V, k, zero_model_rows)
    if nan_col is not None:
        m[:, nan_col] = np.nan
    return Case(name, m, _rows(rs, k, row_lengths, zero_weight_rows), _entries(rs, V, doc_lengths))


def _cases():
    out = [
        # V = 1: every entry is word 0; k = 1; the last document empty
        _case("v1_k1", 1, 1, 1, [0, 1, 63, 64, 65, 129, 0], [1, 1, 1, 0, 1, 1, 1]),
        _case("v65_k3", 2, 65, 3, [1, 63, 64, 65, 129, 0, 5], [0, 1, 2, 3, 3, 3, 2]),
        _case("v65_k4", 3, 65, 4, [65, 64, 1, 129, 0], [4, 2, 4, 1, 4]),
        _case("v65_k5", 4, 65, 5, [129, 0, 63, 65, 64, 0], [5, 5, 2, 0, 1, 3]),
        # the long document: 4097 entries, 65 per lane; rows of k entries
        _case("v5000_k200_long", 5, 5000, 200, [4097, 1, 129, 65, 0], [5, 200, 2, 200, 1]),
        # the tile of 256 staged weights: rows of 255, 256, 257 and k = 1024 entries, documents of more than one round of 64
        _case("v5000_k1024_tiles", 6, 5000, 1024, [65, 64, 129, 65, 3, 0], [255, 256, 257, 1024, 0, 1]),
        # words absent from the model (their rows are zeros: z == 0), scored at the floor or unscored
        _case("absent_words", 7, 65, 5, [65, 64, 10, 0], [3, 5, 1, 2], zero_model_rows=range(0, 65, 3)),
        # a catch model with a NaN column (an empty cluster): rows 0 and 2 store topic 2, rows 1 and 3 do not
        Case("nan_column", _nan_model(), (np.array([0, 3, 5, 6, 8]), np.array([0, 2, 4, 1, 3, 2, 0, 1]),
                                            np.array([.5, .25, .25, .5, .5, 1., .125, .875], np.float32)),
             _entries(np.random.RandomState(8), 65, [65, 64, 7, 129])),
        # rows whose weights are all 0: no weights under normalise, z == 0 without
        _case("zero_rows", 9, 65, 4, [65, 3, 64, 1], [2, 4, 4, 0], zero_weight_rows=(1, 2)),
    ]
    return out


def _nan_model():
    m = _model(np.random.RandomState(8), 65, 5)
    m[:, 2] = np.nan
    return m


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------------------
def _probe_with(**kw):
    """the case v65_k3 with some of its arrays replaced"""
    c = BY_NAME["v65_k3"]
    a = dict(model=c.model, woff=c.woff.copy(), wtopic=c.wtopic.copy(), wweight=c.wweight.copy(), cnt=c.cnt.copy(), word=c.word.copy(), off=c.off.copy())
    for key, (i, v) in kw.items():
        a[key][i] = v
    return a


def _f32(x):
    return float(np.float32(x))


# (name, the arrays, the keywords of HotPath.score_docs, the text): refused before any launch
REFUSALS = [
    ("measure", _probe_with(), dict(measure=7), "score_docs: unknown measure 7"),
    ("normalise", _probe_with(), dict(normalise=2), "score_docs: normalise = 2, not 0 or 1"),
    ("floor_nan", _probe_with(), dict(floor=float("nan")), "score_docs: floor = nan, not finite and >= 0"),
    ("floor_negative", _probe_with(), dict(floor=-1.0), "score_docs: floor = -1, not finite and >= 0"),
    ("floor_infinite", _probe_with(), dict(floor=float("inf")), "score_docs: floor = inf, not finite and >= 0"),
    ("w_offsets_first", _probe_with(woff=(0, 1)), {}, "score_docs: w_offsets[0] = 1, not 0"),
    ("w_offsets_descend", _probe_with(woff=(3, 0)), {}, "score_docs: w_offsets descend at row 2"),
    ("offsets_first", _probe_with(off=(0, 1)), {}, "score_docs: offsets[0] = 1, not 0"),
    ("offsets_descend", _probe_with(off=(3, 10)), {}, "score_docs: offsets descend at row 2"),
]
# found on the device: the first offender named
FAULTS = [
    ("topic_out_of_range", _probe_with(wtopic=(2, 3)), "score_docs: weight entry 2 (row 2) has topic 3 >= num_topics 3"),
    ("topics_descend", _probe_with(wtopic=(4, 0)), "score_docs: weight entry 4 (row 3), topic 0: the topics of a row must ascend strictly"),
    ("weight_nan", _probe_with(wweight=(5, np.nan)), "score_docs: weight entry 5 (row 3) has weight nan: a weight is finite, >= 0 and < 2^31"),
    ("weight_negative", _probe_with(wweight=(1, -0.5)), "score_docs: weight entry 1 (row 2) has weight -0.5: a weight is finite, >= 0 and < 2^31"),
    ("weight_large", _probe_with(wweight=(8, 2.0 ** 31)), "score_docs: weight entry 8 (row 4) has weight 2.14748e+09: a weight is finite, >= 0 and < 2^31"),
    ("two_bad_weights", _probe_with(wweight=(7, np.inf), wtopic=(3, 9)), "score_docs: weight entry 3 (row 3) has topic 9 >= num_topics 3"),
    ("word_out_of_range", _probe_with(word=(70, 65)), "score_docs: entry 70 (document 2) has word 65 >= vocab 65"),
    ("count_negative", _probe_with(cnt=(0, -2.0)), "score_docs: entry 0 (document 0) has count -2: a count is finite and >= 0"),
    ("count_nan", _probe_with(cnt=(200, np.nan)), "score_docs: entry 200 (document 4) has count nan: a count is finite and >= 0"),
    ("two_bad_entries", _probe_with(cnt=(300, np.inf), word=(130, 4000000000)), "score_docs: entry 130 (document 3) has word 4000000000 >= vocab 65"),
    ("weight_before_entry", _probe_with(cnt=(0, -1.0), wweight=(8, -1.0)), "score_docs: weight entry 8 (row 4) has weight -1: a weight is finite, >= 0 and < 2^31"),
]


# ---- a small planted corpus: the resident sources, document completion, the shards ----------------------------------------------------------------
def planted(V, D, K, seed):
    """-> (model (V, K) fp32, columns sum to 1, every word possible under every topic; counts, words, offs of D documents drawn from
    mixtures of its topics, the last one empty)"""
    rs = np.random.RandomState(seed)
    m = np.full((V, K), 0.02 / V)
    for t in range(K):
        own = np.arange(t * (V // K), (t + 1) * (V // K))
        m[own, t] += 0.98 * rs.dirichlet(np.full(own.size, 0.3))
    m = (m / m.sum(0)).astype(np.float32)
    md = m.astype(np.float64)
    off, wd, ct = [0], [], []
    for d in range(D):
        p = md @ rs.dirichlet(np.full(K, 0.2))
        x = rs.multinomial(0 if d == D - 1 else int(rs.randint(5, 200)), p / p.sum())
        w = np.nonzero(x)[0]
        wd.extend(w.tolist())
        ct.extend(x[w].tolist())
        off.append(len(wd))
    return m, np.array(ct, np.float32), np.array(wd, np.uint32), np.array(off, np.int64)
