"""fp64 certificates of the multiplicative-weights inference isle_hip_infer (infer.hip), topic by topic (no GPU; numpy only).

The operation.  One document with kept rows R (n x k, the fp32 model rows whose double sum is > 1e-10), a = count / sum(counts) over
all of the document's words (dropped ones included), weights w.  Step `it` (0-based) is

    z = R w,   g = R^T (a / z),   eta = sqrt(2 float32(log(float32(k))) / (it + 1)) / Lf,   e = eta g,
    w'_t = w_t exp(e_t) / N,   N = sum_s w_s exp(e_s).

All inputs are >= 0: every sum is of like-signed terms, so every bound below is relative and holds for any order and any tree of the
sums, with or without FMA.  u = 2^-24, u' = u / (1 - u); a product of m factors (1 + d_i)^(+-1), |d_i| <= u, lies in exp(+- m u')
(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1, in its exponential form).

certify_step: |w'^_t - w'_t| <= rel[t] w'_t + 2^-126 with

    rel[t] = ((e_t + sum_s w'_s e_s) (k + n + C1) + k + C2) u (1 + 2^-3),   C1 = 8, C2 = 3,

w' the fp64 step from the fp32 w.  Derivation, ^ marking computed values:
  1. z^_r = z_r exp(th), |th| <= k u': k products, k - 1 additions (padding columns are exact zeros).
  2. a^_r = fl(count / sum): one rounding (the sum of small integer counts is exact); q^_r = fl(a^_r / z^_r): one more.  So
     q^_r = (a_r / z_r) exp(th), |th| <= (k + 2) u'.
  3. g^_t = sum_r R_rt q^_r: n products, n - 1 additions in any tree (the kernels add 4 or 16 partial gradients in fixed order):
     g^_t = g_t exp(th), |th| <= (k + n + 2) u'.
  4. eta^ is computed in double from the device's logf(k).  logf is within LOGF_ULP = 3 ulp (the OpenCL accuracy table for log; no
     OCML table is at hand, so the OpenCL figure is taken), the correctly rounded float32(log k) of the statement within 1/2 ulp, and
     one ulp is at most 2 u relative: log k differs by at most (2 * 3 + 1) u relative, eta, through the square root, by at most 4 u.
     The double operations (the quotient, sqrt, eta * g, exp, w * exp) add a few 2^-53, counted as one more u.  A product R_rt w_t
     that underflows costs at most 2^-149 against z_r >= Z_FLOOR = 2^-100 (asserted): k 2^-49 relative, counted as one more u.
     Together the exponent x^_t = eta^ g^_t satisfies |x^_t - e_t| <= e_t rho, rho = exp(m u') - 1, m = k + n + 2 + 4 + 1 + 1 = k + n + C1.
     (A product R_rt q^_r that underflows moves g by at most n 2^-149 absolutely, the exponent by eta times that: below 2^-120 for
     any eta < 2^20, and part of the last unit of C2.)
  5. p^_t = fl(w_t exp(x^_t)) = w_t exp(e_t) exp(D_t + th), |D_t| <= e_t rho, |th| <= u' (the cast to float).
  6. N^ = sum_t p^_t with k - 1 additions: N^ / N = sum_s w'_s exp(D_s + th_s), |th_s| <= k u', because w_s exp(e_s) / N = w'_s.  By
     Jensen N^ / N >= exp(-(rho sum_s w'_s e_s + k u')); with exp(x) <= 1 + x + x^2 for x <= 1 and rho max_s e_s <= 1,
     N^ / N <= exp(k u') (1 + rho (sum_s w'_s e_s) (1 + rho max_s e_s)).
  7. w'^_t = fl(p^_t / N^): one more rounding.  So |log(w'^_t / w'_t)| <= L_t = rho e_t + rho ebar (1 + rho emax) + (k + 2) u', ebar the
     w'-weighted mean of e; one more u in C2 covers the absolute terms of 4.
  Size condition, asserted: m <= 2^11 and A = ((emax + ebar) m + k + C2) u <= 2^-5.  Then rho <= m u' (1 + 2^-12), rho emax <= 1.001 * 2^-5,
  L_t <= 1.032 A_t, and exp(L) - 1 <= L (1 + L) <= 1.065 A_t <= A_t (1 + 2^-3), A_t the first-order bound (the bracket times u).  The
  floor 2^-126 makes the statement hold whether subnormal results are kept or flushed.  The fp64 reference's own rounding (k 2^-53
  relative) is nine orders below u.

certify_llh: s = sum_r a_r log z_r; the outputs are s * avg_doc_sz and s * words_in_doc.  Term r: log z^_r = log z_r + th with
|th| <= k u' — an absolute error of the logarithm, which is what covers a term with z near 1, where log z is near 0; logf adds
2 LOGF_ULP u relative to the logarithm, a^_r and the product one rounding each, the sum n - 1, the final scaling one.  So
|out - s c| <= ((n + 2 LOGF_ULP + 2 + 2) S + (k + 1) A) u c + 2^-126 with S = sum_r a_r |log z_r|, A = sum_r a_r, using
gamma(m) <= (m + 2) u (asserted: m <= 5790, as in gram_certificate).

certify_top is exact: no tolerance, against the device's own weights.

plan_lf decides from the fp64 trajectory alone which Lipschitz guess Lf = Lfguess 2^g the runs of a document use.  exp is taken in
double and the product w exp(x) cast to float, so a guess overflows surely when, in the first iteration from uniform,
max_t (log w_t + e_t) > log(FLT_MAX) + LF_MARGIN: that entry becomes inf, the normaliser inf, the weight NaN, and the NaN persists for
a run of any length.  A guess is surely finite when in every iteration up to J log N stays below log(FLT_MAX) - LF_MARGIN (N, the sum,
bounds every term), every z_r stays above Z_FLOOR and the size condition of certify_step holds.  A document is eligible if its first
surely-finite guess exists among the ten and every earlier guess is surely overflowing.  LF_MARGIN = 0.05 is five times the largest
exponent error the size condition allows (88.8 * 2^-13 ~ 0.011); the margins decide eligibility only, they are not tolerances.
"""
import os

import numpy as np

import route_reads

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_F32 = 2.0 ** -24
TINY = 2.0 ** -126
C1 = 8
C2 = 3
SECOND_ORDER = 1.0 + 2.0 ** -3
LOGF_ULP = 3
Z_FLOOR = 2.0 ** -100
LOG_FLT_MAX = float(np.log(np.float64(np.finfo(np.float32).max)))
LF_MARGIN = 0.05
A_MAX = 2.0 ** -5
M_MAX = 2 ** 11
_GAMMA_K_MAX = 5790  # largest m with gamma(m) <= (m + 2) u
ROW_SUM_MIN = 1.0e-10  # src/infer.cpp:376
LF_GUESSES = 10
J_DEFAULT = 15

# k_infer's dispatch (infer.hip): every instantiation with a k inside it and on both of its edges
K_VALUES = (1, 2, 3, 7, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 700, 1023, 1024)
K_PER_FORM = (7, 100, 200, 300, 1024)  # one k per instantiation: switch values, repeat calls, the null weights pointer
KEPT_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513)
CAP_VALUES = ("16", "512", "1000000")  # n < cap, == cap, == cap + 1 are in KEPT_COUNTS for 16 and 512; 1000000: k_infer's clamp decides
INFER_SWITCHES = {"ISLE_INFER_CAP_ROWS"}
V_DEFAULT = 1403  # not a multiple of 4
MAX_LEFT_OUT = 0.05


def instantiation(k):
    nq = (k + 3) // 4
    if nq <= 64:
        nf = (nq + 15) // 16
        return "inf_docs16_k<%d>" % (1 if nf <= 1 else 2 if nf <= 2 else 4)
    return "inf_docs_k<%d>" % (2 if (nq + 63) // 64 <= 2 else 4)


def lds_cap_rows(k):
    """Rows of a document that fit in LDS next to the kernel's own buffers (k_infer's clamp)."""
    ld = (k + 3) & ~3
    fixed = (17 if ld // 4 <= 64 else 5) * ld * 4
    return (163840 - 256 - fixed) // (ld * 4 + 4)


def infer_switches_read(table_names):
    """Names of the switches infer.hip reads (route_reads.py)."""
    src = open(os.path.join(_ROOT, "isle_amd", "csrc", "infer.hip")).read()
    assert "getenv" not in src
    return route_reads.switches_read(src, table_names)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 statement
# ---------------------------------------------------------------------------------------------------------------------------------
def eta64(k, it, Lf):
    return float(np.sqrt(2.0 * float(np.float32(np.log(np.float64(k)))) / float(it + 1)) / float(np.float32(Lf)))


def step64(R, a, w, it, Lf):
    """-> (w', e, z, logN): the fp64 step from w; R, a, w are taken as they are (cast to fp64)."""
    R = np.asarray(R, np.float64)
    a = np.asarray(a, np.float64)
    w = np.asarray(w, np.float64)
    k = R.shape[1]
    z = R @ w
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = R.T @ (a / z)
        e = eta64(k, it, Lf) * g
        lw = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)), -np.inf) + e
        top = float(np.max(lw))
        p = np.exp(lw - top)
        N = p.sum()
        return p / N, e, z, top + float(np.log(N))


def _report(name, bad, ratio, got, want, extra=""):
    idx = np.argsort(np.where(bad, ratio, -1.0), axis=None)[::-1][:5]
    rep = ["%s[%d] = %r vs fp64 %r: error / bound = %.4g" % (name, i, float(got.flat[i]), float(want.flat[i]), ratio.flat[i]) for i in idx]
    raise AssertionError("%d entries outside the fp32 bound%s:\n  %s" % (int(bad.sum()), extra, "\n  ".join(rep)))


def step_bound(R, a, w_prev32, it, Lf):
    """-> (w64, rel, A_max): the fp64 step and the relative bound per topic; asserts the preconditions and the size condition."""
    R = np.asarray(R)
    assert R.dtype == np.float32 and R.ndim == 2 and np.asarray(w_prev32).dtype == np.float32
    n, k = R.shape
    assert n >= 1 and np.all(R >= 0) and np.all(np.asarray(a) > 0) and np.all(np.asarray(w_prev32) >= 0), "precondition: inputs >= 0"
    w64, e, z, _ = step64(R, a, w_prev32, it, Lf)
    assert np.all(z >= Z_FLOOR), "precondition: z64 >= 2^-100 (got %g)" % z.min()
    assert np.all(np.isfinite(w64)) and np.all(np.isfinite(e))
    m = k + n + C1
    ebar = float(w64 @ e)
    A = ((e + ebar) * m + k + C2) * U_F32
    assert m <= M_MAX and float(A.max()) <= A_MAX, "size condition: m = %d, A = %g" % (m, A.max())
    return w64, A * SECOND_ORDER, float(A.max())


def certify_step(R, a, w_prev32, w_next32, it, Lf):
    """Every entry of w_next32 within rel[t] w64[t] + 2^-126 of the fp64 step from w_prev32.  -> {'max_ratio': max error / bound}."""
    w_next32 = np.asarray(w_next32)
    assert w_next32.dtype == np.float32 and w_next32.shape == (np.asarray(R).shape[1],)
    w64, rel, _ = step_bound(R, a, w_prev32, it, Lf)
    bound = rel * w64 + TINY
    with np.errstate(invalid="ignore"):
        err = np.abs(w_next32.astype(np.float64) - w64)
    ratio = np.where(np.isfinite(err), err / bound, np.inf)
    bad = ratio > 1.0
    if bad.any():
        _report("w", bad, ratio, w_next32, w64, " (iteration %d, k %d, n %d)" % (it, w64.shape[0], np.asarray(R).shape[0]))
    return {"max_ratio": float(ratio.max()), "rel_max": float(rel.max())}


def certify_llh(R, a, w32, words_in_doc, avg_doc_sz, llh32):
    """llh32 = (s avg_doc_sz, s words_in_doc), s = sum_r a_r log z_r, each within its relative bound.  -> {'max_ratio': ...}."""
    R = np.asarray(R)
    llh32 = np.asarray(llh32)
    assert R.dtype == np.float32 and np.asarray(w32).dtype == np.float32 and llh32.dtype == np.float32 and llh32.shape == (2,)
    n, k = R.shape
    a = np.asarray(a, np.float64)
    assert np.all(R >= 0) and np.all(a > 0) and np.all(np.asarray(w32) >= 0), "precondition: inputs >= 0"
    z = R.astype(np.float64) @ np.asarray(w32, np.float64)
    assert np.all(z >= Z_FLOOR), "precondition: z64 >= 2^-100 (got %g)" % z.min()
    lz = np.log(z)
    s = float(a @ lz)
    S = float(a @ np.abs(lz))
    m = n + 2 * LOGF_ULP + 2
    assert max(m, k) <= _GAMMA_K_MAX
    unit = ((m + 2) * S + (k + 1) * float(a.sum())) * U_F32
    scale = np.array([float(avg_doc_sz), float(words_in_doc)])
    want = s * scale
    bound = unit * np.abs(scale) + TINY
    with np.errstate(invalid="ignore"):
        err = np.abs(llh32.astype(np.float64) - want)
    ratio = np.where(np.isfinite(err), err / bound, np.inf)
    bad = ratio > 1.0
    if bad.any():
        _report("llh", bad, ratio, llh32, want, " (k %d, n %d)" % (k, n))
    return {"max_ratio": float(ratio.max())}


def certify_top(weights32, k, top_topic, top_weight, llh=None):
    """Exact: the heaviest five topics with weight > float32(1) / float32(k) of the given weights, in decreasing weight, ties to the
    lowest index, -1 / 0 where there is none, top_weight bit-equal to the weight it names.  With llh: a document with llh[d, 0] == 0 did
    not converge and has uniform weights, llh[d, 1] == 0 and no topic."""
    W = np.asarray(weights32)
    tt = np.asarray(top_topic)
    tw = np.asarray(top_weight)
    assert W.dtype == np.float32 and tw.dtype == np.float32 and W.ndim == 2 and W.shape[1] == k
    assert tt.shape == (W.shape[0], 5) and tw.shape == tt.shape
    unif = np.float32(1) / np.float32(k)
    for d in range(W.shape[0]):
        w = W[d]
        cand = np.flatnonzero(w > unif)
        cand = cand[np.argsort(-w[cand].astype(np.float64), kind="stable")][:5]  # stable: ties keep the lowest index first
        want_t = np.full(5, -1, np.int64)
        want_t[:len(cand)] = cand
        want_w = np.zeros(5, np.float32)
        want_w[:len(cand)] = w[cand]
        assert np.array_equal(tt[d], want_t), "document %d: top topics %s, the weights give %s" % (d, tt[d], want_t)
        assert np.array_equal(tw[d].view(np.uint32), want_w.view(np.uint32)), "document %d: top weights %s, the weights give %s" % (d, tw[d], want_w)
        if llh is not None and llh[d, 0] == 0:
            assert llh[d, 1] == 0 and np.all(w == unif) and np.all(tt[d] == -1), "document %d did not converge but is not uniform" % d


SURE_FINITE, SURE_OVERFLOW, BORDERLINE = "finite", "overflow", "borderline"


def classify_guess(R, a, k, Lf, J):
    """One Lipschitz guess on the fp64 trajectory from uniform: SURE_OVERFLOW / SURE_FINITE / BORDERLINE."""
    R64 = np.asarray(R, np.float64)
    n = R64.shape[0]
    w = np.full(k, np.float32(1) / np.float32(k), np.float64)
    for it in range(J):
        wn, e, z, logN = step64(R64, a, w, it, Lf)
        if it == 0 and float(np.max(np.log(w) + e)) > LOG_FLT_MAX + LF_MARGIN:
            return SURE_OVERFLOW
        if not (logN < LOG_FLT_MAX - LF_MARGIN) or not np.all(z >= Z_FLOOR) or not np.all(np.isfinite(wn)):
            return BORDERLINE
        A = ((float(e.max()) + float(wn @ e)) * (k + n + C1) + k + C2) * U_F32
        if A > A_MAX or k + n + C1 > M_MAX:
            return BORDERLINE
        w = wn
    zl = R64 @ w  # the log-likelihood reads z once more
    return SURE_FINITE if np.all(zl >= Z_FLOOR) else BORDERLINE


def plan_lf(R, a, k, Lfguess, J=J_DEFAULT):
    """-> the Lf (float32 value as float) that every run of 1..J iterations of this document uses, or None if the document is not
    eligible: its first surely-finite guess must exist and every earlier guess be surely overflowing."""
    Lf = np.float32(Lfguess)
    for _ in range(LF_GUESSES):
        c = classify_guess(R, a, k, float(Lf), J)
        if c == SURE_FINITE:
            return float(Lf)
        if c != SURE_OVERFLOW:
            return None
        Lf = np.float32(Lf * np.float32(2))
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
EDGE_LOW = (1, 2, 3)    # rows whose sum is just below the 1e-10 rule: dropped
EDGE_HIGH = (4, 5, 6)   # rows just above it: kept
COMMON_WORD = 8         # occurs in every document of two or more kept rows


def build_model(V, k, seed, kind="peaked"):
    """peaked: the rand ** 6 columns of test_gpu_infer.make_case with every seventh row zero.  zeros: the same with exact zeros inside
    kept rows: the last quarter of the topics (at least one, for k >= 2) is zero in the first half of the words, and three entries in
    ten are zero everywhere else, so that some topics have g_t = 0 exactly.  Rows EDGE_LOW / EDGE_HIGH sum to 0.9e-10 / 1.1e-10."""
    rng = np.random.default_rng(seed)
    M = rng.random((V, k)).astype(np.float32) ** 6
    if kind == "zeros":
        assert k >= 2
        M[rng.random((V, k)) < 0.3] = 0
        M[: V // 2, k - max(1, k // 4):] = 0
        M[np.arange(V), rng.integers(0, k - max(1, k // 4), V)] += np.float32(0.01)  # no row becomes empty by chance
    else:
        assert kind == "peaked"
    M /= M.sum(0, keepdims=True)
    M[::7] = 0.0
    for rows_, total in ((EDGE_LOW, 0.9e-10), (EDGE_HIGH, 1.1e-10)):
        for r in rows_:
            v = rng.random(k) + 0.5
            M[r] = (v * (total / v.sum())).astype(np.float32)
    ok = M.astype(np.float64).sum(1) > ROW_SUM_MIN
    assert not ok[list(EDGE_LOW)].any() and ok[list(EDGE_HIGH)].all() and ok[COMMON_WORD]
    return M


def build_docs(M, seed, extra_counts=(), half=False):
    """A deterministic corpus over the model M: one document per kept-row count of KEPT_COUNTS and extra_counts (each with 0..2 dropped
    words mixed in), an empty document, a document whose words are all absent from the model, a document made of the rows on both sides
    of the 1e-10 rule; COMMON_WORD in every document of two or more kept rows; a document count that is not a multiple of 4.
    half: words from the first half of the vocabulary only (the zeros model: g_t = 0 for the last topics).
    -> dict(offs, rows, counts, kept (list of id arrays), a (list of fp64 arrays), words (array))."""
    rng = np.random.default_rng(seed)
    V = M.shape[0]
    ok = M.astype(np.float64).sum(1) > ROW_SUM_MIN
    special = set(EDGE_LOW) | set(EDGE_HIGH) | {COMMON_WORD}
    lim = V // 2 if half else V
    kept_ids = np.array([w for w in np.flatnonzero(ok) if w not in special and w < lim])
    drop_ids = np.array([w for w in np.flatnonzero(~ok) if w not in special])
    counts_n = list(KEPT_COUNTS) + [c for c in extra_counts if c not in KEPT_COUNTS]
    assert max(counts_n) - 1 <= len(kept_ids)
    docs = []
    for n in counts_n:
        if n == 0:
            docs.append(np.zeros(0, np.int64))
            continue
        ids = rng.choice(kept_ids, size=n - 1 if n >= 2 else n, replace=False)
        if n >= 2:
            ids = np.append(ids, COMMON_WORD)
        docs.append(np.concatenate([ids, rng.choice(drop_ids, size=n % 3, replace=False)]))
    docs.append(rng.choice(drop_ids, size=3, replace=False))      # all words absent from the model
    docs.append(np.array(EDGE_LOW + EDGE_HIGH))                    # only the rows around the 1e-10 rule
    if len(docs) % 4 == 0:
        docs.append(np.append(rng.choice(kept_ids, size=5, replace=False), COMMON_WORD))
    docs = [np.sort(d).astype(np.uint32) for d in docs]
    offs = np.zeros(len(docs) + 1, np.int64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    rows = np.concatenate(docs)
    counts = rng.integers(1, 6, size=rows.shape[0]).astype(np.float32)
    kept, a = [], []
    for d in range(len(docs)):
        c = counts[offs[d]:offs[d + 1]].astype(np.float64)
        keep = ok[docs[d]]
        kept.append(docs[d][keep].astype(np.int64))
        a.append(c[keep] / c.sum() if len(c) else c)
    assert len(docs) % 4 != 0
    return dict(offs=offs, rows=rows, counts=counts, kept=kept, a=a, words=np.diff(offs))


def avg_doc_size(case):
    nz = int((case["words"] > 0).sum())
    return float(int(case["counts"].astype(np.float64).sum()) // max(nz, 1))


_CASES = {}


def make_case(k, kind="peaked", cap=None, Lf=10.0, J=J_DEFAULT, V=V_DEFAULT):
    """The corpus, the model and the plan of one GPU case (cached).  cap: the value of ISLE_INFER_CAP_ROWS (a string) or None; documents
    of eff - 1, eff and eff + 1 kept rows are added, eff = min(cap, what fits in LDS), where the vocabulary allows."""
    key = (k, kind, cap, Lf, J, V)
    if key not in _CASES:
        extra = ()
        if cap is not None:
            eff = min(int(cap), lds_cap_rows(k))
            if 2 <= eff <= 600:
                extra = (eff - 1, eff, eff + 1)
        M = build_model(V, k, 1000 + k, kind)
        case = build_docs(M, 2000 + k, extra_counts=extra, half=(kind == "zeros"))
        case.update(M=M, k=k, Lf=Lf, J=J, cap=cap, kind=kind, avg=avg_doc_size(case))
        case["plan"] = [plan_lf(M[r], a, k, Lf, J) if len(r) else None for r, a in zip(case["kept"], case["a"])]
        _CASES[key] = case
    return _CASES[key]


def left_out(case):
    """(documents with kept rows that the plan leaves out, documents with kept rows)."""
    some = [d for d in range(len(case["kept"])) if len(case["kept"][d])]
    return sum(case["plan"][d] is None for d in some), len(some)


# Lf = 1e-3: every document doubles five to nine times.  The first guess that survives the first iteration has exponents near 88: the
# weights collapse onto one topic, and with the peaked model the second iteration then overflows for most documents, so a run of two
# or more iterations takes a later guess than the run of one and the prefix is not one trajectory.  The peaked cases therefore run
# J = 1 (every document's first step, under its doubled Lf); the zeros model at k = 2 stays finite and runs all fifteen.
LF_CASES = [dict(k=30, Lf=1e-3, J=1), dict(k=300, Lf=1e-3, J=1), dict(k=2, kind="zeros", Lf=1e-3)]


def gpu_cases():
    """Every case test_gpu_infer_certified.py runs, as keyword arguments of make_case."""
    out = [dict(k=k) for k in K_VALUES]
    out += [dict(k=k, kind="zeros") for k in K_PER_FORM]
    out += [dict(k=k, cap=c) for k in K_PER_FORM for c in CAP_VALUES]
    out += LF_CASES
    return out


def case_id(kw):
    return "k%d-%s-cap%s-Lf%g-J%d" % (kw["k"], kw.get("kind", "peaked"), kw.get("cap"), kw.get("Lf", 10.0), kw.get("J", J_DEFAULT))


def certify_prefix(case, runs, stats=None):
    """runs[j], j = 0..J: the outputs of a run with iters = j (runs[0] may be None: w_0 is the fp32 uniform vector).  Certifies every
    eligible document at every j: the step from w_{j-1} to w_j, the llh, the top five, the convergence count; documents without kept rows
    must come back unconverged and uniform.  -> dict(w_ratio, llh_ratio, certified, left_out)."""
    k, M, J = case["k"], case["M"], case["J"]
    unif = np.float32(1) / np.float32(k)
    res = dict(w_ratio=0.0, llh_ratio=0.0, certified=0, left_out=0)
    for j in range(1, J + 1):
        g = runs[j]
        assert g["weights"].dtype == np.float32 and g["weights"].shape == (len(case["kept"]), k)
        assert g["nconverged"] == int((g["llh"][:, 0] != 0).sum())
        certify_top(g["weights"], k, g["top_topic"], g["top_weight"], llh=g["llh"])
    for d, (ids, a) in enumerate(zip(case["kept"], case["a"])):
        if len(ids) == 0:
            for j in range(1, J + 1):
                g = runs[j]
                assert np.all(g["llh"][d] == 0) and np.all(g["weights"][d] == unif) and np.all(g["top_topic"][d] == -1)
            continue
        Lf = case["plan"][d]
        if Lf is None:
            res["left_out"] += 1
            continue
        R = M[ids]
        prev = np.full(k, unif, np.float32)
        for j in range(1, J + 1):
            g = runs[j]
            assert g["llh"][d, 0] != 0, "document %d (n = %d) did not converge with iters = %d" % (d, len(ids), j)
            w = g["weights"][d]
            res["w_ratio"] = max(res["w_ratio"], certify_step(R, a, prev, w, j - 1, Lf)["max_ratio"])
            res["llh_ratio"] = max(res["llh_ratio"], certify_llh(R, a, w, case["words"][d], case["avg"], g["llh"][d])["max_ratio"])
            prev = w
        res["certified"] += 1
    if stats is not None:
        s = stats.setdefault(instantiation(k), dict(w_ratio=0.0, llh_ratio=0.0, certified=0, left_out=0))
        s["w_ratio"] = max(s["w_ratio"], res["w_ratio"])
        s["llh_ratio"] = max(s["llh_ratio"], res["llh_ratio"])
        s["certified"] += res["certified"]
        s["left_out"] += res["left_out"]
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy fp32 emulations of one step (and the mutants the certificates must reject)
# ---------------------------------------------------------------------------------------------------------------------------------
F = np.float32


def _seq_sum(v):
    return np.cumsum(np.asarray(v, F), dtype=F)[-1] if len(v) else F(0)


def _tree_sum(v, axis):
    v = np.asarray(v, F)
    v = np.moveaxis(v, axis, 0)
    n = 1
    while n < v.shape[0]:
        n *= 2
    v = np.concatenate([v, np.zeros((n - v.shape[0],) + v.shape[1:], F)])
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def emulate_z(R, w, tree=False):
    R = np.asarray(R, F)
    if tree:
        return _tree_sum(R * w[None, :], 1)
    z = np.zeros(R.shape[0], F)
    for t in range(R.shape[1]):
        z = z + R[:, t] * w[t]
    return z


def emulate_step(R, a, w, it, Lf, tree=False, mutant=None, w_stale=None):
    """One fp32 step as the kernels compute it: fp32 products and sums (sequential, or pairwise with four partial gradients), eta and the
    exponential in double.  a: fp64 count / sum.  mutant names a deliberate defect (see test_infer_certificate_cpu.py)."""
    R = np.asarray(R, F)
    w = np.asarray(w, F)
    n, k = R.shape
    a32 = np.asarray(a, np.float64).astype(F)
    if mutant == "a_not_normalised":
        a32 = (np.asarray(a, np.float64) / np.asarray(a, np.float64).min()).astype(F)
    q = a32 / emulate_z(R, w_stale if mutant == "stale_weights" else w, tree)
    rows = np.arange(n)
    if mutant == "last_row":
        rows = rows[:-1]
    if mutant == "row_4_mod_8":
        rows = rows[rows % 8 != 4]
    if tree:
        parts = []
        for wave in range(4):
            gp = np.zeros(k, F)
            for r in rows[rows % 4 == wave]:
                gp = gp + R[r] * q[r]
            parts.append(gp)
        if mutant == "partial_not_added":
            parts[1][int(np.argmax(parts[1]))] = 0
        g = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    else:
        g = np.zeros(k, F)
        for r in rows:
            g = g + R[r] * q[r]
        if mutant == "partial_not_added":
            t = int(np.argmax(g))
            g[t] = g[t] - _seq_sum((R[:, t] * q)[1::4])
    logk = np.log(np.float64(k + 1)) if mutant == "log_k_plus_1" else np.float64(np.log(F(k)))
    with np.errstate(divide="ignore"):
        eta = np.sqrt(2.0 * logk / np.float64(it if mutant == "eta_it" else it + 1)) / np.float64(F(Lf))
    with np.errstate(over="ignore", invalid="ignore"):
        p = (w.astype(np.float64) * np.exp(eta * g.astype(np.float64))).astype(F)
        if tree:
            shares = [_tree_sum(p[s::4], 0) if len(p[s::4]) else F(0) for s in range(4)]
            if mutant == "normaliser_share":
                shares[2] = F(0)
            N = ((shares[0] + shares[1]) + shares[2]) + shares[3]
        else:
            N = _seq_sum(p[: k - k // 4] if mutant == "normaliser_share" else p)
        if mutant == "padded_topic":
            assert k % 4
            N = N + F(1) / F(k)
        out = p / N
    if mutant == "small_topic_scaled":
        small = out < F(1e-3) * out.max()
        assert small.any()
        out = np.where(small, out * F(1.01), out).astype(F)
    return out.astype(F)


def emulate_llh(R, a, w, words_in_doc, avg_doc_sz, tree=False, mutant=None):
    z = emulate_z(R, w, tree)
    terms = np.asarray(a, np.float64).astype(F) * np.log(z.astype(F))
    s = _tree_sum(terms, 0) if tree else _seq_sum(terms)
    first, second = s * F(avg_doc_sz), s * F(words_in_doc)
    return np.array([second, first] if mutant == "llh_swapped" else [first, second], F)


def emulate_top(W, k, mutant=None):
    """The top-five rule on a D x k weight array.  -> (top_topic, top_weight)."""
    W = np.asarray(W, F)
    unif = F(1) / F(k)
    tt = np.full((W.shape[0], 5), -1, np.int32)
    tw = np.zeros((W.shape[0], 5), F)
    for d in range(W.shape[0]):
        w = W[d]
        cand = np.flatnonzero(w >= unif if mutant == "top_ge" else w > unif)
        if mutant == "top_tie_high":
            cand = cand[::-1]
        cand = cand[np.argsort(-w[cand].astype(np.float64), kind="stable")][:5]
        tt[d, :len(cand)] = cand
        tw[d, :len(cand)] = w[(cand + 1) % k] if mutant == "top_wrong_weight" else w[cand]
    return tt, tw
