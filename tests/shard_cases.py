"""The sharded (N > 1) path held against fp64 at shard edges: layouts, inputs, the per-rank worker and the certificates
(no GPU needed to import this module; the worker alone opens the device).  tests/rank_launch.py starts the ranks and gives each its
context and communicator.

Layouts give the document bounds explicitly (rank r holds documents [bounds[r], bounds[r + 1])):

  L2  2 ranks  [0, ceil(D / 2), D], D odd       a plain split, unequal by one
  L3  3 ranks  [0, 1, D, D]                     a one-document shard and an empty last shard
  L4  4 ranks  [0, 0, a, a, D], a = D // 3      an empty first and an empty middle shard
  LP  4 ranks  plan_shards on a corpus whose document 2 holds more than 3/4 of the entries: the planner's own empty shards

Per layout: the Gram apply (four kinds of values, b in {1, 10, 11, 25, 32}), thresholding (L3, L4: a shard that keeps no column), k-means++
and both Lloyd loops (L2, L3, L4; k in {9, 65, 300}).  Apart from the layouts, three Krylov-Schur cases put the row slices of the sharded
orthogonalisation (ks_row_slice) on their edges: a slice of zero rows, ragged slices, a leading dimension that is no multiple of four.

The worker runs as one fresh process per rank on one GPU over the host-staged transport (isle_hip_comm_init_host completed by gloo, as
test_gpu_multirank.py does) and writes every array it fetched to an .npz per rank.  The certificates below take those per-rank arrays
("ranks": a list of mappings, one per rank) and hold them against fp64; tests/test_shard_cases_cpu.py feeds them arrays made from the
fp64 reference and the CPU oracle alone, right ones and ones made by a wrong rule, so no bound rests on what the device returns.

Bounds: gram_certificate / kmeans_certificate / ks_certificate / stages_certificate, plus two statements of arithmetic:
- the all-reduce of Z adds at most N - 1 roundings to an entry, in any order: coefficient n_w + max n_d + 2 + (N - 1);
- the centroid bound (n_c + m_c + 2) u holds for any tree of the n_c additions, so it does not depend on how the sums were split.
"""
import os

import numpy as np

import gram_certificate as gc
import kmeans_certificate as kc
import ks_certificate as ksc
import rank_launch
import stages_certificate as stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORLD = {"L2": 2, "L3": 3, "L4": 4, "LP": 4, "slice-empty": 4, "ld-odd": 4, "ld-even": 3}  # layouts, then the Krylov-Schur cases


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------------------
def plan_shards_py(offs, parts):
    """isle_hip_plan_shards restated: bound p is the first document at or behind p / parts of the entries, never below bound p - 1."""
    offs = np.asarray(offs, np.int64)
    D, nnz = len(offs) - 1, int(offs[-1])
    b = [0]
    for p in range(1, parts):
        d = int(np.searchsorted(offs, (nnz * p) // parts, side="left"))
        b.append(max(min(d, D), b[-1]))
    b.append(D)
    return np.asarray(b, np.int64)


def bounds(layout, D, offs=None):
    if layout == "L2":
        assert D % 2 == 1
        return np.array([0, (D + 1) // 2, D], np.int64)
    if layout == "L3":
        return np.array([0, 1, D, D], np.int64)
    if layout == "L4":
        a = D // 3
        return np.array([0, 0, a, a, D], np.int64)
    assert layout == "LP" and offs is not None
    return plan_shards_py(offs, 4)


def rank_of_doc(bnd, d):
    """The rank whose range holds document d (the last of equal bounds: empty ranges hold nothing)."""
    return np.searchsorted(np.asarray(bnd), np.asarray(d), side="right") - 1


def shard(B, bnd, rank):
    """-> (vals, rows, offs, doc_offset) of rank's documents of the CSC dict B."""
    d0, d1 = int(bnd[rank]), int(bnd[rank + 1])
    o0, o1 = int(B["offs"][d0]), int(B["offs"][d1])
    return B["vals"][o0:o1], B["rows"][o0:o1], (B["offs"][d0:d1 + 1] - o0).astype(np.int64), d0


# ---------------------------------------------------------------------------------------------------------------------------------
# Gram apply: inputs
# ---------------------------------------------------------------------------------------------------------------------------------
GRAM_V = gc.GL_RB + 1  # two word bands, the second of one row
GRAM_D = 601
GRAM_WIDTHS = (1, 10, 11, 25, 32)  # 10 | 11: the panel edge; 32: the widest
GRAM_KINDS = ("rowconst", "perrank", "entry", "sqrt")
_GRAM = {}


def gram_pattern(layout):
    if layout != "LP":
        return gc.pattern_random(GRAM_V, GRAM_D, 4, 40, 11, must=(GRAM_V - 1,))
    rng = np.random.default_rng(12)
    cols = [rng.choice(GRAM_V, size=1 + d % 2, replace=False) for d in range(GRAM_D)]
    cols[2] = rng.choice(GRAM_V - 1, size=3600, replace=False)
    cols[0] = np.append(cols[0], GRAM_V - 1)
    return gc.pattern_from_lists(GRAM_V, cols)


def gram_case(layout, kind):
    """dict(V, D, rows, offs, vals, bounds, world, X {b: (V, b)}, B64, special): one matrix and its inputs.  special: the rank whose
    documents carry per-entry values (kind "entry"), else -1."""
    key = (layout, kind)
    if key in _GRAM:
        return _GRAM[key]
    V, D = GRAM_V, GRAM_D
    rows, offs = gram_pattern(layout)
    bnd = bounds(layout, D, offs)
    world = WORLD[layout]
    doc = np.repeat(np.arange(D), np.diff(offs))
    rk = rank_of_doc(bnd, doc)
    special = -1
    if kind == "sqrt":
        vals, _ = gc.sqrt_row_values(V, rows, 5)
    elif kind == "perrank":  # the value of word w by (w, rank): row-constant on every rank, not over the corpus
        shift = np.array([0, 1, 0, 2])[rk]  # three values, four ranks: the ranks that hold documents in any one layout get different shifts
        vals = np.asarray(gc.DYADIC_S, np.float32)[(rows.astype(np.int64) + shift) % 3]
    else:
        vals, _ = gc.dyadic_row_values(V, rows, 5)
        if kind == "entry":
            special = int(np.flatnonzero(np.diff(bnd) > 1)[-1])  # the last rank with more than one document
            mine = rk == special
            vals = vals.copy()
            vals[mine] = gc.dyadic_entry_values(rows, 6)[mine]
    B64 = gc.csc64(V, vals, rows, offs)
    X = {b: (gc.normal_X(V, b, 100 + b) if kind == "sqrt" else gc.dyadic_X(V, b, 100 + b, B=B64)) for b in GRAM_WIDTHS}
    _GRAM[key] = dict(V=V, D=D, rows=rows, offs=offs, vals=vals.astype(np.float32), bounds=bnd, world=world, X=X, B64=B64, special=special,
                      layout=layout, kind=kind)
    return _GRAM[key]


def words_of_ranks(case):
    """(V, world) bool: word w occurs on rank r."""
    doc = np.repeat(np.arange(case["D"]), np.diff(case["offs"]))
    rk = rank_of_doc(case["bounds"], doc)
    occ = np.zeros((case["V"], case["world"]), bool)
    occ[case["rows"].astype(np.int64), rk] = True
    return occ


def row_constant(vals, rows, V):
    """every word holds one value"""
    first = np.full(V, np.nan)
    first[np.asarray(rows, np.int64)[::-1]] = np.asarray(vals)[::-1]
    return bool(np.all(first[np.asarray(rows, np.int64)] == vals))


def has_empty_shard(bnd):
    return bool(np.any(np.diff(bnd) == 0))


def same_on_all_ranks(ranks, key):
    """the replicated result `key`: bit-identical on every rank -> rank 0's"""
    a = np.asarray(ranks[0][key])
    for r, q in enumerate(ranks[1:], 1):
        b = np.asarray(q[key])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s differs between rank 0 and rank %d" % (key, r)
    return a


def certify_gram_case(case, ranks):
    """Every width of one Gram case.  -> dict(forms, max_ratio_over_coeff (kind sqrt) | exact)."""
    kind, world = case["kind"], case["world"]
    forms = [int(np.asarray(q["g_%s_form" % kind]).ravel()[0]) for q in ranks]
    assert len(forms) == world
    assert len(set(forms)) == 1, "operator forms differ between the ranks: %s" % forms  # one form on all ranks, whatever the shards
    if kind == "entry":
        assert forms[0] == 0, forms
    elif not has_empty_shard(case["bounds"]):
        assert forms[0] == 1, forms  # every shard row-constant: the banded form, with per-rank scales
    out = dict(forms=forms, max_ratio_over_coeff=0.0)
    for b in GRAM_WIDTHS:
        Z = same_on_all_ranks(ranks, "g_%s_b%d" % (kind, b))
        X = case["X"][b]
        Z64, M, B = gc.gram64(case["V"], case["vals"], case["rows"], case["offs"], X)
        gc.certify_structure(Z, B, X)
        if kind == "sqrt":
            res = gc.certify_gram(Z, Z64, M, B, extra=world - 1)
            out["max_ratio_over_coeff"] = max(out["max_ratio_over_coeff"], res["max_ratio_over_coeff"])
        else:
            gc.certify_exact(Z, Z64, M)
    return out


def gram_reference_ranks(case, leave_out=None):
    """What every rank must hold, from fp64 alone: the sum of the shards' fp64 products, rounded to fp32 once.  leave_out: a rank whose
    Z is left out of the sum (a wrong rule)."""
    world, kind = case["world"], case["kind"]
    res = {"g_%s_form" % kind: np.array([0 if kind == "entry" or has_empty_shard(case["bounds"]) else 1])}
    for b in GRAM_WIDTHS:
        Z = np.zeros((case["V"], b))
        for r in range(world):
            if r == leave_out:
                continue
            v, rw, of, _ = shard(case, case["bounds"], r)
            Z += gc.gram64(case["V"], v, rw, of, case["X"][b])[0]
        res["g_%s_b%d" % (kind, b)] = np.asfortranarray(Z.astype(np.float32))
    return [res] * world


# ---------------------------------------------------------------------------------------------------------------------------------
# k-means: inputs
# ---------------------------------------------------------------------------------------------------------------------------------
KM_V, KM_D = 403, 3001
KM_KS = (9, 65, 300)
KM_LAYOUTS = ("L2", "L3", "L4")
KM_REPS = 3
KM_FREE_SEED = 7
KM_OUTLIER_SCALE = 64.0
_KM = {}


def km_corpus(outlier):
    """make_B at V = 403 trimmed to D = 3001.  outlier: the last document's values scaled by 64, so that its distance to any seed is a
    large part of the k-means++ residual's total (and the document is not row-constant any more)."""
    if outlier not in _KM:
        if False not in _KM:
            from tools.synth import make_B
            B0 = make_B(KM_V, 3300, 20, 3)
            assert B0["D"] >= KM_D, B0["D"]
            n = int(B0["offs"][KM_D])
            B = dict(V=B0["V"], D=KM_D, vals=B0["vals"][:n].copy(), rows=B0["rows"][:n].copy(), offs=B0["offs"][:KM_D + 1].copy())
            B["X"] = kc.csc_points(B)
            _KM[False] = B
        if outlier:
            B = dict(_KM[False])
            B["vals"] = B["vals"].copy()
            B["vals"][int(B["offs"][KM_D - 1]):] *= np.float32(KM_OUTLIER_SCALE)
            B["X"] = kc.csc_points(B)
            _KM[True] = B
    return _KM[outlier]


class KmRef:
    """The fp64 side of one (corpus, k): U (random orthonormal, fp32), P64 = B^T U, |B|^T |U|, the squared norms, the rounding the device's
    fp32 projection of a document may carry, and the injected seeds (the last document is never a seed)."""

    def __init__(self, outlier, k):
        self.B, self.k = km_corpus(outlier), k
        X = self.B["X"]
        U = np.linalg.qr(np.random.default_rng(17 * k).standard_normal((KM_V, k)))[0]
        self.U = np.asfortranarray(U, dtype=np.float32)
        U64 = self.U.astype(np.float64)
        self.P64 = np.asarray(X.T @ U64)
        self.Pabs = np.asarray(abs(X).T @ np.abs(U64))
        self.pn2 = np.einsum("ij,ij->i", self.P64, self.P64)
        self.Perr = ((np.diff(self.B["offs"]) + 1) * 2.0 ** -24)[:, None] * self.Pabs
        self.seeds = np.sort(np.random.default_rng(k + 1).choice(KM_D - 1, k, replace=False)).astype(np.uint64)


def km_ref(outlier, k):
    if (outlier, k) not in _KM:
        _KM[(outlier, k)] = KmRef(outlier, k)
    return _KM[(outlier, k)]


def degenerate_start(c):
    """Twins (bit-identical), a zero centre, centres on documents, and two far-off centres whose clusters are empty on every rank."""
    k = c.k
    C = c.P64[c.seeds.astype(np.int64)].astype(np.float32)
    C[k - 1] = C[1]
    C[k - 2] = C[1]
    C[3] = 0.0
    far = 1e3 * float(np.abs(C).max())
    C[5] = far
    C[6] = -far
    return C


def kmpp_schedule(k):
    """The dice of every round when no draw repeats a seed (injected seeds: exactly these rounds; free-running: at least as many)."""
    s, draws = 1, []
    maxdraw = 2 + int(np.ceil(np.sqrt(k)))
    while s < k:
        nd = 0
        while nd < 1 + np.sqrt(max(s - 5, 0)):
            nd += 1
        nd = min(nd, maxdraw)
        draws.append(nd)
        s += min(nd, k - s)
    return draws


def concat(ranks, key):
    return np.concatenate([np.asarray(q[key]) for q in ranks])


def certify_kmpp_injected(c, ranks):
    """C_lowd = P[seeds], min_dist per document, and the residual: the fp64 sum of the certified distances of documents 0 .. D - 2 within
    the sum of their allowances.  -> dict(residual, want, allow)."""
    k = c.k
    g = dict(seeds=same_on_all_ranks(ranks, "pp%d_seeds" % k), C_lowd=same_on_all_ranks(ranks, "pp%d_C" % k))
    res = float(same_on_all_ranks(ranks, "pp%d_res" % k).ravel()[0])
    assert int(same_on_all_ranks(ranks, "pp%d_rounds" % k).ravel()[0]) == len(kmpp_schedule(k))
    md = concat(ranks, "pp%d_md" % k)
    assert md.shape == (c.B["D"],)
    d, E = kc.certify_kmeanspp(c, g, md)
    want, allow = float(d[:-1].sum()), float(E[:-1].sum())
    assert abs(res - want) <= allow, ("k=%d: residual %.9g, fp64 sum of the min-distances of documents 0 .. D - 2 %.9g, allowance %.3g "
                                      "(last document's distance %.9g)" % (k, res, want, allow, d[-1]))
    return dict(residual=res, want=want, allow=allow, ratio=abs(res - want) / allow)


def certify_kmpp_free(c, ranks):
    k = c.k
    seeds = same_on_all_ranks(ranks, "fr%d_seeds" % k).astype(np.int64)
    assert len(np.unique(seeds)) == k and seeds.min() >= 0 and seeds.max() < c.B["D"], "seeds not distinct or out of range"
    Cl = same_on_all_ranks(ranks, "fr%d_C" % k)
    Bs = c.B["X"][:, seeds].T.toarray()
    res = kc.certify_gemm(Bs, c.U, Cl, what="free-running k-means++ seeds k=%d:" % k)
    rounds = int(same_on_all_ranks(ranks, "fr%d_rounds" % k).ravel()[0])
    sched = kmpp_schedule(k)
    assert rounds >= len(sched), (rounds, len(sched))
    return dict(rounds=rounds, gemm_ratio=res["max_ratio"], wide_round=max(sched) > 16)


def _note(stats, res):
    stats["max_ratio"] = max(stats.get("max_ratio", 0.0), res["max_ratio"])
    stats["off"] = stats.get("off", 0) + res.get("off", 0)


def certify_projected(c, ranks, tag, C0, near_ties=False):
    """Lloyd in span(U) by the prefix method: runs with max_reps = 1 .. KM_REPS from C0, stored under `tag`."""
    k, stats = c.k, dict(cen_ratio=0.0)
    runs = []
    for r in range(1, KM_REPS + 1):
        it = int(same_on_all_ranks(ranks, "%s_r%d_it" % (tag, r)).ravel()[0])
        runs.append(dict(iters=it, assign=concat(ranks, "%s_r%d_assign" % (tag, r)), C=same_on_all_ranks(ranks, "%s_r%d_C" % (tag, r))))
    C_in = C0
    for r, res in enumerate(runs, 1):
        if res["iters"] < r:  # stopped early: the previous run's bits
            prev = runs[r - 2]
            assert res["iters"] == prev["iters"] and np.array_equal(res["assign"], prev["assign"])
            assert res["C"].tobytes() == prev["C"].tobytes()
            break
        what = "%s k=%d iter %d:" % (tag, k, r)
        _note(stats, kc.certify_assignment(c.P64, c.pn2, C_in, res["assign"], what=what, near_ties=near_ties))
        cen = kc.certify_centroids(c.P64, res["assign"], [q["assign"] for q in runs[:r - 1]], res["C"], X_abs=c.Pabs, X_err=c.Perr, what=what)
        stats["cen_ratio"] = max(stats["cen_ratio"], cen["max_ratio"])
        stats["empty"] = cen["empty"]
        C_in = res["C"]
    stats["runs"] = runs
    return stats


def certify_sparse(c, ranks, tag, lift_from, reproducible, frob_tol):
    """Lloyd on B from the lifted centres, by the prefix method."""
    k, X, stats = c.k, c.B["X"], dict(cen_ratio=0.0)
    lifted = same_on_all_ranks(ranks, "%s_lift" % tag)
    kc.certify_gemm(c.U, np.asarray(lift_from).T, lifted, what="lift k=%d:" % k)
    runs = []
    for r in range(1, KM_REPS + 1):
        it = int(same_on_all_ranks(ranks, "%s_r%d_it" % (tag, r)).ravel()[0])
        runs.append(dict(iters=it, assign=concat(ranks, "%s_r%d_assign" % (tag, r)), C=same_on_all_ranks(ranks, "%s_r%d_cen" % (tag, r))))
    C_in = lifted
    for r, res in enumerate(runs, 1):
        if res["iters"] < r:
            if reproducible:
                prev = runs[r - 2]
                assert res["iters"] == prev["iters"] and np.array_equal(res["assign"], prev["assign"])
                assert res["C"].tobytes() == prev["C"].tobytes()
            break
        what = "%s k=%d iter %d:" % (tag, k, r)
        _note(stats, kc.certify_assignment(X, None, np.asarray(C_in).T, res["assign"], what=what))
        cen = kc.certify_centroids(X, res["assign"], [q["assign"] for q in runs[:r - 1]], res["C"].T, frob_tol=frob_tol, what=what)
        stats["cen_ratio"] = max(stats["cen_ratio"], cen["max_ratio"])
        C_in = res["C"]
    return stats


# ---------------------------------------------------------------------------------------------------------------------------------
# thresholding
# ---------------------------------------------------------------------------------------------------------------------------------
TH_V, TH_K = 1200, 5
TH_FLAT, TH_FLAT_WORDS, TH_REGULAR = 100, 1000, 200  # documents 0 .. 99: a thousand words once each; then 200 planted-topic documents
TH_LAYOUTS = ("L3", "L4")
TH_RATE, TH_SEED = 0.3, 11
_TH = {}


def th_corpus():
    """Counts A (V = 1200, D = 300).  The first 100 documents hold 1000 words once each: their normalised counts avg / 1000 round to 0
    (the corpus average stays below 500 tokens), so the threshold rule keeps none of them.  On L3 they are the one-document shard, on L4
    the whole of rank 1: a shard with D > 0 whose B has no column."""
    if "A" not in _TH:
        from tools.synth import Corpus
        cnt, rows, offs = Corpus(TH_V, TH_REGULAR, TH_K, 3).A()
        rng = np.random.default_rng(4)
        flat = np.concatenate([np.sort(rng.choice(TH_V, TH_FLAT_WORDS, replace=False)) for _ in range(TH_FLAT)]).astype(np.uint32)
        n = TH_FLAT * TH_FLAT_WORDS
        _TH["A"] = dict(V=TH_V, D=TH_FLAT + TH_REGULAR, vals=np.concatenate([np.ones(n, np.float32), cnt]), rows=np.concatenate([flat, rows]),
                        offs=np.concatenate([np.arange(TH_FLAT) * TH_FLAT_WORDS, n + offs]).astype(np.int64))
    return _TH["A"]


def th_reference(sampled):
    """B of the whole corpus as one rank must build it: the plain restatement (stages_certificate.ref_threshold); with sampling, the CPU
    port (tools.synth), whose key draw is the host code of both sides.  -> dict(rows, vals, offs, original_cols, zetas, D, entries_above)."""
    if sampled not in _TH:
        A = th_corpus()
        full = stc.ref_threshold(A["V"], A["vals"], A["rows"], A["offs"], TH_K)
        if sampled:
            from tools.synth import Corpus
            port = Corpus.from_csc(A["V"], A["D"], A["vals"], A["rows"], A["offs"]).threshold(TH_K, sample_rate=TH_RATE, sample_seed=TH_SEED)
            assert 0 < port["D"] < full["D"]
            _TH[True] = dict(port, entries_above=full["nnz"], zetas=full["zetas"])
        else:
            _TH[False] = dict(full, entries_above=full["entries_above"])
    return _TH[sampled]


def certify_threshold(want, bnd, ranks, tag):
    """The shards' B side by side is the single-rank B bit for bit (rows, vals, column lengths, original_cols), the thresholds are the
    corpus's on every rank, and doc_offset / D_global tile B's columns."""
    for f in ("rows", "original_cols"):
        got = concat(ranks, "%s_%s" % (tag, f))
        assert got.shape == np.asarray(want[f]).shape and np.array_equal(got.astype(np.int64), np.asarray(want[f]).astype(np.int64)), "%s: %s differs" % (tag, f)
    got = concat(ranks, "%s_vals" % tag)
    assert got.dtype == np.float32 and got.tobytes() == np.asarray(want["vals"], np.float32).tobytes(), "%s: vals differ" % tag
    lens = np.concatenate([np.diff(np.asarray(q["%s_offs" % tag])) for q in ranks])
    assert np.array_equal(lens, np.diff(want["offs"])), "%s: column lengths differ" % tag
    z = same_on_all_ranks(ranks, "%s_zetas" % tag)
    assert z.tobytes() == np.asarray(want["zetas"], np.float32).tobytes(), "%s: thresholds differ" % tag
    at = 0
    for r, q in enumerate(ranks):
        off, glob, Db, above, kept = (int(x) for x in np.asarray(q["%s_meta" % tag]))
        assert np.asarray(q["%s_offs" % tag])[0] == 0 and len(q["%s_offs" % tag]) == Db + 1
        assert (off, glob) == (at, want["D"]), "%s rank %d: doc_offset %d of %d, expected %d of %d" % (tag, r, off, glob, at, want["D"])
        assert above == want["entries_above"] and kept == Db
        oc = np.asarray(q["%s_original_cols" % tag]).astype(np.int64)
        assert np.all((oc >= bnd[r]) & (oc < bnd[r + 1])), "%s rank %d holds a column of another rank's document" % (tag, r)
        at += Db
    assert at == want["D"]
    return [int(np.asarray(q["%s_meta" % tag])[2]) for q in ranks]


def threshold_reference_ranks(want, bnd, tag, count_dropped=False):
    """`want` cut into the layout's shards.  count_dropped: a wrong rule — a shard's place among B's columns counts the documents it
    held, not the columns it kept."""
    oc = np.asarray(want["original_cols"]).astype(np.int64)
    ranks, at = [], 0
    for r in range(len(bnd) - 1):
        cols = np.flatnonzero((oc >= bnd[r]) & (oc < bnd[r + 1]))
        c0, c1 = (int(cols[0]), int(cols[-1]) + 1) if cols.size else (0, 0)
        o0, o1 = int(want["offs"][c0]), int(want["offs"][c1])
        ranks.append({"%s_rows" % tag: np.asarray(want["rows"])[o0:o1], "%s_vals" % tag: np.asarray(want["vals"], np.float32)[o0:o1],
                      "%s_offs" % tag: np.asarray(want["offs"])[c0:c1 + 1] - o0, "%s_original_cols" % tag: np.asarray(want["original_cols"])[c0:c1],
                      "%s_zetas" % tag: np.asarray(want["zetas"], np.float32),
                      "%s_meta" % tag: np.array([at, want["D"], c1 - c0, want["entries_above"], c1 - c0], np.int64)})
        at += int(bnd[r + 1] - bnd[r]) if count_dropped else c1 - c0
    return ranks


# ---------------------------------------------------------------------------------------------------------------------------------
# Krylov-Schur through the sparse entry: the row-sharded orthogonalisation at its slice edges
# ---------------------------------------------------------------------------------------------------------------------------------
KS_TOL, KS_MAXIT, KS_SEED = 1e-4, 100, 1
KS_CASES = {
    # zero-row slice, ragged slice, the plain kernels (m < 32)
    "slice-empty": dict(V=33, nev=4, blk=4, ncv=12, slices=[(0, 12), (12, 24), (24, 33), (33, 33)]),
    # ld & 3 != 0: update_k strided, vtf_mfma_k off its float4 path once the basis reaches 64 columns, row chunk halved (to 256)
    "ld-odd": dict(V=1026, nev=40, blk=10, ncv=90, slices=[(0, 260), (260, 520), (520, 780), (780, 1026)]),
    # update_mfma_k strided and 16-byte aligned at r0, ragged last slice
    "ld-even": dict(V=1028, nev=40, blk=10, ncv=90, slices=[(0, 344), (344, 688), (688, 1028)]),
}
# (case, tag, environment): the row-sharded step (the default with several ranks), the replicated one, and the split small EVD once
KS_RUNS = [(name, tag, env) for name in KS_CASES for tag, env in (("shard", {}), ("repl", {"ISLE_KS_ROWSHARD": "0"}))] + [("ld-odd", "split", {"ISLE_EVD_SPLIT": "1"})]
_KS = {}


def ks_row_slice_py(dim, world, rank):
    """ks_host.h ks_row_slice: rows per rank rounded up to a multiple of four, the slices clipped to dim."""
    nloc = (-(-dim // world) + 3) & ~3
    r0 = min(dim, rank * nloc)
    return r0, min(dim, r0 + nloc)


def ks_case(name):
    """The case with B (CSC dict), its even document bounds, A64 = B64 B64^T dense, lam (its eigenvalues, descending)."""
    if name not in _KS:
        c = dict(KS_CASES[name], name=name, world=WORLD[name])
        V = c["V"]
        if V == 33:  # hand-made, dense: four separated leading values over a decaying bulk
            rng = np.random.default_rng(33)
            D = 60
            Q = np.linalg.qr(rng.standard_normal((V, V)))[0]
            W = np.linalg.qr(rng.standard_normal((D, V)))[0]
            sig = np.sqrt(np.concatenate([[1.0, 0.8, 0.6, 0.45], np.linspace(0.1, 0.01, V - 4)]))
            M = ((Q * sig) @ W.T).astype(np.float32)
            B = dict(V=V, D=D, vals=M.T.reshape(-1).copy(), rows=np.tile(np.arange(V, dtype=np.uint32), D), offs=np.arange(D + 1, dtype=np.int64) * V)
        else:
            from tools.synth import make_B
            B0 = make_B(V, 3000, c["nev"], 1)
            B = dict(V=B0["V"], D=B0["D"], vals=B0["vals"], rows=B0["rows"], offs=B0["offs"])
        X = kc.csc_points(B).toarray()
        c["B"], c["A64"] = B, X @ X.T
        c["lam"] = np.linalg.eigvalsh(c["A64"])[::-1]
        c["bounds"] = np.linspace(0, B["D"], c["world"] + 1).astype(np.int64)
        c["m"] = c["ncv"] + c["blk"]  # an upper bound on the rows of H
        _KS[name] = c
    return _KS[name]


def ks_residual_bound(c):
    """r_i <= tol lam_i + C[residual] m 2^-24 lam_1 for the leading nev + 1 eigenvalues: the solver's own test (ks_first_unconverged divides
    the estimate by the Ritz value) plus the certificate's rounding allowance."""
    lam = c["lam"][:c["nev"] + 1]
    return KS_TOL * lam + ksc.C["residual"] * c["m"] * ksc.U_F32 * lam[0]


def ks_routes(c):
    """(slice rows, m, route) of every orthogonalisation step of the row-sharded solve, per slice."""
    sizes, _ = ksc.ortho_sizes(c["nev"], c["blk"], c["ncv"], 1)
    return [(r1 - r0, m, ksc.route(r1 - r0, b, m, ld=c["V"])) for r0, r1 in c["slices"] for m, b in sorted(set(sizes))]


def certify_ks(c, ranks, tag):
    """A posteriori, whatever the start block: residual enclosure of the leading nev eigenvalues (a theorem: a symmetric matrix has an
    eigenvalue within ||A u - l u|| / ||u|| of l), the solver's residual test, orthonormality, Rayleigh quotients.
    -> dict(residual, orth, rayleigh: error / bound; restarts)."""
    nev, m, lam, A = c["nev"], c["m"], c["lam"], c["A64"]
    cnt = same_on_all_ranks(ranks, "%s_counts" % tag)  # rc, nconv, restarts, napplies
    assert int(cnt[0]) == 0 and int(cnt[1]) == nev, "rc %d, nconv %d of %d" % (cnt[0], cnt[1], nev)
    ev = same_on_all_ranks(ranks, "%s_evals" % tag).astype(np.float64)
    U = same_on_all_ranks(ranks, "%s_U" % tag).astype(np.float64)
    assert ev.shape == (nev,) and U.shape == (c["V"], nev)
    AU = A @ U
    un = np.linalg.norm(U, axis=0)
    r = np.linalg.norm(AU - U * ev, axis=0) / un
    lo, hi = ev - r, ev + r
    order = np.argsort(-ev)
    assert np.array_equal(order, np.arange(nev)), "Ritz values not in descending order"
    assert np.all(hi[1:] < lo[:-1]), "residual intervals overlap: %s" % np.flatnonzero(~(hi[1:] < lo[:-1]))[:5]
    for i in range(nev):
        inside = np.flatnonzero((lam >= lo[i]) & (lam <= hi[i]))
        assert list(inside) == [i], "interval %d [%.9g, %.9g] holds the eigenvalues %s (the %d-th is %.9g)" % (i, lo[i], hi[i], list(inside), i, lam[i])
    bound = ks_residual_bound(c)[:nev]
    res = float((r / bound).max())
    assert res <= 1.0, "residual %d: %.3g > tol lam_i + C m u lam_1 = %.3g" % (int(np.argmax(r / bound)), r[np.argmax(r / bound)], bound[np.argmax(r / bound)])
    orth = float(np.abs(U.T @ U - np.eye(nev)).max() / (ksc.C["orth"] * m * ksc.U_F32))
    assert orth <= 1.0, "max |U^T U - I| is %.3g of its bound" % orth
    ray = float(np.abs(np.sum(U * AU, axis=0) - ev).max() / (ksc.C["rayleigh"] * m * ksc.U_F32 * lam[0]))
    assert ray <= 1.0, "max |u^T A u - lam| is %.3g of its bound" % ray
    return dict(residual=res, orth=orth, rayleigh=ray, restarts=int(cnt[2]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the worker: one process per rank
# ---------------------------------------------------------------------------------------------------------------------------------
def worker_main(rank, port, out, job):
    """job: a layout (Gram apply, thresholding, k-means on its shards) or a Krylov-Schur case."""
    def body(hp, rank, world, res):
        if job in KS_CASES:
            _worker_ks(hp, job, rank, res)
        else:
            _worker_gram(hp, job, rank, res)
            if job in TH_LAYOUTS:
                _worker_threshold(hp, job, rank, res)
            if job in KM_LAYOUTS:
                _worker_kmeans(hp, job, rank, res)
    rank_launch.run_rank(WORLD[job], int(rank), int(port), out, body)


def _worker_gram(hp, layout, rank, res):
    for kind in GRAM_KINDS:
        case = gram_case(layout, kind)
        v, rw, of, d0 = shard(case, case["bounds"], rank)
        hp.upload_csc(case["V"], v, rw, of, doc_offset=d0, docs_global=case["D"])
        for b in GRAM_WIDTHS:
            res["g_%s_b%d" % (kind, b)] = hp.gram_apply(case["X"][b])
        res["g_%s_form" % kind] = np.array([hp.operator_form()])


def _worker_threshold(hp, layout, rank, res):
    A = th_corpus()
    cnt, rows, offs, d0 = shard(A, bounds(layout, A["D"]), rank)
    for tag, kw in (("th", {}), ("ths", dict(sample_rate=TH_RATE, sample_seed=TH_SEED))):
        hp.upload_counts(A["V"], cnt, rows, offs, doc_offset=d0, docs_global=A["D"])
        info = hp.threshold(TH_K, **kw)
        B = hp.get_B()
        for f in ("rows", "vals", "offs", "original_cols", "zetas"):
            res["%s_%s" % (tag, f)] = B[f]
        res["%s_meta" % tag] = np.array([hp.doc_offset, hp.D_global, hp.D, info["entries_above_threshold"], info["docs_kept"]], np.int64)


def _worker_ks(hp, name, rank, res):
    c = ks_case(name)
    B = c["B"]
    v, rw, of, d0 = shard(B, c["bounds"], rank)
    hp.upload_csc(B["V"], v, rw, of, doc_offset=d0, docs_global=B["D"])
    r = hp.compute_block_ks(c["nev"], blk=c["blk"], ncv=c["ncv"], maxit=KS_MAXIT, tol=KS_TOL, seed=KS_SEED, allow_noconv=True)
    res["ks_counts"] = np.array([r["rc"], r["nconv"], r["restarts"], r["napplies"]], np.int64)
    res["ks_evals"], res["ks_U"] = r["evals"], hp.get_U(c["nev"])


def _upload_km(hp, B, bnd, rank):
    v, rw, of, d0 = shard(B, bnd, rank)
    hp.upload_csc(B["V"], v, rw, of, doc_offset=d0, docs_global=B["D"])


def _worker_kmeans(hp, layout, rank, res):
    bnd = bounds(layout, KM_D)
    os.environ["ISLE_KMPP_TRACK"] = "0"
    # k-means++ on the corpus with the outlier: injected seeds (residual, min_dist), then free-running
    _upload_km(hp, km_corpus(True), bnd, rank)
    for k in KM_KS:
        c = km_ref(True, k)
        hp.set_U(c.U)
        g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
        res["pp%d_seeds" % k], res["pp%d_C" % k] = g["seeds"], g["C_lowd"]
        res["pp%d_res" % k], res["pp%d_rounds" % k] = np.array([g["residual"]], np.float64), np.array([g["rounds"]])
        res["pp%d_md" % k] = hp.get_min_dist() if hp.D else np.zeros(0, np.float32)
        f = hp.kmeans_init_on_projected_space(k, rng_seed=KM_FREE_SEED)
        res["fr%d_seeds" % k], res["fr%d_C" % k], res["fr%d_rounds" % k] = f["seeds"], f["C_lowd"], np.array([f["rounds"]])
    # both Lloyd loops on the row-constant corpus
    _upload_km(hp, km_corpus(False), bnd, rank)
    for k in KM_KS:
        c = km_ref(False, k)
        hp.set_U(c.U)
        g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
        res["c0_%d" % k] = g["C_lowd"]
        for tag, C0 in (("lp%d" % k, g["C_lowd"]), ("dg%d" % k, degenerate_start(c))):
            for r in range(1, KM_REPS + 1):
                lp = hp.run_lloyds_on_projected_space(k, C0, max_reps=r)
                res["%s_r%d_assign" % (tag, r)], res["%s_r%d_C" % (tag, r)], res["%s_r%d_it" % (tag, r)] = lp["assign"], lp["C_lowd"], np.array([lp["iters"]])
        last = res["lp%d_r%d_C" % (k, KM_REPS)]
        for r in range(1, KM_REPS + 1):
            lifted = hp.left_multiply_by_U(last)
            ls = hp.run_lloyds(k, max_reps=r)
            res["ls%d_r%d_assign" % (k, r)], res["ls%d_r%d_cen" % (k, r)], res["ls%d_r%d_it" % (k, r)] = ls["assign"], ls["centers"], np.array([ls["iters"]])
        res["ls%d_lift" % k] = lifted
    res["km_form"] = np.array([hp.operator_form()])
    if layout == "L2":  # k > 224: Lloyd in span(U) takes its first assignment and tile bounds from the tracked k-means++ rounds
        k = KM_KS[-1]
        c = km_ref(False, k)
        del os.environ["ISLE_KMPP_TRACK"]
        os.environ["ISLE_KMPP_SPARSE"] = "1"
        os.environ["ISLE_DEBUG_HAMERLY"] = "1"
        hp.set_U(c.U)
        for r in range(1, KM_REPS + 1):
            g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
            lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=r)
            res["tk%d_r%d_assign" % (k, r)], res["tk%d_r%d_C" % (k, r)], res["tk%d_r%d_it" % (k, r)] = lp["assign"], lp["C_lowd"], np.array([lp["iters"]])
        res["tk%d_c0" % k] = g["C_lowd"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher
# ---------------------------------------------------------------------------------------------------------------------------------
def launch(layout, tmp, env=None, timeout=rank_launch.LAUNCH_TIMEOUT_S, tag=""):
    """rank_launch.launch of the layout's (or the Krylov-Schur case's) ranks"""
    return rank_launch.launch(layout + tag, layout + tag, WORLD[layout], tmp, rank_launch.module_command("shard_cases", layout), env=env, timeout=timeout)
