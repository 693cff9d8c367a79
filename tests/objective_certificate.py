"""The k-means objective (isle_hip_kmeans_objective) stated in numpy and the bounds its outputs are held to.  All bounds are derived,
none measured:

  doc_dist[d] = max(0, |x_d - c_a(d)|^2) in fp64 on fp32 inputs.
    WORD (n_d entries, centre c over V words): the device sums V exact squares c_w^2 and n_d terms v_i^2 - 2 v_i c_{w_i} (two exact
      products, one rounded difference) and adds the two sums: at most n_d + V + 3 roundings of partial sums whose magnitudes never exceed
      M = |c|^2 + sum_i (v_i^2 + 2 |v_i c_{w_i}|), in whatever order.   |doc_dist - truth| <= (n_d + V + 3) 2^-52 M.
    PROJECTED (k coordinates): differences p_j - c_j rounded once, squared, summed:   <= (k + 2) 2^-52 sum_j (p_dj - c_j)^2.
  cluster_sums[t]: every distance is rounded to a multiple of q = 2^(ex - 53), ex the binary exponent (frexp) of the largest distance,
    and the multiples are summed exactly: the sum of its documents' bounds plus n_t q / 2; one final rounding to double is inside the
    documents' bounds (they grant 2^-52 of M per document, the conversion costs 2^-53 of the sum).  q is recomputed here from the largest
    value a distance may have (truth + bound), which is never below the device's q.
  total: the sum of the cluster bounds, and bit-equal to the clusters' sums added in ascending order.
  cluster_sizes: equal to bincount.  An empty cluster: exactly 0.

The truth is formed in extended precision (np.longdouble), so that its own rounding does not count against the bounds."""
import numpy as np

U52 = 2.0 ** -52
LD = np.longdouble


def word_truth(B, assign, centers):
    """-> (truth, bound) per document, WORD space.  B: CSC dict (V, vals, rows, offs), centers V x k (fp32 values), assign D."""
    V = int(B["V"])
    offs = np.asarray(B["offs"], np.int64)
    D = len(offs) - 1
    Cl = np.asarray(centers, np.float32).astype(LD)
    cn = (Cl * Cl).sum(axis=0)
    truth = np.zeros(D, LD)
    bound = np.zeros(D, np.float64)
    for d in range(D):
        s, e = offs[d], offs[d + 1]
        t = int(assign[d])
        v = np.asarray(B["vals"][s:e], np.float32).astype(LD)
        cw = Cl[np.asarray(B["rows"][s:e], np.int64), t]
        truth[d] = cn[t] + (v * v - 2 * v * cw).sum()  # = |x_d - c|^2: the words outside the document contribute c_w^2
        M = float(cn[t] + (v * v + 2 * np.abs(v * cw)).sum())
        bound[d] = (int(e - s) + V + 3) * U52 * M
    return np.maximum(truth, 0), bound


def proj_truth(P, assign, centers):
    """-> (truth, bound) per document, PROJECTED space.  P: D x k fp32 rows as the device holds them, centers k x k (rows = centres)."""
    Pl = np.asarray(P, np.float32).astype(LD)
    Cl = np.asarray(centers, np.float32).astype(LD)
    k = Cl.shape[1]
    x = Pl - Cl[np.asarray(assign, np.int64)]
    truth = (x * x).sum(axis=1)
    return truth, (k + 2) * U52 * truth.astype(np.float64)


def quantum(truth, bound):
    m = float((truth + bound).max()) if len(truth) else 0.0
    return 0.0 if m == 0.0 else 2.0 ** (np.frexp(m)[1] - 53)


def cluster_truth(truth, bound, assign, k):
    """-> (sums (longdouble), bounds, sizes) per cluster"""
    a = np.asarray(assign, np.int64)
    sizes = np.bincount(a, minlength=k)
    q = quantum(truth, bound)
    sums = np.zeros(k, LD)
    bnds = np.zeros(k, np.float64)
    np.add.at(sums, a, truth)
    np.add.at(bnds, a, bound)
    return sums, bnds + sizes * (q / 2), sizes


def certify(got, truth, bound, assign, k):
    """got: dict(sums, sizes, total[, doc_dist]) as HotPath.kmeans_objective returns it (doc_dist of ALL documents, ranks side by side).
    AssertionError names the first output outside its certificate; -> dict of the worst error / bound ratios."""
    sums_t, bnd_t, sizes = cluster_truth(truth, bound, assign, k)
    worst = {}
    if got.get("doc_dist") is not None:
        dd = np.asarray(got["doc_dist"], np.float64)
        assert dd.shape == truth.shape, "doc_dist has %r entries, the corpus %r documents" % (dd.shape, truth.shape)
        assert (dd >= 0).all(), "doc_dist[%d] is negative" % int(np.argmax(dd < 0))
        err = np.abs(dd.astype(LD) - truth).astype(np.float64)
        bad = err > bound
        assert not bad.any(), "doc_dist[%d] = %r, truth %r: off by %.3g, bound %.3g" % (
            int(np.argmax(bad)), dd[np.argmax(bad)], float(truth[np.argmax(bad)]), err[np.argmax(bad)], bound[np.argmax(bad)])
        worst["doc"] = float(np.max(err / np.where(bound > 0, bound, np.inf))) if len(err) else 0.0
    assert np.array_equal(np.asarray(got["sizes"], np.int64), sizes), "cluster_sizes differ from bincount"
    s = np.asarray(got["sums"], np.float64)
    assert s.shape == (k,)
    for t in np.flatnonzero(sizes == 0):
        assert s[t] == 0.0, "cluster %d is empty, its sum is %r" % (t, s[t])
    err = np.abs(s.astype(LD) - sums_t).astype(np.float64)
    bad = err > bnd_t
    assert not bad.any(), "cluster_sums[%d] = %r, truth %r: off by %.3g, bound %.3g" % (
        int(np.argmax(bad)), s[np.argmax(bad)], float(sums_t[np.argmax(bad)]), err[np.argmax(bad)], bnd_t[np.argmax(bad)])
    worst["cluster"] = float(np.max(err / np.where(bnd_t > 0, bnd_t, np.inf)))
    tot = 0.0
    for t in range(k):
        tot += float(s[t])
    assert got["total"] == tot, "total %r is not the clusters' sums added in ascending order (%r)" % (got["total"], tot)
    worst["total"] = certify_total(got["total"], truth, bound, assign, k)
    return worst


def certify_total(total, truth, bound, assign, k):
    """the total alone (a trace entry) -> its error / bound"""
    sums_t, bnd_t, _ = cluster_truth(truth, bound, assign, k)
    err, b = float(abs(LD(total) - sums_t.sum())), float(bnd_t.sum())
    assert err <= b, "total %r, truth %r: off by %.3g, bound %.3g" % (total, float(sums_t.sum()), err, b)
    return err / b if b > 0 else 0.0


def restate(truth, assign, k):
    """What a correct implementation returns, up to rounding: fp64 values of the truth, summed per cluster with one rounding (for the
    checker's own tests)."""
    a = np.asarray(assign, np.int64)
    dd = truth.astype(np.float64)
    sums = np.zeros(k, LD)  # the device adds the quantised distances exactly: a plain fp64 sum of n_t terms would not meet the bound
    np.add.at(sums, a, dd.astype(LD))
    sums = sums.astype(np.float64)
    tot = 0.0
    for t in range(k):
        tot += float(sums[t])
    return dict(sums=sums, sizes=np.bincount(a, minlength=k).astype(np.uint64), total=tot, doc_dist=dd)


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted cases (tests/test_gpu_kmeans_objective.py; restated on the host by tests/test_objective_certificate_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
CASE_V, CASE_D = 257, 333
CASE_KS = (1, 5, 65, 300)
CASE_LENGTHS = (0, 1, 63, 64, 65, 200)  # documents 0 .. 5: around the wave's width, and several strides
OUTLIER_DOC = 7
_CASES = {}


def case_corpus():
    """V = 257, D = 333: documents of 0, 1, 63, 64, 65 and 200 entries, the others of 2 .. 40; document 7 scaled by 64 (as
    shard_cases.KM_OUTLIER_SCALE does), so that it alone sets the exponent the distances are quantised by."""
    if "B" not in _CASES:
        rng = np.random.default_rng(5)
        lens = np.concatenate([CASE_LENGTHS, rng.integers(2, 41, CASE_D - len(CASE_LENGTHS))]).astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = np.concatenate([np.sort(rng.choice(CASE_V, n, replace=False)) for n in lens]).astype(np.uint32)
        vals = (0.05 + rng.random(int(offs[-1]))).astype(np.float32)
        vals[offs[OUTLIER_DOC]:offs[OUTLIER_DOC + 1]] *= np.float32(64.0)
        # document 4 (the one-member cluster's, its centre the document's bits): eighths, so that |c|^2 and the document's sum are exact
        # in fp64 in any order and cancel to exactly 0 (with other values the two orders leave a rounding residue of either sign)
        vals[offs[4]:offs[5]] = (rng.integers(1, 17, lens[4]) / 8.0).astype(np.float32)
        _CASES["B"] = dict(V=CASE_V, D=CASE_D, vals=vals, rows=rows, offs=offs)
    return _CASES["B"]


def dense_doc(B, d):
    x = np.zeros(int(B["V"]), np.float32)
    s, e = int(B["offs"][d]), int(B["offs"][d + 1])
    x[B["rows"][s:e]] = B["vals"][s:e]
    return x


def case_U(k):
    """Orthonormal columns as far as V allows; beyond (k = 300 > V = 257) unit columns: the objective asks nothing of U."""
    rng = np.random.default_rng(100 + k)
    Q = np.linalg.qr(rng.standard_normal((CASE_V, min(k, CASE_V))))[0]
    if k > CASE_V:
        R = rng.standard_normal((CASE_V, k - CASE_V))
        Q = np.concatenate([Q, R / np.linalg.norm(R, axis=0)], axis=1)
    return np.asfortranarray(Q, dtype=np.float32)


def case_partition(k, kind):
    """kind "crafted": a random partition with cluster k - 1 empty (k > 1), document 4 alone in cluster 1 (k >= 5) and the centres 2 and
    3 meant to be twins; "one": every document in cluster 0."""
    if kind == "one":
        return np.zeros(CASE_D, np.uint32)
    rng = np.random.default_rng(200 + k)
    a = rng.integers(0, max(k - 1, 1), CASE_D).astype(np.uint32)
    if k >= 5:
        a[a == 1] = 0
        a[4] = 1
    return a


def case_word_centers(k):
    """V x k, column-major: random non-negative centres; centre 1 = document 4's bits (its distance must be exactly 0), centres 2 and 3
    bit-identical."""
    B = case_corpus()
    C = np.asfortranarray((0.3 * np.random.default_rng(300 + k).random((CASE_V, k))).astype(np.float32))
    if k >= 5:
        C[:, 1] = dense_doc(B, 4)
        C[:, 3] = C[:, 2]
    return C


def case_proj_centers(k, P):
    """k x k, rows = centres, around the rows of P; centre 1 = row 4's bits, centres 2 and 3 bit-identical."""
    rng = np.random.default_rng(400 + k)
    C = (P[rng.integers(0, CASE_D, k)] + 0.1 * rng.standard_normal((k, k))).astype(np.float32)
    if k >= 5:
        C[1] = P[4]
        C[3] = C[2]
    return np.ascontiguousarray(C)
