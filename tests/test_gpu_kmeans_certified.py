"""Every document at every iteration of both Lloyd loops, in every form the switch table names for them, certified against fp64
(tests/kmeans_certificate.py), at the topic counts where the kernels change form.

The prefix method: a loop is run from one start with max_reps = 1, 2, ..., R.  Iteration r of the run with max_reps = r was computed
against the centres the run with max_reps = r - 1 returned, so its assignment is certified against those centres and its centres against
its assignment.  Lloyd in span(U) is bitwise reproducible, and so is Lloyd on B with a row-constant B (integer centroid counts): there the
prefix must be exact as well — a run that stopped early returns the previous run's bits.  The gather form of Lloyd on B (float sums of
perturbed values) is reproducible only up to rounding: the centres the run with max_reps = r used internally may differ in the last bits
from those the run with r - 1 returned, and the slack E of the assignment certificate covers that difference; its prefix is not compared
bit for bit.

U is a random orthonormal fp32 matrix set with set_U, so that the certificate does not depend on the eigensolver; one case takes the U of
compute_block_ks.  At k = 257 and k = 1000 the number of documents makes the assignment products take the bf16 route
(ceil(D / 256) ceil(k / 256) >= 512); ISLE_DEBUG_HAMERLY=1 shows that the route was taken and that the bounds pruned documents."""
import re

import numpy as np
import pytest

import kmeans_certificate as kc
from kmeans_certificate import FLOAT_SUMS_ROW_CONSTANT_FROB, certify_assignment, certify_centroids, certify_gemm, csc_points

pytestmark = pytest.mark.gpu

_CORPORA = {}
STATS = {}  # loop -> [largest gap / (E(c) + E(c*)), documents off the fp64 arg-min, documents certified]


@pytest.fixture(scope="module", autouse=True)
def certificate_margins(request):
    """At the end of the module: the largest gap / (E(c) + E(c*)) and the documents off the fp64 arg-min per loop, on the terminal, with or
    without -s."""
    yield STATS
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    for loop, (ratio, off, n) in sorted(STATS.items()):
        line = "k-means certificate, %s: largest gap / (E(c) + E(c*)) %.3g; %d of %d certified assignments off the fp64 arg-min" % (loop, ratio, off, n)
        if tr is not None:
            tr.write_line(line)
        assert ratio <= 1.0 and off <= n


def _note(loop, res):
    s = STATS.setdefault(loop, [0.0, 0, 0])
    s[0] = max(s[0], res["max_ratio"])
    s[1] += res["off"]
    s[2] += res["D"]


def _trim(B, D):
    n = int(B["offs"][D])
    return dict(V=B["V"], D=D, vals=B["vals"][:n].copy(), rows=B["rows"][:n].copy(), offs=B["offs"][:D + 1].copy())


def corpus(name):
    """small: V = 2003 (not a multiple of 4), D = 6001; big: V = 3001, D = 65601 (k = 257 on the bf16 route), its first 33001
    documents for k = 1000.  D is never a multiple of 64.  tiles511 / tiles512: V = 2003, D = 130 816 / 130 817 — at k <= 256 the
    assignment products have 511 / 512 tiles of 256 x 256, the edge of their bf16 form (route_host.h route_gemm_assign_fused_ok)."""
    if name not in _CORPORA:
        from tools.synth import make_B
        if name == "small":
            B = _trim(make_B(2003, 6100, 20, 3), 6001)
        elif name == "gather":  # perturbed values: the gather form of the operator
            B = dict(corpus("small"))
            B["vals"] = B["vals"] * (1.0 + 0.01 * np.random.default_rng(1).random(B["vals"].shape[0])).astype(np.float32)
        elif name == "big":
            B = _trim(make_B(3001, 66000, 50, 5), 65601)
        elif name == "tiles512":
            B = _trim(make_B(2003, 131000, 20, 7), 130817)
        elif name == "tiles511":
            B = _trim(corpus("tiles512"), 130816)
        else:
            B = _trim(corpus("big"), 33001)
        B["X"] = csc_points(B)
        _CORPORA[name] = B
    return _CORPORA[name]


def corpus_for(k):
    return corpus("big" if k == 257 else "big1000" if k == 1000 else "small")


_FP64 = {}  # the fp64 projection of the last (corpus, k, seed) only: the tests run grouped by k


def _dense_product(Xs, U64):
    """Xs (V, D) sparse: (D, dim) = Xs^T U64 over blocks of documents on the host's threads."""
    from concurrent.futures import ThreadPoolExecutor
    Xr = Xs.T.tocsr()
    spans = [(d0, min(Xr.shape[0], d0 + 4096)) for d0 in range(0, Xr.shape[0], 4096)]
    with ThreadPoolExecutor(16) as ex:
        return np.concatenate(list(ex.map(lambda s: np.asarray(Xr[s[0]:s[1]] @ U64), spans)), axis=0)


class Case:
    """B uploaded, a random orthonormal U (or a given one) set, the fp64 projection and its magnitudes |B|^T |U| (the last corpus, k and
    seed cached), and the rounding the device's fp32 projection of each document may carry."""

    def __init__(self, hp, B, k, seed=0, U=None):
        self.hp, self.B, self.k = hp, B, k
        hp.upload_csc(B["V"], B["vals"], B["rows"], B["offs"])
        key = (id(B), k, seed) if U is None and any(B is v for v in _CORPORA.values()) else None
        if key not in _FP64:
            if U is None:
                U = np.linalg.qr(np.random.default_rng(seed + 17 * k).standard_normal((B["V"], k)))[0]
            U = np.asfortranarray(U, dtype=np.float32)
            U64 = U.astype(np.float64)
            P64 = _dense_product(B["X"], U64)
            ent = (U, P64, _dense_product(abs(B["X"]), np.abs(U64)), np.einsum("ij,ij->i", P64, P64))
            if key is None:
                self.U, self.P64, self.Pabs, self.pn2 = ent
            else:
                _FP64.clear()
                _FP64[key] = ent
        if key is not None:
            self.U, self.P64, self.Pabs, self.pn2 = _FP64[key]
        self.Perr = ((np.diff(B["offs"]) + 1) * 2.0 ** -24)[:, None] * self.Pabs  # (nnz_d + 1) 2^-24 (|B|^T |U|)_d
        hp.set_U(self.U)
        self.seeds = np.sort(np.random.default_rng(seed + 1).choice(B["D"], k, replace=False)).astype(np.uint64)


PROJ_TAGS = ("hamerly, projected", "tile bounds, projected")
SPARSE_TAGS = ("yinyang", "hamerly")


def _bounded(err, D, tags):
    """(tag, iteration, active documents) of every bounded iteration reported with ISLE_DEBUG_HAMERLY=1 under one of the tags."""
    return [(t, int(i), int(n)) for t, i, n in re.findall(r"\[([^\]]+)\] iter (\d+) active (\d+) of %d\b" % D, err) if t in tags]


def _group_pruned(err, D):
    """Yinyang's group filter at work in an iteration from the second on: fewer groups scanned per active document than there are groups
    ('group scans n (x per active document, of G)'; by group: 'x per active document, of G' pairs beside the own group's scan, of G - 1)."""
    for it, x, G in re.findall(r"\[yinyang\] iter (\d+) active \d+ of %d; group scans \d+ \(([\d.]+) per active document, of (\d+)\)" % D, err):
        if int(it) >= 1 and float(x) < int(G):
            return True
    for it, x, G in re.findall(r"\[yinyang\] iter (\d+) active \d+ of %d; by group: \d+ pairs beside the own-group scans \(([\d.]+) per active "
                               r"document, of (\d+)\)" % D, err):
        if int(it) >= 1 and float(x) < int(G) - 1:
            return True
    return False


def _check_pruned(err, D, k, loop, tag=None):
    """The bounded iterations of one loop ran (under the form's tag where given) and some iteration from the second on skipped documents,
    or certifying them proves nothing about the bounds.  The second iteration often re-examines every document (the first update moves the
    centres far), so one pruning iteration is asked for, not all.  Lloyd in span(U) at k < 63: on a random U the projected documents are
    so evenly spread that its single Hamerly bound skips nothing in any iteration (k = 8 and 9: every document active in iterations 2 to
    6); there only the report of its bounded iterations is asserted.  Lloyd on B must prune at every k > 1: documents skipped whole, or
    with Yinyang bounds groups skipped (k = 9 from a start four projected iterations in: every centre moves more than 0.3 in every iteration,
    no document is skipped whole, and 1.4 of the 2 groups are scanned per active document)."""
    act = _bounded(err, D, PROJ_TAGS if loop == "projected" else SPARSE_TAGS)
    assert act, "no bounded iteration of %s was reported" % loop
    if tag is not None:
        assert {t for t, _, _ in act} == {tag}, {t for t, _, _ in act}
    if loop != "projected" or k >= 63:
        assert any(n < D for _, i, n in act if i >= 1) or (tag == "yinyang" and _group_pruned(err, D)), act
    return act


def projected_trajectory(c, C0, R, before=None, loop="projected", near_ties=False):
    hp, k = c.hp, c.k
    runs = []
    for r in range(1, R + 1):
        if before:
            before()
        runs.append(hp.run_lloyds_on_projected_space(k, C0, max_reps=r))
    C_in = C0
    for r, res in enumerate(runs, 1):
        if res["iters"] < r:  # stopped early: the previous run's bits
            prev = runs[r - 2]
            assert res["iters"] == prev["iters"], (r, res["iters"], prev["iters"])
            assert np.array_equal(res["assign"], prev["assign"])
            assert np.array_equal(res["C_lowd"].view(np.uint32), prev["C_lowd"].view(np.uint32))
            break
        _note(loop, certify_assignment(c.P64, c.pn2, C_in, res["assign"], what="%s k=%d iter %d:" % (loop, k, r), near_ties=near_ties))
        certify_centroids(c.P64, res["assign"], [q["assign"] for q in runs[:r - 1]], res["C_lowd"], X_abs=c.Pabs, X_err=c.Perr,
                          what="%s k=%d iter %d:" % (loop, k, r))
        C_in = res["C_lowd"]
    return runs


def sparse_trajectory(c, R, C0=None, lift_from=None, reproducible=True, loop="Lloyd on B", near_ties=False, frob_tol=1e-6):
    """C0: explicit (V, k) centres; lift_from: C_lowd lifted by left_multiply_by_U before every run (the projection route of the first
    assignment).  frob_tol: see FLOAT_SUMS_ROW_CONSTANT_FROB."""
    hp, k, X = c.hp, c.k, c.B["X"]
    runs, start = [], C0
    for r in range(1, R + 1):
        if lift_from is not None:
            lifted = hp.left_multiply_by_U(lift_from)
            if start is None:
                certify_gemm(c.U, lift_from.T, lifted, what="lift k=%d:" % k)
                start = lifted
            runs.append(hp.run_lloyds(k, max_reps=r))
        else:
            runs.append(hp.run_lloyds(k, centers=C0, max_reps=r))
    C_in = start
    for r, res in enumerate(runs, 1):
        if res["iters"] < r:
            if reproducible:
                prev = runs[r - 2]
                assert res["iters"] == prev["iters"]
                assert np.array_equal(res["assign"], prev["assign"])
                assert np.array_equal(res["centers"].view(np.uint32), prev["centers"].view(np.uint32))
            break
        _note(loop, certify_assignment(X, None, np.asarray(C_in).T, res["assign"], what="%s k=%d iter %d:" % (loop, k, r), near_ties=near_ties))
        certify_centroids(X, res["assign"], [q["assign"] for q in runs[:r - 1]], res["centers"].T, frob_tol=frob_tol,
                          what="%s k=%d iter %d:" % (loop, k, r))
        C_in = res["centers"]
    return runs


def certify_kmeanspp(c, g):
    """kmeans_certificate.certify_kmeanspp on this context's min_dist."""
    kc.certify_kmeanspp(c, g, c.hp.get_min_dist())


# 224 / 225: Hamerly's single bound / tile bounds in span(U) (route_host.h route_proj_plan); 248 / 249: 31 / 32 Yinyang groups, by document / by
# group on B (route_sparse_plan)
KS = [1, 7, 8, 9, 63, 64, 65, 224, 225, 248, 249, 255, 256, 257, 1000]


@pytest.mark.parametrize("k", KS)
def test_both_loops_iteration_by_iteration(hp, k, monkeypatch, capfd):
    """Lloyd in span(U) from k-means++ seeds (first assignment computed), then Lloyd on B from the lifted centres (first assignment
    through the projection) and from explicit centres (first assignment through the sparse product).  Centres placed on documents of a
    row-constant B hold many near-exact ties (distances are short sums of a few distinct values): the fp32 CPU oracle leaves 22 / 32 / 33
    documents off the fp64 arg-min at k = 7 / 65 / 256 in its first iteration, the library the same numbers, every gap within E.  Those
    starts allow the documents whose fp64 runner-up is within E besides the usual max(3, 3e-4 D)."""
    big = k >= 257
    c = Case(hp, corpus_for(k), k)
    D = c.B["D"]
    monkeypatch.setenv("ISLE_KMPP_TRACK", "0")
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    certify_kmeanspp(c, g)
    capfd.readouterr()
    R = 4 if big else 6
    runs = projected_trajectory(c, g["C_lowd"], R)
    err = capfd.readouterr().err
    if k > 1 and runs[-1]["iters"] >= 2:
        _check_pruned(err, D, k, "projected", "tile bounds, projected" if k > 224 else "hamerly, projected")
    if k == 1000:
        assert "the two-term pass left" in err
    sparse_trajectory(c, R, lift_from=runs[-1]["C_lowd"])
    err = capfd.readouterr().err
    if big:
        assert re.search(r"the two-term pass left \d+ of %d rows open" % D, err), err[-2000:]
    if k > 1:
        _check_pruned(err, D, k, "Lloyd on B", "yinyang")
    if not big:
        docs = np.asfortranarray(c.B["X"][:, c.seeds.astype(np.int64)].toarray().astype(np.float32))
        sparse_trajectory(c, R, C0=docs, near_ties=True)
    assert hp.operator_form() == 1


# Forms of Lloyd in span(U).  Tile bounds exist at k > 224 only (route_host.h, route_proj_plan: tiles = hamerly && k > 224 && ...), and ISLE_PROJ_BOUNDS,
# ISLE_PROJ_FULL and ISLE_PROJ_ACTIVE are read on that path alone (k_proj_full_by_gemm, k_proj_assign_tiles): at k = 9 and 65 they would
# rerun the default form, so they run at k = 257 and 1000.
PROJ_TILE_FORMS = [{"ISLE_PROJ_BOUNDS": "hamerly"}, {"ISLE_PROJ_FULL": "gemm"}, {"ISLE_PROJ_FULL": "fused"}, {"ISLE_PROJ_ACTIVE": "tiles"}]
PROJ_FORMS = PROJ_TILE_FORMS + [{"ISLE_PROJ_SUMS": "fresh"}, {"ISLE_NO_HAMERLY": "1"}]
# Forms of Lloyd on B.  Regrouping and the fused filter-and-tighten launch belong to the by-group Yinyang form, which the loop takes at
# k >= 249 (route_host.h, route_sparse_plan: yy_mode = ... G >= 32 ? 2 : 0; regroup = yinyang && yy_mode == 2 && ...): they run at k = 257 and 1000.
SPARSE_GROUP_FORMS = [{"ISLE_YY_FUSED": "0"}, {"ISLE_YY_REGROUP": "0"}]
SPARSE_FORMS = [{"ISLE_KMEANS_BOUNDS": "hamerly"}, {"ISLE_KMEANS_BOUNDS": "none"}, {"ISLE_YY_MODE": "doc"}, {"ISLE_YY_MODE": "docg"},
                {"ISLE_YY_MODE": "group"}, {"ISLE_YY_MOVERS": "0"}, {"ISLE_CENTERS_FRESH": "1"}, {"ISLE_FIRST_ASSIGN": "sparse"},
                {"ISLE_FIRST_ASSIGN": "projection"}] + SPARSE_GROUP_FORMS
# Forms of both loops: the assignment products, and the gather form of the operator on the row-constant B (ISLE_GRAM_LDS=0, read at the
# first use of the operator after the upload: the k-wide products through the row-gather kernels, float centroid sums, no movers).
BOTH_FORMS = [{"ISLE_GEMM_TERMS": "3"}, {"ISLE_GEMM_BF16X3": "0"}, {"ISLE_GEMM_EPILOGUE": "0"}, {"ISLE_GEMM_DMA": "0"}, {"ISLE_GRAM_LDS": "0"}]


def _fid(f):
    return ",".join("%s=%s" % (a[5:], b) for a, b in f.items())


FORM_CASES = [pytest.param(k, f, id="%d-%s" % (k, _fid(f))) for k in (9, 65, 257, 1000) for f in PROJ_FORMS + SPARSE_FORMS + BOTH_FORMS
              if k >= 257 or (f not in PROJ_TILE_FORMS and f not in SPARSE_GROUP_FORMS)]


@pytest.mark.parametrize("k,form", FORM_CASES)
def test_every_form(hp, k, form, monkeypatch, capfd):
    """Each switch of the table for the two loops, iteration by iteration, with its route shown by the debug report: the tag of the bounds
    that ran ([hamerly, projected] / [tile bounds, projected] / [yinyang] / [hamerly], none without bounds), pruning from the second
    iteration on, and the two-term bf16 product where the form takes it."""
    big = k >= 257
    c = Case(hp, corpus_for(k), k, seed=1)
    D = c.B["D"]
    for a, b in form.items():
        monkeypatch.setenv(a, b)
    monkeypatch.setenv("ISLE_KMPP_TRACK", "0")
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    gather = form == {"ISLE_GRAM_LDS": "0"}
    R = 3 if big else 4
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    capfd.readouterr()
    if form in SPARSE_FORMS:
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=2)
        start = lp["C_lowd"]
    else:
        if "ISLE_PROJ_FULL" in form:  # the first iteration is a full pass: through the bf16 product (gemm) or the register kernel (fused)
            hp.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=1)
            first = capfd.readouterr().err
            assert ("the two-term pass left" in first) == (form["ISLE_PROJ_FULL"] == "gemm"), first[-2000:]
        runs = projected_trajectory(c, g["C_lowd"], R, loop="projected")
        err = capfd.readouterr().err
        if form == {"ISLE_NO_HAMERLY": "1"}:
            assert not _bounded(err, D, PROJ_TAGS)
        else:
            tag = "tile bounds, projected" if big and form != {"ISLE_PROJ_BOUNDS": "hamerly"} else "hamerly, projected"
            _check_pruned(err, D, k, "projected", tag)
        # with tile bounds at k = 1000 the full passes go through the bf16 product by default (2 D k^2 >= 2e10)
        if k == 1000 and form in ({"ISLE_PROJ_ACTIVE": "tiles"}, {"ISLE_PROJ_SUMS": "fresh"}):
            assert "the two-term pass left" in err
        start = runs[-1]["C_lowd"]
    capfd.readouterr()
    if form not in PROJ_FORMS:
        sparse_trajectory(c, R, lift_from=start, reproducible=not gather, frob_tol=FLOAT_SUMS_ROW_CONSTANT_FROB if gather else 1e-6)
        err = capfd.readouterr().err
        bf16 = big and not (form.get("ISLE_GEMM_BF16X3") == "0" or form.get("ISLE_GEMM_EPILOGUE") == "0" or form.get("ISLE_GEMM_TERMS") == "3"
                            or form.get("ISLE_FIRST_ASSIGN") == "sparse" or form.get("ISLE_KMEANS_BOUNDS") in ("hamerly", "none"))
        if bf16:
            assert "the two-term pass left" in err, err[-2000:]
        if form.get("ISLE_KMEANS_BOUNDS") == "none":
            assert not _bounded(err, D, SPARSE_TAGS)
        else:
            _check_pruned(err, D, k, "Lloyd on B", "hamerly" if form.get("ISLE_KMEANS_BOUNDS") == "hamerly" else "yinyang")
    assert hp.operator_form() == (0 if gather else 1)


@pytest.mark.parametrize("k", [224, 225, 257, 1000])
def test_first_assignment_taken_from_kmeanspp_rounds(hp, k, monkeypatch, capfd):
    """At k > 224 Lloyd in span(U) may start from the nearest seeds and tile minima the k-means++ rounds kept instead of computing its
    first assignment (ISLE_KMPP_TRACK): certified like the computed one.  k = 224: the last k whose rounds keep nothing, computed."""
    c = Case(hp, corpus_for(k), k, seed=2)
    monkeypatch.setenv("ISLE_KMPP_SPARSE", "1")
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    holder = {}

    def before():
        holder["g"] = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)

    before()
    C0 = holder["g"]["C_lowd"]
    certify_kmeanspp(c, holder["g"])
    capfd.readouterr()
    projected_trajectory(c, C0, 3, before=before)
    err = capfd.readouterr().err
    assert err.count("first assignment taken from the k-means++ rounds") == (3 if k > 224 else 0), err[-2000:]
    assert err.count("first assignment computed") == (0 if k > 224 else 3), err[-2000:]


@pytest.mark.parametrize("D", [130816, 130817])
def test_assignment_product_at_512_tiles(hp, D, monkeypatch, capfd):
    """k = 64 on 511 / 512 tiles of 256 x 256: below, the first assignment of Lloyd on B through the projection is the f32 product and the
    pass over its D x k scratch; from 512 tiles on the two-term bf16 product with the epilogue inside, which reads the split copy the
    projection leaves.  k-means++, Lloyd in span(U) and Lloyd on B from the lifted centres on either side, and the route as the debug report
    shows it."""
    k = 64
    c = Case(hp, corpus("tiles512" if D == 130817 else "tiles511"), k, seed=3)
    assert c.B["D"] == D
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    certify_kmeanspp(c, g)
    runs = projected_trajectory(c, g["C_lowd"], 2)
    capfd.readouterr()
    sparse_trajectory(c, 2, lift_from=runs[-1]["C_lowd"])
    err = capfd.readouterr().err
    assert bool(re.search(r"the two-term pass left \d+ of %d rows open" % D, err)) == (D == 130817), err[-2000:]
    assert hp.operator_form() == 1


def test_projected_loop_on_the_eigensolvers_U(hp):
    k = 20
    B = corpus("small")
    hp.upload_csc(B["V"], B["vals"], B["rows"], B["offs"])
    hp.compute_block_ks(k, seed=1, allow_noconv=True)
    c = Case(hp, B, k, U=hp.get_U(k))
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    certify_kmeanspp(c, g)
    runs = projected_trajectory(c, g["C_lowd"], 6)
    sparse_trajectory(c, 5, lift_from=runs[-1]["C_lowd"])


@pytest.mark.parametrize("k", [9, 65])
def test_gather_form_of_lloyd_on_B(hp, k, monkeypatch):
    """Perturbed values: the gather form of the operator, float centroid sums (reproducible up to rounding only)."""
    c = Case(hp, corpus("gather"), k, seed=3)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    runs = projected_trajectory(c, g["C_lowd"], 4)
    sparse_trajectory(c, 5, lift_from=runs[-1]["C_lowd"], reproducible=False)
    assert hp.operator_form() == 0
    docs = np.asfortranarray(c.B["X"][:, c.seeds.astype(np.int64)].toarray().astype(np.float32))
    sparse_trajectory(c, 4, C0=docs, reproducible=False, near_ties=True)


def _degenerate_start(c):
    """Twins (bit-identical), a zero centre, centres exactly on documents, and two far-off centres whose clusters stay empty."""
    k = c.k
    C = c.P64[c.seeds.astype(np.int64)].astype(np.float32)  # on documents (the rows of P up to the projection's rounding)
    C[k - 1] = C[1]
    C[k - 2] = C[1]
    C[3] = 0.0
    far = 1e3 * float(np.abs(C).max())
    C[5] = far
    C[6] = -far
    return C


@pytest.mark.parametrize("k", [9, 65])
def test_degenerate_starts_and_empty_documents(hp, k):
    """Twins, a zero centre, centres on documents, clusters empty from the first iteration on, and empty document columns (their arg-min
    is the centre of smallest norm, the lower index among equals).  Such a start holds many documents at a near-tie: at k = 65 with centres
    on documents 9 documents are at an exact fp64 tie between centres that are not bit-identical and 19 within E, and the fp32 CPU oracle
    itself leaves 5 of 6001 off the fp64 arg-min in its first iteration, as the library does.  Off the arg-min are therefore allowed, beside
    the usual max(3, 3e-4 D), the documents whose fp64 runner-up is within E of their best; the gap of every one stays within E."""
    B0 = corpus("small")
    D0 = B0["D"]
    empty = np.array([0, 17, 2000, D0 - 1])
    lens = np.diff(B0["offs"])
    lens[empty] = 0
    keep = np.ones(B0["offs"][-1], bool)
    for e in empty:
        keep[B0["offs"][e]:B0["offs"][e + 1]] = False
    offs = np.zeros(D0 + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    B = dict(V=B0["V"], D=D0, vals=B0["vals"][keep], rows=B0["rows"][keep], offs=offs)
    B["X"] = csc_points(B)
    c = Case(hp, B, k, seed=4)
    rng = np.random.default_rng(k)
    c.seeds = np.sort(rng.choice(np.setdiff1d(np.arange(D0), empty), k, replace=False)).astype(np.uint64)
    C0 = _degenerate_start(c)
    runs = projected_trajectory(c, C0, 4, loop="projected", near_ties=True)
    a1 = runs[0]["assign"]  # afterwards the empty clusters' centres are zero: twins of each other at the origin
    assert not np.isin(a1, [5, 6, k - 2, k - 1]).any() and (a1 == 1).any()
    assert (a1[empty] == 3).all()  # the zero centre
    # Lloyd on B: explicit centres (documents, twins, zero, far off) and the same start lifted
    docs = np.asfortranarray(c.B["X"][:, c.seeds.astype(np.int64)].toarray().astype(np.float32))
    docs[:, k - 1] = docs[:, 1]
    docs[:, 3] = 0.0
    docs[:, 5] = 1e3 * docs.max()
    res = sparse_trajectory(c, 4, C0=docs, near_ties=True)
    a1 = res[0]["assign"]
    assert not np.isin(a1, [5, k - 1]).any() and (a1 == 1).any() and (a1[empty] == 3).all()
    sparse_trajectory(c, 4, lift_from=C0, near_ties=True)


def test_twins_in_different_yinyang_groups_after_regrouping(hp, capfd, monkeypatch):
    """k = 257 on the bf16 route: the by-group Yinyang form regroups the centres by the squared norms of the lifted columns (stable: equal
    norms keep their labels' order) into groups of eight.  A centre is copied over the one of largest norm so that the twins take the norm
    ranks 8 m + 7 and 8 m + 8 — groups m and m + 1 of the regrouped order — with a relative margin of 1e-3 to their neighbours, ten times
    the worst-case rounding of an fp32 norm over 3001 words, so that the device's order is this one.  The lower-numbered twin must take
    every document they tie on."""
    k = 257
    c = Case(hp, corpus_for(k), k, seed=5)
    g = hp.kmeans_init_on_projected_space(k, inject_seeds=c.seeds)
    C0 = g["C_lowd"].copy()

    def lifted_norms(C):
        L = hp.left_multiply_by_U(C).astype(np.float64)
        return L, np.einsum("ij,ij->j", L, L)

    _, n2 = lifted_norms(C0)
    order = np.argsort(n2, kind="stable")
    t = int(order[-1])
    rank = next(r for r in range(7, k - 9, 8)
                if n2[order[r - 1]] < n2[order[r]] * (1 - 1e-3) and n2[order[r + 1]] > n2[order[r]] * (1 + 1e-3))
    s = int(order[rank])
    C0[t] = C0[s]
    lifted, n2 = lifted_norms(C0)
    lo, hi = min(s, t), max(s, t)
    assert np.array_equal(lifted[:, lo].astype(np.float32).view(np.uint32), lifted[:, hi].astype(np.float32).view(np.uint32))
    pos = np.empty(k, np.int64)
    pos[np.argsort(n2, kind="stable")] = np.arange(k)
    assert (pos[lo], pos[hi]) == (rank, rank + 1) and rank % 8 == 7  # groups rank // 8 and rank // 8 + 1
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    capfd.readouterr()
    runs = sparse_trajectory(c, 3, lift_from=C0)
    err = capfd.readouterr().err
    assert "the two-term pass left" in err
    assert (runs[0]["assign"] == lo).any() and not (runs[0]["assign"] == hi).any()


LIFT_SHAPES = [(4097, 1), (4097, 31), (4097, 32), (4097, 33), (4097, 64), (4097, 100), (70001, 130), (262145, 257)]


@pytest.mark.parametrize("V,N", LIFT_SHAPES)
def test_lift_product_against_fp64(hp, V, N):
    """left_multiply_by_U (k_gemm_nn, gemm_f32.h) at each tile configuration of gemm_dispatch: 256 x 32, 256 x 64, 128 x 128, 256 x 128
    (>= 512 tiles), 256 x 256 (>= 1024 tiles).  K = 37 (not a multiple of 16), V not a multiple of 256."""
    K = 37
    rng = np.random.default_rng(V + N)
    offs = np.array([0, 2, 3, 5], np.int64)
    rows = np.array([0, V - 1, 5, 1, V - 2], np.uint32)
    hp.upload_csc(V, np.ones(5, np.float32), rows, offs)
    U = np.asfortranarray(rng.standard_normal((V, K)).astype(np.float32))
    hp.set_U(U)
    Cl = rng.standard_normal((N, K)).astype(np.float32)
    out = hp.left_multiply_by_U(Cl)
    certify_gemm(U, Cl.T, out, what="lift V=%d K=%d N=%d:" % (V, K, N))
