"""What a context keeps from call to call, and what voids it (isle_amd/csrc/resident_host.h): a sequence on a USED context must give what a
fresh context gives for the same inputs, bit for bit, and a call whose input was voided must refuse with its message.  A forgotten
invalidation raises no error; it shows here as a differing bit.

(a) U replaced (same k, another k) behind a full chain;  (b) P overwritten by Lloyd on B (explicit centres: the wide product of the LDS
form lands in the projection's buffer);  (c) a rewrite of A that is refused;  (d) catchwords for another k behind a topic model.  (a) and
(b) also at the two shapes where the copies of the projection exist (route_host.h route_gemm_tiles, route_want_a2, route_kmpp_plan):
k = 160 on 130 817 documents (512 tiles of 256 x 256: the assignment products read the split copy; k >= 160: the grouped projection
writes it by position) and k = 260 on 65 281 documents (512 tiles at two column tiles; k > 224: tile bounds, and the first assignment
the k-means++ rounds keep).  A new count matrix voiding the inference result, the document reports and the inference text is held by
test_gpu_infer_resident.py, test_gpu_doc_report.py and test_gpu_infer_text.py; a new B by test_gpu_upload.py."""
import re

import numpy as np
import pytest

import isle_amd
from isle_amd._lib import IsleHipError

pytestmark = pytest.mark.gpu

V = 2000
SHAPES = {"small": (10, 1000), "split160": (160, 130817), "split260": (260, 65281)}
_B, _FRESH = {}, {}


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s differs from the fresh context's" % what


def same_chain(got, want):
    assert got.keys() == want.keys()
    for name in want:
        same_bits(got[name], want[name], name)


def matrix(shape):
    if shape not in _B:
        from tools.synth import make_B
        if shape == "small":
            _B[shape] = make_B(V, 1000, 10, 3)
        else:
            if "wide" not in _B:
                _B["wide"] = make_B(V, 131000, 20, 7)
            W, D = _B["wide"], SHAPES[shape][1]
            n = int(W["offs"][D])
            _B[shape] = dict(V=V, D=D, vals=W["vals"][:n].copy(), rows=W["rows"][:n].copy(), offs=W["offs"][:D + 1].copy())
        assert shape == "small" or _B[shape]["D"] == SHAPES[shape][1]
    return _B[shape]


def basis(k, seed):
    """the Q factor of a random V x k matrix: no eigensolve"""
    return np.asfortranarray(np.linalg.qr(np.random.default_rng(seed).standard_normal((V, k)))[0], dtype=np.float32)


def upload(h, B):
    h.upload_csc(B["V"], B["vals"], B["rows"], B["offs"])


def chain(h, k, reps=3):
    """from the projection on: everything the k-means calls hand out"""
    out = dict(P=h.get_projection(k))
    g = h.kmeans_init_on_projected_space(k, rng_seed=5)
    out.update(seeds=g["seeds"], seed_rows=g["C_lowd"], min_dist=h.get_min_dist())
    lp = h.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=reps)
    ob = h.kmeans_objective(k, space="projected")
    out.update(proj_assign=lp["assign"], proj_centres=lp["C_lowd"], proj_sums=ob["sums"], proj_sizes=ob["sizes"])
    out["lifted"] = h.left_multiply_by_U(lp["C_lowd"])
    ls = h.run_lloyds(k, max_reps=reps)
    ob = h.kmeans_objective(k, space="word")
    out.update(assign=ls["assign"], centres=ls["centers"], sums=ob["sums"], sizes=ob["sizes"])
    return out


def fresh(shape, k=None):
    """chain() of a fresh context given B and the second basis of k columns: computed once, shared, never written"""
    k = SHAPES[shape][0] if k is None else k
    if (shape, k) not in _FRESH:
        h = isle_amd.HotPath(0)
        try:
            upload(h, matrix(shape))
            h.set_U(basis(k, 2))
            _FRESH[(shape, k)] = chain(h, k)
        finally:
            h.close()
    return _FRESH[(shape, k)]


@pytest.fixture
def used(request):
    """a context of its own that has run the whole chain under a first basis"""
    shape = request.param
    k = SHAPES[shape][0]
    h = isle_amd.HotPath(0)
    upload(h, matrix(shape))
    h.set_U(basis(k, 1))
    chain(h, k)
    yield shape, k, h
    h.close()


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("used", list(SHAPES), indirect=True)
def test_U_replaced_by_one_of_the_same_k(used, monkeypatch, capfd):
    shape, k, h = used
    h.run_lloyds_on_projected_space(k, fresh(shape)["seed_rows"], max_reps=2)  # the resident state is that of the loop in span(U)
    assert h.kmeans_objective(k, space="projected")["sizes"].sum() == SHAPES[shape][1]
    h.set_U(basis(k, 2))
    with pytest.raises(IsleHipError, match="the projection P of the resident partition was released"):
        h.kmeans_objective(k, space="projected")
    with pytest.raises(IsleHipError, match="no resident centres for the word space and k = %d" % k):
        h.kmeans_objective(k, space="word", assign=np.zeros(SHAPES[shape][1], np.uint32))
    same_bits(h.get_projection(k), fresh(shape)["P"], "P")
    with pytest.raises(IsleHipError, match="the projection P of the resident partition was released"):
        h.kmeans_objective(k, space="projected")  # P is there again, but it is not the one the loop ran on
    with pytest.raises(IsleHipError, match="lloyds_sparse: no device-resident centres for k = %d" % k):
        h.run_lloyds(k)  # (the refused call has already taken `assign` from the loop in span(U): "no resident partition" from here on)
    with pytest.raises(IsleHipError, match="no resident partition for the projected space and k = %d" % k):
        h.kmeans_objective(k, space="projected")
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    capfd.readouterr()
    same_chain(chain(h, k), fresh(shape))
    err = capfd.readouterr().err
    if shape != "small":  # the route the shape was chosen for: Lloyd on B's first assignment through the two-term product on the split copy
        assert re.search(r"the two-term pass left \d+ of %d rows open" % SHAPES[shape][1], err), err[-2000:]
    if shape == "split260":
        assert "[tile bounds, projected]" in err, err[-2000:]


def test_U_replaced_by_one_of_another_k():
    shape, k2 = "small", 7
    h = isle_amd.HotPath(0)
    try:
        upload(h, matrix(shape))
        h.set_U(basis(10, 1))
        chain(h, 10)
        h.set_U(basis(k2, 2))
        with pytest.raises(IsleHipError, match="U has 7 columns, k = 10"):
            h.kmeans_init_on_projected_space(10, rng_seed=5)
        with pytest.raises(IsleHipError, match="projected space needs U of k = 10 columns, U has 7"):
            h.kmeans_objective(10, space="projected")
        with pytest.raises(IsleHipError, match="lloyds_sparse: no device-resident centres for k = 10"):
            h.run_lloyds(10)
        same_chain(chain(h, k2), fresh(shape, k2))
    finally:
        h.close()


# ---- (b) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("used", list(SHAPES), indirect=True)
def test_P_overwritten_by_lloyd_on_B(used):
    shape, k, h = used
    want = fresh(shape)
    h.set_U(basis(k, 2))
    h.run_lloyds_on_projected_space(k, want["seed_rows"], max_reps=2)
    assert h.operator_form() == 1
    h.timing_enable(True)
    h.timing_reset()
    h.run_lloyds(k, centers=want["lifted"], max_reps=2)  # explicit centres: the first assignment's wide product is written into P
    with pytest.raises(IsleHipError, match="no resident partition for the projected space and k = %d" % k):
        h.kmeans_objective(k, space="projected")
    assert h.timing_get()["project"][1] == 0
    same_bits(h.get_projection(k), want["P"], "P")
    # it was made again, not read back: the product alone where the grouped projection wrote the split copy by position on its way, the
    # product and the transposed copy behind it at the small shape (api_kmeans.cpp ensure_P: a timed scope each)
    assert h.timing_get()["project"][1] == (2 if shape == "small" else 1)
    h.timing_enable(False)
    lp = h.run_lloyds_on_projected_space(k, want["seed_rows"], max_reps=3)
    same_bits(lp["assign"], want["proj_assign"], "proj_assign")
    same_bits(lp["C_lowd"], want["proj_centres"], "proj_centres")
    same_bits(h.kmeans_objective(k, space="projected")["sums"], want["proj_sums"], "proj_sums")


def test_lloyd_in_span_U_twice_on_the_seeds_of_one_kmeanspp_call(monkeypatch, capfd):
    """The first assignment the k-means++ rounds kept is used once: the second run on the same seeds computes its own, as a fresh context
    does that was given those centres without a k-means++ call before it."""
    shape = "split260"
    k = SHAPES[shape][0]
    monkeypatch.setenv("ISLE_KMPP_SPARSE", "1")  # every round through the thin products, which keep the nearest seeds
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    h1, h2 = isle_amd.HotPath(0), isle_amd.HotPath(0)
    try:
        for h in (h1, h2):
            upload(h, matrix(shape))
            h.set_U(basis(k, 2))
        g = h1.kmeans_init_on_projected_space(k, rng_seed=5)
        capfd.readouterr()
        h1.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=3)
        first = capfd.readouterr().err
        assert first.count("first assignment taken from the k-means++ rounds") == 1 and "first assignment computed" not in first, first[-2000:]
        again = h1.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=3)
        second = capfd.readouterr().err
        assert second.count("first assignment computed") == 1 and "taken from the k-means++ rounds" not in second, second[-2000:]
        alone = h2.run_lloyds_on_projected_space(k, g["C_lowd"], max_reps=3)
        for name in ("assign", "C_lowd", "iters"):
            same_bits(np.asarray(again[name]), np.asarray(alone[name]), name)
        same_bits(h1.kmeans_objective(k, space="projected")["sums"], h2.kmeans_objective(k, space="projected")["sums"], "proj_sums")
    finally:
        h1.close()
        h2.close()


# ---- (c), (d): the stages either side --------------------------------------------------------------------------------------------------
def counts():
    from tools.synth import Corpus
    if "A" not in _B:
        c = Corpus(V, 1000, 10, 3)
        _B["A"] = (c,) + tuple(c.A())
    return _B["A"]


def kmeans_side(h, k=10):
    r = h.compute_block_ks(k, seed=2)
    out = chain(h, k)
    out["evals"] = r["evals"]
    return out


def test_a_refused_rewrite_of_A_leaves_no_A_and_the_kmeans_side_as_it_was():
    c, cnt, rows, offs = counts()
    h1, h2 = isle_amd.HotPath(0), isle_amd.HotPath(0)
    try:
        for h in (h1, h2):
            h.upload_counts(V, cnt, rows, offs)
            h.threshold(10)
        with pytest.raises(IsleHipError, match="ingest_tdf: bad character on line 2"):
            h1.ingest_tdf(b"1 1 3\n2 x 1\n3 2 1\n", V, 1000)
        with pytest.raises(IsleHipError, match="get_A: no count matrix"):
            h1.get_A()
        with pytest.raises(IsleHipError, match="threshold: no count matrix uploaded"):
            h1.threshold(10)
        with pytest.raises(IsleHipError, match="catchwords: no count matrix uploaded"):
            h1.find_catchwords(10, 5, assign=np.zeros(h1.D, np.uint32))
        same_chain(kmeans_side(h1), kmeans_side(h2))  # B is still the thresholded one
        h1.upload_counts(V, cnt, rows, offs)           # and a good A is taken afterwards
        for a, b in zip(h1.get_A(), (cnt, rows, offs)):
            assert np.array_equal(a, b)
    finally:
        h1.close()
        h2.close()


def test_catchwords_for_another_k_void_the_topic_model():
    from oracle import oracle as O
    c, cnt, rows, offs = counts()
    D, k1, k2 = 1000, 10, 7
    h1, h2 = isle_amd.HotPath(0), isle_amd.HotPath(0)
    try:
        for h in (h1, h2):
            h.upload_counts(V, cnt, rows, offs)
            h.threshold(k1)
        planted = c.planted()[h1.get_B()["original_cols"].astype(np.int64)].astype(np.uint32)
        pairs = np.array([[0, 1], [2, 5]])
        h1.find_catchwords(k1, O.catchword_rank(D, k1), assign=planted)
        h1.construct_topic_model(k1, O.model_rank_threshold(D, k1), D)
        assert h1.doc_report_text("top_two") and h1.edge_topics(pairs).shape == (V, 2)

        def stage2(h):
            cw = h.find_catchwords(k2, O.catchword_rank(D, k2), assign=planted % k2)
            return dict(thresholds=cw["thresholds"], catch_topic=cw["catch_topic"], catch_report=h.doc_report_text("catchwords"))

        got, want = stage2(h1), stage2(h2)
        for what in ("topic_sums", "topic_sums_by_doc", "top_two"):
            with pytest.raises(IsleHipError, match="doc_report_text: run isle_hip_topic_model first"):
                h1.doc_report_text(what)
        with pytest.raises(IsleHipError, match="edge_topics: run isle_hip_topic_model first"):
            h1.edge_topics(pairs)
        with pytest.raises(IsleHipError, match=r"topic_model: run isle_hip_catchwords\(num_topics = 10\) first"):
            h1.construct_topic_model(k1, O.model_rank_threshold(D, k1), D)
        for h, out in ((h1, got), (h2, want)):
            tm = h.construct_topic_model(k2, O.model_rank_threshold(D, k2), D)
            out.update({n: tm[n] for n in ("model", "model_threshold", "top1", "top2", "dts_off", "dts_topic", "dts_val")})
            out["edges"] = h.edge_topics(pairs)
            for what in ("topic_sums", "topic_sums_by_doc", "top_two"):
                out[what] = np.frombuffer(h.doc_report_text(what), np.uint8)
            out["catch_report"] = np.frombuffer(out["catch_report"], np.uint8)
        # the model's columns are summed with float atomics (post.hip, post_model_acc_k): two runs of ONE context differ in the last bits, so
        # the model and what is mixed from it are held to the tolerance test_gpu_post.py holds the model to; everything else bit for bit
        for name in ("model", "edges"):
            np.testing.assert_allclose(got.pop(name), want.pop(name), rtol=2e-5, atol=1e-9, err_msg=name)
        same_chain(got, want)
    finally:
        h1.close()
        h2.close()
