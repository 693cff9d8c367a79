"""Document-topic inference on the resident count matrix (isle_hip_infer_resident / isle_hip_get_infer_entries,
HotPath.infer_resident, ISLETrainer::output_doc_topic_weights).

The contract is equality with the certified path: for the same fp32 model and the same documents the resident path returns the bits
of HotPath.infer in top_topic, top_weight, llh and nconverged, and its entries are exactly {(d, t, W[d, t]) : converged(d),
W[d, t] > min_weight} of that call's dense weights W.  No tolerance appears anywhere; the fp64 certificate of
test_gpu_infer_certified.py covers the new path through this equality.  Inputs: infer_certificate.make_case (V = 1403, documents of
0 .. 513 kept words, an empty document, documents that do not converge)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import infer_certificate as ic
from infer_resident_rule import expected_entries
from isle_amd import HotPath, IsleHipError
from isle_amd.hot_path import entry_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "trainer_infer_main")
KS = (1, 3, 5, 7, 100, 200, 256, 257, 300, 1023, 1024)   # every instantiation of the dispatch, ld != k, tile edges of the pack kernel
DENSE = ("top_topic", "top_weight", "llh")
_REF = {}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def reference(hp, k):
    """HotPath.infer on the case of k, once per session; never modified."""
    if k not in _REF:
        case = ic.make_case(k)
        r = hp.infer(case["M"], case["offs"], case["rows"], case["counts"])
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[k] = (case, r)
    return _REF[k]


def load(hp, case):
    hp.upload_counts(case["M"].shape[0], case["counts"], case["rows"], case["offs"])
    return case["offs"].shape[0] - 1


def check(got, ref, lo=0, hi=None, min_weight=None):
    hi = ref["llh"].shape[0] if hi is None else hi
    for name in DENSE:
        assert bits(got[name]) == bits(ref[name][lo:hi]), name
    assert got["nconverged"] == int((ref["llh"][lo:hi, 0] != 0).sum())
    offs, topic, weight = expected_entries(ref["weights"][lo:hi], ref["llh"][lo:hi], min_weight)
    assert got["nentries"] == topic.shape[0]
    assert np.array_equal(got["offs"], offs) and got["offs"].dtype == np.int64
    assert np.array_equal(got["topic"], topic)
    assert bits(got["weight"]) == bits(weight)


@pytest.mark.parametrize("k", KS)
def test_bit_equality_with_the_host_path(hp, k):
    case, ref = reference(hp, k)
    D = load(hp, case)
    got = hp.infer_resident(case["M"])
    assert ref["nconverged"] == got["nconverged"] and 0 < got["nconverged"] < D   # the case holds both kinds of document
    assert got["avg_doc_sz"] == ref["avg_doc_sz"] == case["avg"]
    check(got, ref)
    conv = ref["llh"][:, 0] != 0
    assert (np.diff(got["offs"])[~conv] == 0).all() and (np.diff(case["offs"]) == 0).any()
    if k > 1:
        assert got["nentries"] > 0


def small_case(V, k):
    """A model whose rows differ in every column and a few documents over it, for any V >= 1."""
    rng = np.random.default_rng(31 * V + k)
    M = ((rng.random((V, k)) + 0.25) / max(V, 2)).astype(np.float32)   # columns sum to about one, never to exactly one (V = 1: log z != 0)
    docs = [np.sort(rng.choice(V, size=min(V, n), replace=False)).astype(np.uint32) for n in (1, 2, 5, 33, 64, 65, 200)]
    offs = np.zeros(len(docs) + 1, np.int64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    rows = np.concatenate(docs)
    return M, offs, rows, rng.integers(1, 6, size=rows.shape[0]).astype(np.float32)


@pytest.mark.parametrize("V", (1, 63, 64, 65, 1403))
@pytest.mark.parametrize("k", KS)
def test_pack_kernel_through_one_iteration(hp, V, k):
    # the packed model is not observable on its own: one iteration under it is, and every weight is an entry with min_weight = 0
    M, offs, rows, counts = small_case(V, k)
    ref = hp.infer(M, offs, rows, counts, iters=1)
    hp.upload_counts(V, counts, rows, offs)
    got = hp.infer_resident(M, iters=1, min_weight=0.0)
    assert got["nconverged"] > 0
    check(got, ref, min_weight=0.0)
    assert got["nentries"] == (ref["weights"][ref["llh"][:, 0] != 0] > 0).sum()


@pytest.mark.parametrize("k", (7, 300))
def test_results_do_not_depend_on_the_chunking(hp, k):
    case, ref = reference(hp, k)
    D = load(hp, case)
    for chunk in (1, 7, D - 1, D, D + 1, 0):
        check(hp.infer_resident(case["M"], chunk_docs=chunk), ref)
        check(hp.infer_resident(case["M"], chunk_docs=chunk, min_weight=0.0), ref, min_weight=0.0)


@pytest.mark.parametrize("k", (5, 257))
def test_document_ranges(hp, k):
    case, ref = reference(hp, k)
    D = load(hp, case)
    for lo, hi in ((0, 0), (3, 3), (5, D), (0, D), (2, 9)):
        got = hp.infer_resident(case["M"], docs=(lo, hi), chunk_docs=4)
        assert got["llh"].shape == (hi - lo, 2) and got["offs"].shape == (hi - lo + 1,) and got["offs"][0] == 0
        check(got, ref, lo, hi)
        if lo == hi:
            assert got["nentries"] == 0 and got["nconverged"] == 0


@pytest.mark.parametrize("k", (3, 200))
def test_min_weight(hp, k):
    case, ref = reference(hp, k)
    load(hp, case)
    conv = ref["llh"][:, 0] != 0
    check(hp.infer_resident(case["M"]), ref)                                   # negative -> 1.0f / (float)k
    check(hp.infer_resident(case["M"], min_weight=-3.0), ref)
    every = hp.infer_resident(case["M"], min_weight=0.0)
    check(every, ref, min_weight=0.0)
    assert every["nentries"] == (ref["weights"][conv] > 0).sum()
    none = hp.infer_resident(case["M"], min_weight=2.0)
    check(none, ref, min_weight=2.0)
    assert none["nentries"] == 0 and not none["offs"].any() and none["nconverged"] == conv.sum()
    # a threshold that IS one of the weights: strict >
    w = float(ref["weights"][conv].max())
    at = hp.infer_resident(case["M"], min_weight=w)
    check(at, ref, min_weight=w)
    assert at["nentries"] == 0
    # without the entries
    short = hp.infer_resident(case["M"], fetch_entries=False)
    assert "offs" not in short and short["nentries"] == expected_entries(ref["weights"], ref["llh"])[1].shape[0]


def test_two_identical_calls(hp):
    case, ref = reference(hp, 100)
    load(hp, case)
    a = hp.infer_resident(case["M"], chunk_docs=5)
    b = hp.infer_resident(case["M"], chunk_docs=5)
    for name in DENSE + ("offs", "topic", "weight"):
        assert bits(a[name]) == bits(b[name]), name
    assert (a["nconverged"], a["nentries"]) == (b["nconverged"], b["nentries"])
    check(b, ref)


def _empty_clusters(oc, c):
    a = (c.planted()[oc] % 4).astype(np.uint32)   # topics 0..3 populated, 4 with three documents, 5 empty
    a[:3] = 4
    return a


# the smallest trained pipeline of the post-stage tests; then one with an empty cluster, whose topic is a NaN column in both models (0 / 0)
@pytest.mark.parametrize("V,D,k,seed,assign_fn", [(1000, 8000, 10, 1, None), (2000, 6000, 6, 5, _empty_clusters)], ids=["plain", "empty-cluster"])
def test_resident_models_equal_the_host_path(hp, V, D, k, seed, assign_fn):
    from test_gpu_avg_model import setup_post
    s = setup_post(hp, V, D, k, seed, assign_fn)
    avg = hp.avg_topic_model(k)
    assert np.isnan(avg).any() == (assign_fn is not None)
    cnt, rows, offs = hp.get_A()
    a = hp.avg_doc_sz()
    for name, M in (("catch", s["catch"]), ("avg", avg)):
        ref = hp.infer(np.ascontiguousarray(M), offs, rows, cnt, avg_doc_sz=a)   # (V, k) row-major = the fetched model transposed
        got = hp.infer_resident(name, chunk_docs=2500)
        assert got["avg_doc_sz"] == a
        check(got, ref)       # whatever the host path does with a NaN column, the resident path does the same
        check(hp.infer_resident(name, docs=(17, 4001)), ref, 17, 4001)
        if assign_fn is None:
            assert got["nconverged"] > D // 2 and got["nentries"] >= got["nconverged"]


def test_refusals_leave_the_context_usable():
    case = ic.make_case(7)
    M = np.asfortranarray(case["M"])
    V, k = M.shape
    h = HotPath(0)
    try:
        def call(which=2, model=M, vocab=V, ncols=k, b=0, e=3, iters=15, Lf=10.0):
            nc, ne = C.c_uint64(), C.c_uint64()
            p = None if model is None else model.ctypes.data_as(C.c_void_p)
            return h._lib.isle_hip_infer_resident(h._h, which, p, vocab, ncols, b, e, iters, C.c_float(Lf), C.c_float(-1.0), 0, None, None, None,
                                                  C.byref(nc), C.byref(ne))

        E_ARG = call()   # no count matrix yet
        assert E_ARG != 0
        with pytest.raises(IsleHipError):
            h.infer_entries(3, 0)   # no entries before the first call
        D = load(h, case)
        good = h.infer_resident(case["M"])
        refused = [dict(b=4, e=3), dict(e=D + 1), dict(iters=0), dict(ncols=0), dict(ncols=1025), dict(vocab=V + 1), dict(model=None),
                   dict(which=0), dict(which=1), dict(which=7)]   # no catch / average model on this context; an unknown model
        for kw in refused:
            assert call(**kw) == E_ARG, kw
            assert h._lib.isle_hip_last_error(h._h)
        assert call(ncols=1025) == E_ARG and b"infer: num_topics = 1025 not in [1, 1024]" in h._lib.isle_hip_last_error(h._h)   # isle_hip_infer's words
        # the entries of the previous call are intact after a refusal ...
        off, tp, wt = h.infer_entries(D, good["nentries"])
        assert bits(off) == bits(good["offs"]) and bits(tp) == bits(good["topic"]) and bits(wt) == bits(good["weight"])
        # ... and the context works
        again = h.infer_resident(case["M"])
        for name in DENSE + ("offs", "topic", "weight"):
            assert bits(again[name]) == bits(good[name])
        load(h, case)   # a new A voids them
        with pytest.raises(IsleHipError):
            h.infer_entries(D, good["nentries"])
    finally:
        h.close()


def test_trainer_writes_doc_topic_weights(hp, tmp_path):
    from test_cli_cpu import write_tdf
    from tools.synth import Corpus
    V, D, k = 1500, 4000, 20
    counts, rows, offs = Corpus(V, D, k, seed=6).A()
    tdf = str(tmp_path / "corpus.tdf")
    write_tdf(tdf, counts, rows, offs)
    vocab = str(tmp_path / "vocab.txt")
    open(vocab, "w").write("\n".join("w%d" % i for i in range(V)))
    out = tmp_path / "out"
    out.mkdir()
    base = str(tmp_path / "dump")
    r = subprocess.run([EXE, tdf, vocab, str(out), str(V), str(D), str(k), base], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log_dir = glob.glob(str(out / "*"))[0]
    catch = np.fromfile(base + ".catch.f32", np.float32).reshape(V, k, order="F")
    hp.upload_counts(V, counts, rows, offs)
    got = hp.infer_resident(catch)
    doc = np.repeat(np.arange(D), np.diff(got["offs"]))
    text = "".join("%d\t%d\t%s\n" % (d + 1, t + 1, entry_text(w, "sparse")) for d, t, w in zip(doc, got["topic"], got["weight"]))
    assert got["nentries"] > D // 2
    assert open(os.path.join(log_dir, "DocTopicWeights.tsv"), "rb").read() == text.encode("ascii")
    diag = open(os.path.join(log_dir, "diagnosticLog.txt")).read()
    assert "Number of docs for which inference converged: %d (of %d)\n" % (got["nconverged"], D) in diag
