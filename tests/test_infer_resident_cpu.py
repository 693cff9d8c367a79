"""isle_hip_infer_resident without a GPU: the new symbols are declared in the header and bound with matching arity, and the numpy
restatement of the compaction rule the GPU tests compare against does what include/isle_hip.h says on hand-made weights."""
import os
import re

import numpy as np

from infer_resident_rule import expected_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("isle_hip_infer_resident", "isle_hip_get_infer_entries", "isle_hip_avg_doc_sz")


def test_new_symbols_are_declared_and_bound_with_matching_arity():
    from isle_amd._lib import SYMBOLS
    header = open(os.path.join(ROOT, "include", "isle_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(SYMBOLS[name][1]), name
    assert len(SYMBOLS["isle_hip_infer_resident"][1]) == 16 and len(SYMBOLS["isle_hip_get_infer_entries"][1]) == 4


def test_python_entry_point_exists():
    import inspect
    from isle_amd import HotPath
    sig = inspect.signature(HotPath.infer_resident)
    assert list(sig.parameters)[1:] == ["model", "docs", "iters", "Lf", "min_weight", "chunk_docs", "fetch_entries"]
    assert sig.parameters["iters"].default == 15 and sig.parameters["Lf"].default == 10.0 and sig.parameters["chunk_docs"].default == 0


def test_compaction_rule_on_hand_made_weights():
    f = np.float32
    third = f(1.0) / f(3.0)                      # the default threshold at k = 3, as the driver forms it
    W = np.array([[third, np.nextafter(third, f(1)), np.nextafter(third, f(0))],   # equal: out, one ulp above: in, below: out
                  [0.5, 0.5, 0.0],                                                  # not converged: nothing
                  [np.nan, 0.9, third],                                             # NaN compares false
                  [0.0, 0.0, 0.0],
                  [0.2, 0.9, 0.4]], np.float32)
    llh = np.array([[-1, -1], [0, 0], [-2, -2], [-3, -3], [-0.5, -1]], np.float32)
    offs, topic, weight = expected_entries(W, llh)
    assert offs.dtype == np.int64 and offs.tolist() == [0, 1, 1, 2, 2, 4]
    assert topic.dtype == np.uint32 and topic.tolist() == [1, 1, 1, 2]                # ascending inside a document
    assert weight.tobytes() == np.array([W[0, 1], 0.9, 0.9, 0.4], np.float32).tobytes()
    assert expected_entries(W, llh, -0.25)[1].tolist() == topic.tolist()              # any negative value selects the default
    # the compare is in float: a double threshold between third and its float successor rounds to one of them first
    mid = (float(third) + float(np.nextafter(third, f(1)))) / 2 * (1 - 2.0 ** -40)   # rounds down to third
    assert f(mid) == third and expected_entries(W, llh, mid)[1].tolist() == topic.tolist()
    # 0.0: every positive weight of a converged document; equal to the threshold stays out; 2.0: nothing
    o0, t0, w0 = expected_entries(W, llh, 0.0)
    assert o0.tolist() == [0, 3, 3, 5, 5, 8] and t0.tolist() == [0, 1, 2, 1, 2, 0, 1, 2]
    o2, t2, w2 = expected_entries(W, llh, 2.0)
    assert not o2.any() and t2.size == 0 and w2.size == 0 and w2.dtype == np.float32
    # the default is 1.0f / (float)k, not the double 1 / k rounded differently
    for k in (3, 7, 100, 1000):
        assert f(1.0) / f(k) == np.float32(np.float32(1.0) / np.float32(k))
        Wk = np.full((1, k), f(1.0) / f(k), np.float32)
        assert expected_entries(Wk, np.array([[-1, -1]], np.float32))[1].size == 0    # uniform weights: no entry
