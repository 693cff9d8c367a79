"""The compaction rule of isle_hip_infer_resident, restated in numpy for its tests (include/isle_hip.h)."""
import numpy as np


def expected_entries(W, llh, min_weight=None):
    """The compaction rule on dense weights: converged documents (llh.first != 0), W > min_weight in float (None: 1.0f / (float)k),
    topics ascending.  -> (offs int64, topic uint32, weight float32)."""
    k = W.shape[1]
    mw = np.float32(1.0) / np.float32(k) if min_weight is None or min_weight < 0 else np.float32(min_weight)
    keep = (W > mw) & (llh[:, 0] != 0)[:, None]
    offs = np.zeros(W.shape[0] + 1, np.int64)
    offs[1:] = np.cumsum(keep.sum(axis=1))
    d, t = np.nonzero(keep)   # row-major: documents ascending, topics ascending
    return offs, t.astype(np.uint32), W[d, t]
