"""The k-means objective on document shards: what every rank of a layout computes (the worker, one process per rank over the host-staged
transport) and what the ranks' results are held to on the host.  A plain module: importable without torch and without a GPU.

Inputs, the same for every layout: shard_cases.km_corpus(True) (V = 403, D = 3001, the last document scaled by 64), for k = 65 and 300 a
fixed partition with an empty cluster cut at the layout's bounds, random word-space centres, and in span(U) the fp32 rows of P64 at the
injected seeds as centres.  The trace: Lloyd on B from the lifted seeds, three iterations, on the row-constant corpus."""
import numpy as np

import objective_certificate as oc
import rank_launch
import shard_cases as sc

LAYOUTS = ("W1", "L2", "L3", "L4", "LP")
WORLD = dict(sc.WORLD, W1=1)
KS = (65, 300)
TRACE_K, TRACE_REPS = 65, 3
SCALARS = ("sums", "sizes", "total")


def bounds(layout):
    B = sc.km_corpus(True)
    if layout == "W1":
        return np.array([0, B["D"]], np.int64)
    return sc.bounds(layout, B["D"], B["offs"])


def partition(k):
    """every cluster but the last, which stays empty on every rank"""
    return np.random.default_rng(500 + k).integers(0, k - 1, sc.KM_D).astype(np.uint32)


def word_centers(k):
    return np.asfortranarray((0.2 * np.random.default_rng(600 + k).random((sc.KM_V, k))).astype(np.float32))


def proj_centers(k, outlier=True):
    c = sc.km_ref(outlier, k)
    return np.ascontiguousarray(c.P64[c.seeds.astype(np.int64)].astype(np.float32))


def worker_main(rank, port, out, layout):
    def body(hp, rank, world, res):
        bnd = bounds(layout)
        d0, d1 = int(bnd[rank]), int(bnd[rank + 1])
        sc._upload_km(hp, sc.km_corpus(True), bnd, rank)
        for k in KS:
            hp.set_U(sc.km_ref(True, k).U)
            a = partition(k)[d0:d1]
            for space, C in (("word", word_centers(k)), ("projected", proj_centers(k))):
                got = hp.kmeans_objective(k, space, assign=a, centers=C, fetch_docs=True)
                tag = "%s%d" % (space[0], k)
                res[tag + "_sums"], res[tag + "_sizes"], res[tag + "_total"] = got["sums"], got["sizes"], np.array([got["total"]])
                res[tag + "_dd"] = got["doc_dist"]
            res["P%d" % k] = hp.get_projection(k)
        # the trace of a sharded Lloyd on B
        k = TRACE_K
        c = sc.km_ref(False, k)
        sc._upload_km(hp, sc.km_corpus(False), bnd, rank)
        hp.set_U(c.U)
        hp.left_multiply_by_U(proj_centers(k, False), fetch=False)
        hp.lloyds_trace(True)
        ls = hp.run_lloyds(k, max_reps=TRACE_REPS)
        hp.lloyds_trace(False)
        res["tr_obj"], res["tr_assign"], res["tr_centers"], res["tr_it"] = ls["objective"], ls["assign"], ls["centers"], np.array([ls["iters"]])
        got = hp.kmeans_objective(k, "word")
        res["tr_total"] = np.array([got["total"]])
    rank_launch.run_rank(WORLD[layout], int(rank), int(port), out, body)


def launch(layout, tmp):
    return rank_launch.launch("objective " + layout, "ob_" + layout, WORLD[layout], tmp, rank_launch.module_command("objective_shard_cases", layout))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def certify_replicated(ranks, single, tag):
    """sums, sizes and total: every rank's (a rank without documents too) bit-equal to the one-rank launch's"""
    for r, q in enumerate(ranks):
        for f in SCALARS:
            assert np.array_equal(bits(q["%s_%s" % (tag, f)]), bits(single["%s_%s" % (tag, f)])), "%s_%s of rank %d differs from the one-rank launch" % (tag, f, r)


def certify_side_by_side(ranks, single, tag, bnd):
    dd = sc.concat(ranks, tag + "_dd")
    for r, q in enumerate(ranks):
        assert len(q[tag + "_dd"]) == int(bnd[r + 1] - bnd[r])
    assert np.array_equal(bits(dd), bits(single[tag + "_dd"])), "%s: the ranks' doc_dist side by side are not the one-rank array" % tag


def certify_single(single, k):
    """the one-rank launch itself, within the certificate in both spaces -> worst ratios"""
    B = sc.km_corpus(True)
    a = partition(k)
    out = {}
    for space, tag in (("word", "w%d" % k), ("projected", "p%d" % k)):
        got = dict(sums=single[tag + "_sums"], sizes=single[tag + "_sizes"], total=float(single[tag + "_total"][0]), doc_dist=single[tag + "_dd"])
        tb = oc.word_truth(B, a, word_centers(k)) if space == "word" else oc.proj_truth(single["P%d" % k], a, proj_centers(k))
        out[tag] = oc.certify(got, tb[0], tb[1], a, k)
    return out


def certify_trace(ranks):
    """bit-identical on all ranks; its last entry is the objective of the run's final state (resident call) and lies within the
    certificate of that state -> (trace, error / bound of the last entry)"""
    tr = ranks[0]["tr_obj"]
    assert len(tr) == int(ranks[0]["tr_it"][0]) and len(tr) >= 1
    for r, q in enumerate(ranks):
        assert np.array_equal(bits(q["tr_obj"]), bits(tr)), "the trace of rank %d differs from rank 0's" % r
        assert np.array_equal(bits(q["tr_total"]), bits(tr[-1:])), "rank %d: the resident objective is not the last trace entry" % r
        assert np.array_equal(q["tr_centers"].view(np.uint32), ranks[0]["tr_centers"].view(np.uint32))
    a = sc.concat(ranks, "tr_assign")
    truth, bound = oc.word_truth(sc.km_corpus(False), a, ranks[0]["tr_centers"])
    return tr, oc.certify_total(float(tr[-1]), truth, bound, a, TRACE_K)
