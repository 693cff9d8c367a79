"""The free k-means++ draw on document shards: what every rank of a layout runs (the worker, one process per rank over the host-staged
transport) and what the ranks' results are held to.  A plain module: importable without torch and without a GPU.

Exact cases of tests/kmpp_certificate.py (zeros-front-back, clustered-36, k-300, exhausted-37), so the ONE-RANK replay is the answer on every rank
with `==`: on several ranks the dice are `total x fraction` on the host, `die - my_off` is an integer taken from a double below 2^53, and
the owner of a die's interval searches its own prefix sums (api_kmeans.cpp kmpp_draw_by_ranks).

Layouts: L2 [0, ceil(D / 2), D] and L3 [0, 1, D, D] (a one-document shard and an empty last shard: holds_last is the middle rank).  For
k-300 the L2 cut is moved between two neighbouring seeds of the replay, so that one seed is the last document of shard 0 and the next the
first document of shard 1.  exhausted-37 ends at a zero total: no rank's interval holds the die 0, and the rank that holds the last
document answers D - 1 as the search's clamp does on one rank — on L3 the middle rank, behind which the last shard is empty."""
import numpy as np

import kmpp_certificate as kc
import rank_launch

LAYOUTS = ("L2", "L3")
WORLD = {"L2": 2, "L3": 3}
NAMES = ("zeros-front-back", "clustered-36", "k-300", "exhausted-37")
EDGE_CASE = "k-300"


def edge_cut(name):
    """the first document d such that d - 1 and d are both seeds of the replay"""
    s = np.sort(kc.expected(kc.ALL_CASES[name])["seeds"].astype(np.int64))
    adj = s[1:][np.diff(s) == 1]
    assert adj.size, "%s has no two neighbouring seeds" % name
    return int(adj[0])


def bounds(layout, name):
    D = kc.ALL_CASES[name]["D"]
    if layout == "L3":
        return np.array([0, 1, D, D], np.int64)
    return np.array([0, edge_cut(name) if name == EDGE_CASE else (D + 1) // 2, D], np.int64)


def worker_main(rank, port, out, layout):
    def body(hp, rank, world, res):
        for name in NAMES:
            case = kc.ALL_CASES[name]
            V, vals, rows, offs, U = kc.exact_inputs(case)
            bnd = bounds(layout, name)
            d0, d1 = int(bnd[rank]), int(bnd[rank + 1])
            o0, o1 = int(offs[d0]), int(offs[d1])
            hp.upload_csc(V, vals[o0:o1], rows[o0:o1], (offs[d0:d1 + 1] - o0).astype(np.int64), doc_offset=d0, docs_global=case["D"])
            hp.set_U(U)
            g = hp.kmeans_init_on_projected_space(case["k"], rng_seed=case["rng_seed"])
            res[name + "_seeds"], res[name + "_C"] = g["seeds"], g["C_lowd"]
            res[name + "_rounds"], res[name + "_residual"] = np.array([g["rounds"]]), np.array([g["residual"]], np.float32)
            res[name + "_md"] = hp.get_min_dist()
    rank_launch.run_rank(WORLD[layout], int(rank), int(port), out, body)


def launch(layout, tmp):
    return rank_launch.launch("kmpp " + layout, "kmpp_" + layout, WORLD[layout], tmp, rank_launch.module_command("kmpp_shard_cases", layout))


def certify(ranks, layout, name):
    """every rank's seeds, rounds, residual and C_lowd equal the one-rank replay; the ranks' min_dist side by side is the replay's"""
    case = kc.ALL_CASES[name]
    e = kc.expected(case)
    bnd = bounds(layout, name)
    for r, q in enumerate(ranks):
        what = "%s %s rank %d" % (layout, name, r)
        assert np.array_equal(q[name + "_seeds"], e["seeds"]), "%s: seeds %s, the replay's %s" % (what, q[name + "_seeds"][:12], e["seeds"][:12])
        assert int(q[name + "_rounds"][0]) == e["rounds"], what
        assert float(q[name + "_residual"][0]) == e["residual"], (what, float(q[name + "_residual"][0]), e["residual"])
        assert np.array_equal(q[name + "_C"], kc.exact_P(case)[e["seeds"].astype(np.int64)].astype(np.float32)), what
        assert len(q[name + "_md"]) == int(bnd[r + 1] - bnd[r]), what
    md = np.concatenate([q[name + "_md"] for q in ranks])
    assert np.array_equal(md.view(np.uint32), e["min_dist"].view(np.uint32)), "%s %s: min_dist side by side differs from the replay's" % (layout, name)
