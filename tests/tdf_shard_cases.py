"""One tdf file onto document shards on N > 1 ranks (HotPath.ingest_tdf_file_sharded under a communicator): the per-rank worker, in the
manner of post_shard_cases.py (tests/rank_launch.py starts the ranks).  No GPU needed to import this module; the worker alone opens the device.

A job is a world size: the worker of world N runs every text of tdf_shard_rule.SHARDED made for N ranks, one fresh process per rank on
GPU 0 over the host-staged transport, and stores per text what the rank holds: bounds, A, entries_read, nnz, the line counts.  World 1
runs every text through the single-rank ingest_tdf_file, and THRESHOLD_CASE on to the single-rank threshold: the references of the
device's own.  World AGREE_WORLD ends with a counting stream whose agree_tag differs from rank to rank.  The texts are files the launcher
writes before it starts the ranks."""
import os

import numpy as np

import rank_launch
import tdf_shard_rule as tr

PIECE_BYTES = 64       # pieces far smaller than the texts: every range and every window meets many cuts
WORLDS = (1, 2, 3, 4)


def cases_of(world):
    return [c for c in tr.SHARDED if world == 1 or tr.SHARDED[c][0] == world]


def key(case, what):
    return "%s|%s" % (case, what)


def text_path(tmp, case):
    return os.path.join(tmp, "%s.tdf" % case)


def _threshold(hp, res, case):
    info = hp.threshold(tr.THRESHOLD_K)
    B = hp.get_B()
    for f in ("rows", "vals", "offs", "original_cols", "zetas"):
        res[key(case, "th_%s" % f)] = B[f]
    res[key(case, "th_meta")] = np.array([hp.doc_offset, hp.D_global, hp.D, info["entries_above_threshold"], info["docs_kept"]], np.int64)


def worker_main(rank, port, out, world, tmp):
    world = int(world)

    def body(hp, rank, world, res):
        from isle_amd import IsleHipError
        for case in cases_of(world):
            _, V, D, _ = tr.SHARDED[case]
            if world == 1:
                info = hp.ingest_tdf_file(text_path(tmp, case), V, D, _piece_bytes=PIECE_BYTES)
            else:
                info = hp.ingest_tdf_file_sharded(text_path(tmp, case), V, D, _piece_bytes=PIECE_BYTES)
                for f in ("bounds", "lines_local", "lines_global"):
                    res[key(case, f)] = np.asarray(info[f])
            res[key(case, "cnt")], res[key(case, "rows")], res[key(case, "offs")] = hp.get_A()
            res[key(case, "entries_read")], res[key(case, "nnz")] = np.asarray(info["entries_read"]), np.asarray(info["nnz"])
            if case == tr.THRESHOLD_CASE:
                _threshold(hp, res, case)
        if world == tr.AGREE_WORLD:  # the same bytes everywhere, another tag on every rank: all of them must leave with ISLE_E_COMM
            hp.tdf_begin_counts(9, 5, _piece_bytes=PIECE_BYTES)
            hp.tdf_write(b"1 1 1\n")
            try:
                hp.tdf_finalize_counts(world, agree_tag=1000 + rank)
                res["agree"] = np.array("")
            except IsleHipError as e:
                res["agree"] = np.array(str(e))
    rank_launch.run_rank(world, int(rank), int(port), out, body, comm_at_world_one=False)  # one rank: a context without a communicator


def launch(world, tmp, timeout=rank_launch.LAUNCH_TIMEOUT_S):
    """rank_launch.launch of the world's ranks, behind writing the texts they read"""
    for case in cases_of(world):
        with open(text_path(tmp, case), "wb") as f:
            f.write(tr.SHARDED[case][3])
    return rank_launch.launch("tdf sharded, %d ranks" % world, "tdf_w%d" % world, world, tmp, rank_launch.module_command("tdf_shard_cases", world, tmp), timeout=timeout)


def rank_arrays(ranks, case):
    """the arrays of one text, per rank, under the names certify_sharded takes"""
    return [{f: q[key(case, f)] for f in ("bounds", "cnt", "rows", "offs", "entries_read", "nnz", "lines_local", "lines_global")} for q in ranks]
