"""One tdf file onto document shards on N > 1 ranks (HotPath.ingest_tdf_file_sharded under a communicator): the per-rank worker and its
launcher, in the manner of post_shard_cases.py.  No GPU needed to import this module; the worker alone opens the device.

A job is a world size: the worker of world N runs every text of tdf_shard_rule.SHARDED made for N ranks, one fresh process per rank on
GPU 0 over the host-staged transport, and stores per text what the rank holds: bounds, A, entries_read, nnz, the line counts.  World 1
runs every text through the single-rank ingest_tdf_file, and THRESHOLD_CASE on to the single-rank threshold: the references of the
device's own.  World AGREE_WORLD ends with a counting stream whose agree_tag differs from rank to rank.  The texts are files the launcher
writes before it starts the ranks."""
import os
import subprocess
import sys
import time

import numpy as np

import shard_cases as sc
import tdf_shard_rule as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_TIMEOUT_S = 60  # shard_cases.LAUNCH_TIMEOUT_S: room for four cold Python starts on a shared machine; a clean launch takes a few seconds (profiles/tdf_shard_certificate.md)
PIECE_BYTES = 64       # pieces far smaller than the texts: every range and every window meets many cuts
WORLDS = (1, 2, 3, 4)


def cases_of(world):
    return [c for c in tr.SHARDED if world == 1 or tr.SHARDED[c][0] == world]


def key(case, what):
    return "%s|%s" % (case, what)


def text_path(tmp, case):
    return os.path.join(tmp, "%s.tdf" % case)


WORKER = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
import tdf_shard_cases
tdf_shard_cases.worker_main(*sys.argv[1:])
''' % (ROOT, ROOT)


def _threshold(hp, res, case):
    info = hp.threshold(tr.THRESHOLD_K)
    B = hp.get_B()
    for f in ("rows", "vals", "offs", "original_cols", "zetas"):
        res[key(case, "th_%s" % f)] = B[f]
    res[key(case, "th_meta")] = np.array([hp.doc_offset, hp.D_global, hp.D, info["entries_above_threshold"], info["docs_kept"]], np.int64)


def worker_main(world, rank, port, tmp, out):
    world, rank, port = int(world), int(rank), int(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch.distributed as dist
    from isle_amd import HotPath, IsleHipError
    hp = HotPath(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    if world > 1:
        hp.comm_init_host(world, rank, HotPath.gloo_exchange(dist, world, rank))
    res = {}
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
    np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()
    hp.close()


def launch(world, tmp, timeout=LAUNCH_TIMEOUT_S):
    """One fresh process per rank, all under one time limit; a rank that fails ends the others; nothing is repeated.
    -> dict(ranks (the loaded .npz per rank), outputs, wall (seconds)); shard_cases.LaunchFailed otherwise."""
    assert 1 <= world <= 4
    for case in cases_of(world):
        with open(text_path(tmp, case), "wb") as f:
            f.write(tr.SHARDED[case][3])
    port = sc._free_port()
    procs, logs, outs = [], [], []
    t0 = time.monotonic()
    for r in range(world):
        out = os.path.join(tmp, "tdf_w%d_r%d.npz" % (world, r))
        outs.append(out)
        logs.append(open(os.path.join(tmp, "tdf_w%d_r%d.log" % (world, r)), "w+"))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER, str(world), str(r), str(port), tmp, out], stdout=logs[-1], stderr=subprocess.STDOUT))
    why = None
    try:
        live = list(range(world))
        while live and why is None:
            left = timeout - (time.monotonic() - t0)
            if left <= 0:
                why = "time limit of %d s" % timeout
                break
            try:
                procs[live[0]].wait(timeout=min(left, 0.2))
            except subprocess.TimeoutExpired:
                pass
            for r in list(live):
                rc = procs[r].poll()
                if rc is not None:
                    live.remove(r)
                    if rc != 0:
                        why = "rank %d ended with status %d" % (r, rc)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    wall = time.monotonic() - t0
    texts = []
    for f in logs:
        f.seek(0)
        texts.append(f.read())
        f.close()
    if why is not None:
        raise sc.LaunchFailed("tdf sharded, %d ranks: %s\n%s" % (world, why, "\n".join("--- rank %d\n%s" % (r, t[-2500:]) for r, t in enumerate(texts))))
    return dict(ranks=[dict(np.load(o)) for o in outs], outputs=texts, wall=wall)


def rank_arrays(ranks, case):
    """the arrays of one text, per rank, under the names certify_sharded takes"""
    return [{f: q[key(case, f)] for f in ("bounds", "cnt", "rows", "offs", "entries_read", "nnz", "lines_local", "lines_global")} for q in ranks]
