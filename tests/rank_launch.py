"""What the multi-rank GPU tests share: the launcher of N rank processes, the worker's bootstrap and the module fixtures' rules (a
plain module; importable without torch and without a GPU: the bootstrap alone imports them).

The launcher is what decides what happens when a rank faults, aborts or hangs: one fresh process per rank, one time limit for the launch
as a whole, the first rank that fails ends the others (they would wait in a collective), nothing is repeated, and launch_each starts
nothing behind a launch that failed.  tests/test_rank_launch_cpu.py holds it to that with children that touch no GPU."""
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_TIMEOUT_S = 60  # slowest clean launch 4.3 s, four times that is 17 s; 60 leaves room for four cold Python starts on a shared machine (profiles/shard_certificate.md)


class LaunchFailed(Exception):
    pass


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(label, stem, world, tmp, command, env=None, timeout=LAUNCH_TIMEOUT_S):
    """One fresh process per rank (argv: command(rank, port, out)), all under one time limit; a rank that fails ends the others; nothing
    is repeated.  stdout and stderr of rank r go to <tmp>/<stem>_r<r>.log, out is <tmp>/<stem>_r<r>.npz.
    -> dict(ranks (the loaded .npz per rank), outputs (the log's text per rank), wall (seconds)); LaunchFailed otherwise."""
    assert 1 <= world <= 4
    port = free_port()
    procs, logs, outs = [], [], []
    t0 = time.monotonic()
    for r in range(world):
        out = os.path.join(tmp, "%s_r%d.npz" % (stem, r))
        outs.append(out)
        logs.append(open(os.path.join(tmp, "%s_r%d.log" % (stem, r)), "w+"))
        procs.append(subprocess.Popen(command(r, port, out), stdout=logs[-1], stderr=subprocess.STDOUT, env=dict(os.environ, **(env or {}))))
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
        raise LaunchFailed("%s: %s\n%s" % (label, why, "\n".join("--- rank %d\n%s" % (r, t[-2500:]) for r, t in enumerate(texts))))
    return dict(ranks=[dict(np.load(o)) for o in outs], outputs=texts, wall=wall)


STUB = r'''
import importlib, sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
importlib.import_module(sys.argv[1]).worker_main(*sys.argv[2:])
''' % (ROOT, ROOT)


def module_command(module, *args):
    """-> a command for launch: the child calls <module>.worker_main(rank, port, out, *args), every argument a string."""
    return lambda rank, port, out: [sys.executable, "-c", STUB, module, str(rank), str(port), out] + [str(a) for a in args]


def run_rank(world, rank, port, out, body, comm_at_world_one=True):
    """A rank's life: the context on GPU 0, gloo, the host-staged communicator, body(hp, rank, world, res), res to out."""
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch.distributed as dist
    from isle_amd import HotPath
    hp = HotPath(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    if world > 1 or comm_at_world_one:
        hp.comm_init_host(world, rank, HotPath.gloo_exchange(dist, world, rank))
    res = {}
    body(hp, rank, world, res)
    np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()
    hp.close()


def launch_each(jobs, failed):
    """jobs: (key, name, thunk), one thunk called after another -> {key: the thunk's result or its LaunchFailed}.  failed: the calling
    module's list of the launches that failed; while it holds one, nothing more is started."""
    out = {}
    for key, name, thunk in jobs:
        if failed:
            out[key] = LaunchFailed("not started: the launch %s failed" % failed[0])
            continue
        try:
            out[key] = thunk()
        except LaunchFailed as e:
            out[key] = e
            failed.append(name)
    return out


def ranks_of(launches, key):
    import pytest
    l = launches[key]
    if isinstance(l, Exception):
        pytest.fail(str(l), pytrace=False)
    return l["ranks"]


def write_report(lines, env_name):
    """the lines printed (shown with -s or on a failure) and written to the file os.environ[env_name] names, when set"""
    path = os.environ.get(env_name)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
