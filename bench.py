#!/usr/bin/env python3
"""bench.py — ISLE training hot path (truncated SVD + k-means) on MI355X.

    python bench.py --gpus N --steps K --warmup W
    N > 1, either form: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py
    --gpus N ...` (the launcher's RANK / WORLD_SIZE are used), or plain `python bench.py --gpus N ...`: with no launcher environment the
    script itself starts N fresh rank processes, one per GPU, before any torch / HIP call (launch_ranks), forwards rank 0's line and
    returns the worst exit status.  Fewer than N visible GPUs is an error unless ISLE_BENCH_REHEARSE=1.

A *step* is one pass of the hot path of ISLETrainer::train() (reference src/trainer.cpp:490-571) over the
device-resident thresholded matrix B: compute_block_ks -> kmeans_init_on_projected_space ->
run_lloyds_on_projected_space -> left_multiply_by_U -> run_lloyds, with the reference's hyper-parameters
(include/hyperparams.h).  Metric = docs/sec = (documents of all ranks) * steps / wall time, inputs already in
HBM when the timed region starts.  Workload for every N: BASELINE.json configs[2], the configuration the metric is quoted on —
ONE corpus of vocab 100k x 10M docs x ~1B nnz, k = 1000 (ncv = 2010, include/hyperparams.h:38-40).  It fits one MI355X (~110 GB of
288 GB), so N = 1 runs all of it on one GPU; at N > 1 it is column-sharded N ways (strong scaling: rank r holds documents
[r D/N, (r+1) D/N); Gram / centroid sums are all-reduced with RCCL inside libisle_hip.so).  `--workload c2` runs BASELINE
configs[1] (vocab 50k, 1M docs, ~100M nnz, k = 200; weak scaling at N > 1: 1M documents per rank).

A plain run does what the headline figure needs: it generates and uploads the input, warms up, times the steps and prints the line.
`--full` adds everything else the benchmark measures or checks, all of it outside the timed region: the per-family breakdown
`device_ms_per_step` / `roofline_by_family` (one more, untimed pass), the accuracy gate against the CPU oracle, the CPU baseline, the stages
either side of the path and, for the default workload at N = 1, the secondary runs ("secondary_c2", "secondary_c3shard", "full_cli_c2";
--no-secondary skips them).

Inside the timed region only the Gram-apply launches are bracketed by HIP events (the `roofline` object needs their average
duration over exactly those steps).

`--dump-outputs DIR` writes, after the timed steps, what the last timed step computed as DIR/<name>.npy (float32 / float64, a fixed seeded
sample where an output is large; dump_outputs).  The inputs depend on the arguments only, so two builds can be compared output for output.

One JSON line on stdout (rank 0).  See DESIGN.md §Measurement for the roofline arithmetic.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (vocab, docs, topics, generator seed)          BASELINE.json configs
    "c1": (10_000, 50_000, 50, 12345),     # configs[0] (reference's CPU-runnable case)
    "c2": (50_000, 1_000_000, 200, 2024),  # configs[1] (per rank: weak scaling at N > 1)
    "c3": (100_000, 10_000_000, 1000, 31337),      # configs[2], column-sharded over all ranks (strong scaling)  <- bench default, every N
    "c3shard": (100_000, 1_250_000, 1000, 31337),  # one GPU's share of configs[2] at N = 8
    "c3full": (100_000, 10_000_000, 1000, 31337),  # = c3 (the name earlier rounds' profiles use for the one-GPU run)
    "c4": (100_000, 10_000_000, 1000, 31337),      # configs[3]: importance sampling, sample_rate 0.1 (A on the device -> sampled B -> hot path)
    "c5": (100_000, 10_000_000, 1000, 31337),      # configs[4]: config 3 + catchwords + topic model + 5000 edge topics behind the hot path
    "c4small": (20_000, 200_000, 100, 7),          # the c4 / c5 flows at a size a test can run (tests/test_gpu_bench_contract.py)
    "c5small": (20_000, 200_000, 100, 7),
    "tiny": (2_000, 5_000, 10, 0),
}
CONFIG_INDEX = {"c1": 0, "c2": 1, "c3": 2, "c3full": 2, "c3shard": 2, "c4": 3, "c5": 4, "c4small": 3, "c5small": 4}
# workloads whose A goes to the device and is thresholded there (isle_hip_threshold), the CPU port's B being the checker:
# sample_rate = sampled_threshold_and_copy (src/sparseMatrix.cpp:1365-1435), edge_topics = max_edge_topics of train_edge_topics (src/trainer.cpp:673-685)
WORKLOAD_OPTS = {"c4": {"sample_rate": 0.1}, "c5": {"edge_topics": 5000}, "c4small": {"sample_rate": 0.1}, "c5small": {"edge_topics": 300}}

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense f32 matrix-core peak (v_mfma_f32_32x32x2_f32 ...); SURVEY 8(d) prices the dense contractions against it
SIGMA_GATE = 1e-4        # north_star: top-k singular values within 1e-4 relative error
PARTITION_GATE = 0.999   # k-means against the oracle from the same U and seeds (SURVEY 8c asks >= 0.99; near-ties are all that may differ)
BIG_NNZ = 400_000_000  # above this the CPU legs (accuracy, k-means sample, cpu_baseline) run on bounded samples
DUMP_BYTES_MAX = 64 << 20  # --dump-outputs: all files together
DUMP_DOCS = 1 << 19        # --dump-outputs: documents of the partitions (a fixed sample when B has more)
DUMP_WORDS = 2048          # --dump-outputs: rows of U and of the fetched centres (a fixed sample when the vocabulary is larger)
T_START = time.time()


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def dump_sample(n, m, seed):
    """A fixed, seeded sample of m of range(n) in ascending order (all of range(n) when n <= m)."""
    if n <= m:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(n, m, replace=False))


def dump_outputs(dirname, arrays):
    """--dump-outputs: arrays (name -> float32 / float64 array) as dirname/<name>.npy, at most DUMP_BYTES_MAX bytes in all."""
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BYTES_MAX:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (at most %d)" % (total, DUMP_BYTES_MAX))
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            raise SystemExit("bench.py: --dump-outputs: %s is %s, not float32 / float64" % (name, a.dtype))
        np.save(os.path.join(dirname, name + ".npy"), a)
    log("bench.py: wrote %d outputs of the last timed step (%d bytes) to %s" % (len(arrays), total, dirname))


def csc_columns(B, cols):
    """The CSC sub-matrix of B's columns `cols` (in that order)."""
    offs = B["offs"]
    lens = (offs[cols + 1] - offs[cols]).astype(np.int64)
    so = np.zeros(len(cols) + 1, np.int64)
    np.cumsum(lens, out=so[1:])
    idx = np.repeat(offs[cols] - so[:-1], lens) + np.arange(so[-1], dtype=np.int64)
    return dict(vals=B["vals"][idx], rows=B["rows"][idx], offs=so)


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def kmpp_draws(k):
    """Draws per k-means++ round (src/sparseMatrix.cpp:2183: 1 + ceil(sqrt(max(s - 5, 0))) draws when s seeds exist; the first seed is
    round-less).  Duplicate draws are skipped by the reference, so a round may add fewer centres than it draws: an upper bound per round."""
    s_, out = 1, []
    while s_ < k:
        c = 0
        while c < 1 + max(s_ - 5, 0) ** 0.5 and s_ + c < k:
            c += 1
        out.append(c)
        s_ += c
    return out


def family_rooflines(V, D, nnz, k, b, ncv, restarts, applies, kmpp_rounds, lp_iters, ls_iters, device_ms):
    """SURVEY 8(d)'s algorithmic bytes / flops of every kernel family of the step x the counts THIS run executed, over the family's
    device time (events around every launch, the untimed extra pass) and the bounding peak.  All figures are per step on this rank's
    shard.  `frac` = achieved / peak.  Families without a device time in this run are left out."""
    out = {}

    def put(name, bound, alg, ms, what):
        if not ms or ms <= 0:
            return
        if bound == "hbm":
            ach, peak, unit = alg / (ms * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
        else:
            ach, peak, unit = alg / (ms * 1e-3) / 1e12, MFMA_F32_PEAK_TFLOPS, "TFLOP/s"
        out[name] = {"bound": bound, "algorithmic_%s_per_step" % ("bytes" if bound == "hbm" else "flops"): alg, "device_ms_per_step": round(ms, 3),
                     "achieved": round(ach, 1), "peak": peak, "unit": unit, "frac": round(ach / peak, 4), "what": what}

    g = device_ms.get("gram_pass1", 0.0) + device_ms.get("gram_pass2", 0.0)
    put("gram", "hbm", applies * (8.0 * nnz + 8.0 * (D + 1) + 8.0 * V * b), g,
        "%d applications x (8 nnz + 8 (D+1) + 2*4 V b)" % applies)
    # expand steps: the first sweep orthogonalises against m = 2b, 3b, ... ncv - b basis columns, every restart sweep against k + b ... ncv - b
    ms_ = list(range(2 * b, ncv, b)) + restarts * list(range(k + b, ncv, b)) if k > b else []
    if len(ms_) + 1 != applies:  # a run that stopped early / ran extra sweeps: price the expands it made at the mean width
        ms_ = [sum(ms_) / max(len(ms_), 1)] * max(applies - 1, 0)
    put("ortho", "hbm", sum(16.0 * V * m + 16.0 * V * b for m in ms_), device_ms.get("ortho", 0.0),
        "%d expand steps x (4 (4 V m) + 16 V b), CGS2, m = basis width of the step" % len(ms_))
    put("project", "hbm", 8.0 * nnz + 4.0 * V * k + 4.0 * k * D, device_ms.get("project", 0.0), "P = U^T B once: 8 nnz + 4 V k + 4 k D")
    draws = kmpp_draws(k)[:kmpp_rounds] if kmpp_rounds > 0 else []
    put("kmpp", "hbm", sum(min(4.0 * k * D, 8.0 * nnz + 8.0 * (D + 1) + 4.0 * V * c) + 8.0 * D for c in draws), device_ms.get("kmpp", 0.0),
        "%d rounds x (min(4 k D, 8 nnz + 8 (D+1) + 4 V c) + 8 D), c = the round's draws" % len(draws))
    put("lloyd_proj", "mfma", lp_iters * 2.0 * D * k * k, device_ms.get("lloyd_proj", 0.0),
        "%d iterations x 2 D k^2 (the dense formulation SURVEY 8(d) scores).  Above 1 where the exact distance bounds skip most dense passes and the "
        "passes that run use the bf16 matrix cores (operands split in two / three bf16 terms): see frac_of_bf16_dense_peak" % lp_iters)
    if "lloyd_proj" in out:
        out["lloyd_proj"]["frac_of_bf16_dense_peak"] = round(out["lloyd_proj"]["achieved"] / 2500.0, 4)  # MI355X_MICROARCH.md: 2.5 PFLOP/s dense bf16
    put("sparse", "hbm", ls_iters * (16.0 * nnz + 8.0 * V * k), device_ms.get("sparse_assign", 0.0) + device_ms.get("sparse_update", 0.0),
        "%d iterations of Lloyd on B x (2 (8 nnz) + 2*4 V k)" % ls_iters)
    put("rotate", "mfma", (restarts + 1) * 2.0 * V * (ncv - b) * k, device_ms.get("rotate", 0.0),
        "%d Ritz rotations (every restart + the final extraction) x 2 V (ncv - b) k" % (restarts + 1))
    put("lift", "mfma", 2.0 * V * k * k, device_ms.get("lift", 0.0), "centres = U C: 2 V k^2")
    return out


def gram_kernel_sha16():
    """sha256 (first 16 hex digits) of the Gram-apply kernel's source text — isle_amd/csrc/gram_lds.hip from the banner of the apply kernel
    to the end of gl_apply_k — the key under which a counter pass in profiles/pmc_traffic.json stays valid."""
    import hashlib
    try:
        with open(os.path.join(ROOT, "isle_amd", "csrc", "gram_lds.hip")) as f:
            t = f.read()
        a, z = t.index("// the apply kernel (both passes)"), t.index("#undef GL_ROWS_N")
        return hashlib.sha256(t[a:z].encode()).hexdigest()[:16]
    except Exception:
        return None


def library_sources_sha16():
    """sha256 (first 16 hex digits) over the library's sources (isle_amd/csrc/*.hip, *.h, *.cpp, sorted by name): the key under which the
    whole-step counter pass profiles/r06_step_traffic_by_family.json stays valid."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "isle_amd", "csrc")
    try:
        for fn in sorted(os.listdir(d)):
            if fn.endswith((".hip", ".h", ".cpp")):
                h.update(fn.encode())
                with open(os.path.join(d, fn), "rb") as f:
                    h.update(f.read())
        return h.hexdigest()[:16]
    except Exception:
        return None


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher's environment: start N fresh rank processes of this script (one per GPU, RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set, rendezvous on 127.0.0.1) and wait for them.  The parent makes no torch or HIP
    call, before or after: the children are new processes, nothing is exec'ed from a process that holds the GPU.  Rank 0 inherits this
    process's stdout (its one JSON line is the result), the other ranks' stdout goes to stderr.  Returns the worst exit status.  No rank
    outlives the launcher: when one rank fails the others are given 30 s to notice (their collectives would wait for ever), a SIGTERM /
    SIGINT / SIGHUP that reaches only this process, an exception, or the overall deadline (ISLE_BENCH_DEADLINE_S, default 3300 s) end
    every live child by PID — terminate, then kill after 10 s."""
    import signal
    import socket
    import subprocess
    procs = []

    def end_children(grace=10.0):
        live = [p for p in procs if p.poll() is None]
        for p in live:
            try:
                p.terminate()
            except OSError:
                pass
        t_end = time.time() + grace
        for p in live:
            try:
                p.wait(timeout=max(0.0, t_end - time.time()))
            except subprocess.TimeoutExpired:
                try:
                    p.kill()
                except OSError:
                    pass
        for p in live:
            try:
                p.wait(timeout=10)
            except Exception:
                pass

    class _Signalled(Exception):
        pass

    def on_signal(signum, _frame):
        raise _Signalled(signum)

    old_handlers = {}
    for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        try:
            old_handlers[sg] = signal.signal(sg, on_signal)
        except (ValueError, OSError):
            pass
    deadline = time.time() + float(os.environ.get("ISLE_BENCH_DEADLINE_S", "3300"))
    # the rendezvous port: the listening socket stays open (SO_REUSEADDR on both sides lets rank 0's store bind the same port) until every
    # rank has been started, so that no other process can be handed the port in between
    s = socket.socket()
    s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    try:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=None if r == 0 else sys.stderr.fileno()))
        s.close()
        s = None
        log("bench.py launcher: started %d ranks (pids %s), rendezvous 127.0.0.1:%d" % (n, [p.pid for p in procs], port))
        first_failure = None
        while any(p.poll() is None for p in procs):
            for r, p in enumerate(procs):
                rc = p.poll()
                if rc not in (None, 0) and first_failure is None:
                    first_failure = time.time()
                    log("bench.py launcher: rank %d exited with status %d" % (r, rc))
            if first_failure is not None and time.time() - first_failure > 30:
                log("bench.py launcher: ending the remaining ranks 30 s after the first failure")
                end_children()
                break
            if time.time() > deadline:
                log("bench.py launcher: overall deadline reached (ISLE_BENCH_DEADLINE_S): ending all ranks")
                end_children()
                return 124
            time.sleep(0.2)
    except _Signalled as e:
        log("bench.py launcher: signal %d: ending all ranks" % e.args[0])
        end_children()
        return 128 + int(e.args[0])
    finally:
        if s is not None:
            s.close()
        end_children(grace=5.0)  # no-op when every rank has exited; an exception above must not leave ranks holding their GPUs
        for sg, h in old_handlers.items():
            try:
                signal.signal(sg, h)
            except (ValueError, OSError):
                pass
    worst = 0
    for p in procs:
        rc = p.returncode
        worst = max(worst, rc if rc >= 0 else 128 - rc)
    return worst


def main():
    # stdout carries exactly ONE line, the JSON result: libraries that write to file descriptor 1 on their own (Gloo reports its
    # connections there when a process group is created) are sent to stderr, the result goes to the saved descriptor
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="default: c3 = BASELINE.json configs[2] (one 10M-document corpus, k = 1000; sharded over the ranks at N > 1)")
    ap.add_argument("--full", action="store_true",
                    help="also the per-family breakdown, the accuracy gate, the CPU baseline, the side stages and the secondary runs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the short runs behind the default N = 1 run")
    ap.add_argument("--fetch-centers", action="store_true", help="also copy the final V x k centres to the host inside the timed step")
    ap.add_argument("--no-upstream", action="store_true", help="skip the (untimed-region) stages either side of the path")
    ap.add_argument("--blk", type=int, default=0, help="experiment: block size of the eigensolver (0 = the reference's 10)")
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process becomes the launcher (it has made no torch / HIP call and makes none)
        os.dup2(result_fd, 1)
        os.close(result_fd)
        sys.exit(launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and os.environ.get("ISLE_BENCH_HOLD_S"):  # tests/test_bench_launcher_cpu.py: ranks that stay alive until their launcher ends them
        time.sleep(float(os.environ["ISLE_BENCH_HOLD_S"]))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher's WORLD_SIZE is %d" % (args.gpus, world))
    if world > 1:
        # a collective that never completes ends the run after two minutes, not five (the library's default suits long host phases between
        # collectives; this script has none while collectives are pending), and the launcher then ends the other ranks
        os.environ.setdefault("ISLE_COMM_TIMEOUT_S", "120")
    if world > 1 and "OMP_NUM_THREADS" not in os.environ:  # the ranks share the node's cores (corpus generation, thresholding)
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        os.environ["OMP_NUM_THREADS"] = str(max(1, (os.cpu_count() or 8) // max(local_world, 1)))
    defaulted = args.workload is None
    if defaulted:
        args.workload = "c3"
    import torch
    if world > 1 and os.environ.get("ISLE_BENCH_REHEARSE") != "1":
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        ndev = torch.cuda.device_count()  # counts, does not initialise the device
        if ndev < local_world:
            raise SystemExit("bench.py: --gpus %d needs %d GPUs on this node, %d visible (ISLE_BENCH_REHEARSE=1 rehearses the N-rank flow on "
                             "GPU 0 through the host-staged test transport; its line is marked as not a measurement)" % (args.gpus, local_world, ndev))
    dist = None
    if world > 1:
        import torch.distributed as dist_
        dist = dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)  # host control plane only

    out = run(args, args.workload, rank, world, local_rank, dist, torch, args.steps, args.warmup, full=args.full, breakdown=args.full,
              dump_dir=args.dump_outputs)
    secondary = args.full and defaulted and world == 1 and not args.no_secondary
    if out is not None and secondary:
        # BASELINE configs[1] beside the headline, so that rounds stay comparable: a short run, hot path only
        try:
            sec = run(args, "c2", rank, world, local_rank, dist, torch, 3, 1, full=False)
            out["secondary_c2"] = {"workload": sec["config"]["workload"], "ms_per_step": sec["ms_per_step"], "value": sec["value"],
                                   "unit": "docs/sec", "steps": 3, "warmup": 1, "roofline_frac": sec["roofline"]["frac"],
                                   "avg_gram_apply_ms": sec["roofline"]["avg_launch_ms"]}
        except Exception as e:  # the headline line must not depend on the secondary run
            out["secondary_c2"] = {"error": repr(e)[:300]}
    if out is not None and secondary:
        # one GPU's share of configs[2] at N = 8 — the unit an 8-GPU step actually runs (1.25 M documents, the full vocabulary and k): its
        # step, its Gram apply and its latency chains (QR, EVD) are what the scaling curve is made of, so they are reported next to the headline
        try:
            sec = run(args, "c3shard", rank, world, local_rank, dist, torch, 3, 1, full=False)
            out["secondary_c3shard"] = {"workload": sec["config"]["workload"], "ms_per_step": sec["ms_per_step"], "value": sec["value"],
                                        "unit": "docs/sec", "steps": 3, "warmup": 1, "roofline_frac": sec["roofline"]["frac"],
                                        "avg_gram_apply_ms": sec["roofline"]["avg_launch_ms"], "device_ms_per_step": sec["device_ms_per_step"],
                                        "roofline_frac_by_family": {f: v["frac"] for f, v in sec["roofline_by_family"].items()}}
        except Exception as e:
            out["secondary_c3shard"] = {"error": repr(e)[:300]}
    if out is not None and secondary:
        # SURVEY 8(d)'s second figure: full ISLETrain wall time, tdf text in -> M_hat_catch_sparse out, at BASELINE configs[1]
        try:
            out["full_cli_c2"] = full_cli_leg("c2")
        except Exception as e:
            out["full_cli_c2"] = {"error": repr(e)[:300]}
    if out is not None:
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    log("[rank %d] done at %.1f s since start" % (rank, time.time() - T_START))
    failed_gate = None
    if out is not None:
        gate = out.get("accuracy", {}).get("gate")
        if gate is not None and not gate["passed"]:
            failed_gate = gate["failed"]
    if dist is not None:  # every rank leaves the same way: contexts closed (run), one last barrier, the process group torn down
        dist.barrier()
        dist.destroy_process_group()
    if failed_gate:
        log("bench.py: ACCURACY GATE FAILED: " + "; ".join(failed_gate))
        sys.exit(3)


def full_cli_leg(workload):
    """The reference's own command line on the device (drivers/ISLETrain.cpp:35-46 -> isle_amd/host/ISLETrain): the workload's corpus is
    written as tdf text + a vocabulary file under /dev/shm (or /tmp), the twelve-argument CLI runs once as a child process, its wall time
    and the stage times of its reference-format timerLog.txt (include/timer.h:62-85) are reported, the files are deleted."""
    import shutil
    import subprocess
    import tempfile
    from tools.synth import Corpus
    V, D, k, seed = WORKLOADS[workload]
    t0 = time.time()
    corp = Corpus(V, D, k, seed)
    text = corp.tdf_bytes()
    entries = int(corp.nnz_A)
    del corp
    base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * text.size + (1 << 30) else "/tmp"
    tmp = tempfile.mkdtemp(prefix="isle_cli_", dir=base)
    try:
        tdf = os.path.join(tmp, "corpus.tdf")
        text.tofile(tdf)
        tdf_bytes = int(text.size)
        del text
        vocab = os.path.join(tmp, "vocab.txt")
        with open(vocab, "w") as f:
            f.write("\n".join("w%d" % i for i in range(V)))
        outdir = os.path.join(tmp, "out")
        os.mkdir(outdir)
        t_prep = time.time() - t0
        cmd = [os.path.join(ROOT, "isle_amd", "host", "ISLETrain"), tdf, vocab, outdir, str(V), str(D), str(entries), str(k), "0", "0", "0", "0", "5000"]
        t1 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t1
        res = {"workload": "%s = BASELINE.json configs[%d]: vocab=%d, docs=%d, tdf entries=%d, num_topics=%d, sample=0, edge topics off"
                           % (workload, CONFIG_INDEX[workload], V, D, entries, k),
               "command": "isle_amd/host/ISLETrain <tdf> <vocab> <out> %d %d %d %d 0 0 0 0 5000 (tdf text %d bytes under %s, page cache warm)"
                          % (V, D, entries, k, tdf_bytes, base),
               "returncode": r.returncode, "wall_s": round(wall, 3), "docs_per_s": round(D / wall, 1) if r.returncode == 0 else None,
               "corpus_and_tdf_preparation_s": round(t_prep, 1)}
        if r.returncode != 0:
            res["stderr_tail"] = r.stderr[-400:]
            return res
        logdir = os.path.join(outdir, sorted(os.listdir(outdir))[0])
        stages = {}
        with open(os.path.join(logdir, "timerLog.txt")) as f:
            for ln in f:
                ln = ln.strip()
                if not ln.startswith(("Time for ", "Total time for ")) or "(user)" not in ln:
                    continue
                name = ln.split("..")[0].replace("Time for ", "").strip()
                sysw = ln.split("(user)")[1].strip().split("s(")[0]  # the "(sys)" column is wall-clock
                stages[name] = round(stages.get(name, 0.0) + float(sysw), 4)
        res["stages_s"] = stages
        res["output_files_bytes"] = {fn: os.path.getsize(os.path.join(logdir, fn)) for fn in sorted(os.listdir(logdir))}
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run(args, workload, rank, world, local_rank, dist, torch, steps, warmup, full, breakdown=True, dump_dir=None):
    """One workload: generate, upload, warm up, time `steps` steps; with breakdown=True also one more, untimed pass for the per-family
    device times; with full=True also the accuracy / CPU / side-stage legs; with dump_dir the outputs of the last timed step go there.
    Returns the result object on rank 0, None elsewhere."""
    from isle_amd import HotPath
    from tools.synth import Corpus, effective_cpus

    V, D_per, k, seed = WORKLOADS[workload]
    opts = WORKLOAD_OPTS.get(workload, {})
    sample_rate, edge_topics = float(opts.get("sample_rate", 0.0)), int(opts.get("edge_topics", 0))
    device_stage = bool(opts)
    strong = workload in ("c3", "c3full", "c4", "c5", "c4small", "c5small")
    doc_base = rank * D_per
    if strong:  # one corpus, documents [doc_base, doc_base + D_per) on this rank (the generator seeds every document by its global id)
        D_total = D_per
        doc_base = (D_total * rank) // world
        D_per = (D_total * (rank + 1)) // world - doc_base

    def allreduce_np(a):
        if dist is not None:
            t = torch.from_numpy(a)
            dist.all_reduce(t)
        return a

    # ---------------- synthetic input (not timed): planted-topic Zipf corpus -> thresholded B ------------
    t0 = time.time()
    corp = Corpus(V, D_per, k, seed, doc_base=doc_base)
    nnz_A = corp.nnz_A
    big = nnz_A > BIG_NNZ
    # stages either side of the path: run (outside the timed region) where the tdf text of the corpus is a sensible object — a
    # 1 B-line file is 15 GB of text (SURVEY §8d generates C3-C5 directly as CSC)
    upstream = full and world == 1 and not args.no_upstream and not big and not device_stage
    A_host = corp.A() if upstream else None
    tdf_text = corp.tdf_bytes() if upstream else None
    t_thr0 = time.time()
    planted_all = corp.planted() if full else None  # the accuracy leg's planted-topic agreement

    # ISLE_BENCH_REHEARSE=1: all ranks on GPU 0 with the host-staged test transport (RCCL refuses two ranks on one device).
    # For checking this script's N > 1 control flow on a one-GPU box only: the line it prints is marked and is not a measurement.
    rehearse = world > 1 and os.environ.get("ISLE_BENCH_REHEARSE") == "1"
    hp = HotPath(0 if rehearse else local_rank)
    if rehearse:
        hp.comm_init_host(world, rank, HotPath.gloo_exchange(dist, world, rank))
    elif world > 1:
        uid = [HotPath.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        hp.comm_init(world, rank, uid[0])
    elif os.environ.get("ISLE_FORCE_COMM") == "1":
        # one GPU, 1-rank RCCL communicator: this process has torch's bundled librccl / libamdhip64 mapped (they win the soname lookup when
        # libisle_hip.so is loaded after `import torch`), which is the pair an N > 1 run of this script uses — exercised here on one GPU
        hp.comm_init(1, 0, HotPath.comm_unique_id())

    stage_in = None
    D_A_total = WORKLOADS[workload][1] * (1 if strong else world)  # documents of A over all ranks (the metric's numerator)
    if device_stage:
        # configs[3] / [4]: the count matrix A goes to the device (views, no second host copy), normalize_docs + compute_thresholds +
        # (sampled_)threshold_and_copy run there (src/trainer.cpp:430-485), and the hot path runs on THAT B.  One rank: the CPU port of the
        # same stage (tools/synth_corpus.cpp) is the checker — B, the kept-document map and the thresholds must agree bit for bit.
        cntA, rowsA, offsA = corp.A_views()
        t1 = time.perf_counter()
        hp.upload_counts(V, cntA, rowsA, offsA, doc_offset=doc_base, docs_global=D_A_total)
        t_h2d = time.perf_counter() - t1
        hp.timing_enable(True)
        hp.timing_reset()
        t1 = time.perf_counter()
        info = hp.threshold(k, sample_rate=sample_rate, sample_seed=seed)
        hp.synchronize()
        t_thr_dev = time.perf_counter() - t1
        thr_dev_ms = hp.timing_get()["threshold"][0]
        hp.timing_enable(False)
        if full:  # the host copy of B serves the checks of the full run only
            B = hp.get_B()
            B["D"], B["nnz"] = int(B["D"]), int(B["nnz"])
        else:
            B = {"D": hp.D, "nnz": hp.nnz}
        stage_in = {"stage": "A on the device -> B (normalize_docs + compute_thresholds + %s, src/trainer.cpp:430-485)"
                             % ("sampled_threshold_and_copy, sample_rate %.2f" % sample_rate if sample_rate else "threshold_and_copy"),
                    "docs_A": int(D_per), "nnz_A": int(nnz_A), "docs_kept": info["docs_kept"], "nnz_kept": info["nnz_kept"],
                    "upload_A_wall_ms": round(t_h2d * 1e3, 1), "wall_ms": round(t_thr_dev * 1e3, 1), "device_ms": round(thr_dev_ms, 3)}
        if world == 1 and full:
            t1 = time.time()
            Bc = corp.threshold(k, free_A=True, sample_rate=sample_rate, sample_seed=seed)
            stage_in["cpu_port_ms"] = round((time.time() - t1) * 1e3, 1)
            stage_in["cpu_cores"] = effective_cpus()
            same = {x: bool(np.array_equal(B[x], Bc[x])) for x in ("vals", "rows", "offs", "original_cols", "zetas")}
            stage_in["identical_to_cpu_port"] = same
            del Bc
            if not all(same.values()):
                raise SystemExit("bench.py: the device's thresholded / sampled B differs from the CPU port's: %s" % same)
        del cntA, rowsA, offsA
    else:
        B = corp.threshold(k, free_A=True, allreduce=allreduce_np if dist is not None else None)
    # dominant planted topic of every column of B (the device numbers B's columns by their GLOBAL document, the port by the rank's own)
    planted = planted_all[B["original_cols"].astype(np.int64) - (doc_base if device_stage else 0)] if full else None
    t_thr_cpu = time.time() - t_thr0
    del corp, planted_all
    t_gen = time.time() - t0
    D_loc, nnz_loc = B["D"], B["nnz"]
    counts = np.zeros(world, np.int64)
    counts[rank] = D_loc
    allreduce_np(counts)
    doc_offset = int(counts[:rank].sum())
    D_glob = int(counts.sum())
    tot = np.array([nnz_loc, nnz_A], np.int64)
    allreduce_np(tot)
    nnz_glob = int(tot[0])
    docs_metric = D_A_total if device_stage else D_glob  # docs/sec counts the documents of the INPUT (config 4 keeps a tenth of them in B)
    log("[rank %d] %s corpus: V=%d docs=%d (global %d) nnz(A)=%d nnz(B)=%d  generated in %.1fs (%.1f s since start)" %
        (rank, workload, V, D_loc, D_glob, nnz_A, nnz_loc, t_gen, time.time() - T_START))

    if not device_stage:
        hp.upload_csc(V, B["vals"], B["rows"], B["offs"], doc_offset=doc_offset, docs_global=D_glob)
        log("[rank %d] B on the device at %.1f s since start" % (rank, time.time() - T_START))

    phase_wall = {"block_ks": 0.0, "kmeanspp": 0.0, "lloyd_projected": 0.0, "lift": 0.0, "lloyd_sparse": 0.0}

    def step(i, wall=True):
        t = [time.perf_counter()]
        if args.blk:
            r = hp.compute_block_ks(k, blk=args.blk, ncv=2 * k + args.blk, seed=1 + i, allow_noconv=True)
        else:
            r = hp.compute_block_ks(k, seed=1 + i, allow_noconv=True)
        t.append(time.perf_counter())
        g = hp.kmeans_init_on_projected_space(k, rng_seed=1 + i)
        t.append(time.perf_counter())
        lp = hp.run_lloyds_on_projected_space(k, g["C_lowd"])
        t.append(time.perf_counter())
        hp.left_multiply_by_U(lp["C_lowd"], fetch=False)
        t.append(time.perf_counter())
        # The trainer reads only the partition after this call (closest_docs, src/trainer.cpp:566-575; `centers` is not touched again), so
        # the V x k centres stay in device memory, as they do in isle_amd/host/ISLETrain.cpp.  --fetch-centers copies them to the host as
        # well (the PCIe-inclusive figure quoted in DESIGN.md section 7).
        ls = hp.run_lloyds(k, fetch_centers=args.fetch_centers)
        t.append(time.perf_counter())
        if wall:
            for j, name in enumerate(phase_wall):
                phase_wall[name] += t[j + 1] - t[j]
        return dict(ks=r, kmpp_rounds=g["rounds"], lp_iters=lp["iters"], ls_iters=ls["iters"], assign=ls["assign"], kmpp_C_lowd=g["C_lowd"],
                    lp_C_lowd=lp["C_lowd"], lp_assign=lp["assign"], centers=ls["centers"])

    def fence():
        hp.synchronize()
        if torch.cuda.is_available():
            torch.cuda.synchronize(0 if rehearse else local_rank)
        if dist is not None:
            dist.barrier()

    for i in range(warmup):
        tw = time.perf_counter()
        step(-1 - i, wall=False)
        log("[rank %d] warm-up step %d: %.2f s (%.1f s since start)" % (rank, i, time.perf_counter() - tw, time.time() - T_START))
    hp.timing_enable(2)  # events around the Gram-apply launches only (roofline); everything else runs as in production
    hp.timing_reset()
    fence()
    t0 = time.perf_counter()
    last = None
    step_assigns, step_wall = [], []
    for i in range(steps):
        ts = time.perf_counter()
        last = step(i)
        step_assigns.append(last["assign"])  # looked at behind the timed region
        step_wall.append(time.perf_counter() - ts)
        if big:
            log("[rank %d] step %d of %d done at %.1f s" % (rank, i + 1, steps, time.perf_counter() - t0))  # a line a minute for the watchdog
    fence()
    dt = time.perf_counter() - t0
    # every timed step must have produced a usable partition (the steps differ in their seeds): a run in which some seed's k-means
    # collapsed must not pass as a measurement
    step_nonempty, step_largest = [], []
    for a in step_assigns:
        sz = np.bincount(a, minlength=k).astype(np.int64)
        allreduce_np(sz)
        step_nonempty.append(int((sz > 0).sum()))
        step_largest.append(int(sz.max()))
    del step_assigns
    tm_gram = hp.timing_get()
    if dump_dir is not None:
        # what the last timed step handed its caller (the V x k centres only where --fetch-centers fetched them; U as isle_hip_get_U
        # returns it), before anything else runs on the device
        sizes_all = np.bincount(last["assign"], minlength=k).astype(np.int64)
        allreduce_np(sizes_all)
        if rank == 0:
            docs, words = dump_sample(D_loc, DUMP_DOCS, 1), dump_sample(V, DUMP_WORDS, 2)
            ks = last["ks"]
            outs = {"evals": ks["evals"].astype(np.float64),  # eigenvalues of B B^T (sigma^2)
                    "U_rows": np.ascontiguousarray(hp.get_U(k)[words]), "U_rows_index": words.astype(np.float64),
                    "kmeanspp_centers_lowd": last["kmpp_C_lowd"], "lloyd_projected_centers_lowd": last["lp_C_lowd"],
                    "assign_projected": last["lp_assign"][docs].astype(np.float32), "assign": last["assign"][docs].astype(np.float32),
                    "assign_index": docs.astype(np.float64), "cluster_sizes": sizes_all.astype(np.float64),
                    "counts": np.array([ks["rc"], ks["nconv"], ks["restarts"], ks["napplies"], last["kmpp_rounds"], last["lp_iters"],
                                        last["ls_iters"]], np.float64)}  # rc, nconv, restarts, applications, k-means++ rounds, Lloyd iterations
            if last["centers"] is not None:
                outs["centers_rows"] = np.ascontiguousarray(last["centers"][words])
            dump_outputs(dump_dir, outs)
    tm = None
    if breakdown:
        # per-family breakdown: one more pass, untimed, with events around every launch
        hp.timing_enable(1)
        hp.timing_reset()
        step(steps - 1, wall=False)  # the last timed step again (same seeds), so that the per-family device times describe a timed step
        fence()
        tm = hp.timing_get()
    hp.timing_enable(0)
    dtt = np.array([dt], np.float64)
    if dist is not None:
        t = torch.from_numpy(dtt)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(dtt[0])
    ms_per_step = 1e3 * dt / steps
    value = docs_metric * steps / dt

    # ---------------- roofline of the dominant sparse kernel family (Gram apply) --------------------------
    b = (args.blk or 10) if k > 10 else 1
    n_apply = tm_gram["gram_pass1"][1]  # events of the timed region
    t_apply_ms = (tm_gram["gram_pass1"][0] + tm_gram["gram_pass2"][0]) / max(n_apply, 1)
    # bytes per application = 8*nnz + 8*(D+1) + 2*4*V*b   (this rank's shard)
    alg_bytes = 8.0 * nnz_loc + 8.0 * (D_loc + 1) + 8.0 * V * b
    achieved = alg_bytes / (t_apply_ms * 1e-3) / 1e9 if n_apply else 0.0
    form = hp.operator_form()
    form_kernels = ("LDS-banded form: gl_pack_scale_k + gl_apply_k (pass 1) + gl_apply_k + gl_reduce_cm_k (pass 2)" if form == 1
                    else "gather form: seg_gather_k<3,false> (pass 1) + seg_gather_k<3,true> + reduce_chunks_k (pass 2)")
    # HBM bytes per application from the PMC counters: a committed measurement of this workload on this kernel form
    # (profiles/pmc_traffic.json, collected by tools/pmc_probe.py under rocprofv3 --pmc in passes of their own), or null with the reason
    traffic, traffic_note = None, None
    pmc_key = {"c3": "c3full"}.get(workload, workload)
    if world == 8 and workload in ("c3", "c3full") and WORKLOADS["c3shard"][1] * 8 == WORKLOADS[workload][1]:
        pmc_key = "c3shard"  # rank 0 of eight holds the documents of the c3shard workload (thresholded there on their own statistics): same launches within 0.1 %
    if world > 1 and pmc_key != "c3shard":
        traffic_note = "no counter pass exists for a %d-rank shard" % world
    elif form != 1:
        traffic_note = "profiles/pmc_traffic.json holds the LDS-banded form's counters; this run used the gather form"
    else:
        sha = gram_kernel_sha16()
        try:
            with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
                ent = json.load(f).get(pmc_key, {})
            traffic = ent.get("gram_apply_hbm_bytes_per_launch")
            if traffic is not None and ent.get("kernel_source_sha16") != sha:
                traffic, traffic_note = None, ("profiles/pmc_traffic.json['%s'] was collected on kernel source %s, this build's gl_apply_k is %s: stale, "
                                               "not reported" % (pmc_key, ent.get("kernel_source_sha16"), sha))
        except Exception:
            pass
        if traffic_note is None:
            traffic_note = ("profiles/pmc_traffic.json['%s'] (kernel source %s): rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over tools/pmc_probe.py at "
                            "this size" % (pmc_key, sha) if traffic is not None else "no counter pass committed for workload '%s'" % pmc_key)
    # HBM bytes of a whole step by kernel family, from the counter pass over one config-3 step (tools/r06_steppmc.sh), while it describes this build
    step_traffic = None
    if breakdown and workload in ("c3", "c3full") and world == 1:
        try:
            with open(os.path.join(ROOT, "profiles", "r06_step_traffic_by_family.json")) as f:
                st = json.load(f)
            if st.get("library_sources_sha16") == library_sources_sha16():
                step_traffic = {"hbm_bytes_per_step_by_family": st["hbm_bytes_per_step_by_family"], "source": "profiles/r06_step_traffic_by_family.json "
                                "(rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE over one step, separate passes; sources %s)" % st["library_sources_sha16"]}
            else:
                step_traffic = {"hbm_bytes_per_step_by_family": None, "source": "profiles/r06_step_traffic_by_family.json was collected on library sources %s, "
                                "this build is %s: stale, not reported" % (st.get("library_sources_sha16"), library_sources_sha16())}
        except Exception:
            pass
    roofline = {"bound": "hbm", "kernel": "gram_apply (Z = B(B^T X), b=%d) = %s" % (b, form_kernels),
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_note,
                "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": round(t_apply_ms, 4), "launches": n_apply}
    if breakdown:
        device_ms = {f: round(v[0], 3) for f, v in tm.items() if v[1]}  # the one untimed pass with events around every launch
        by_family = family_rooflines(V, D_loc, nnz_loc, k, b, (2 * k + b) if k > 10 else 2 * k + 10, last["ks"]["restarts"],
                                     last["ks"]["napplies"], last["kmpp_rounds"], last["lp_iters"], last["ls_iters"], device_ms)
        scopes_per_step = int(sum(v[1] for v in tm.values()))  # event-bracketed scopes (a scope may hold several launches; rocprof has the launch count)

    sizes = np.bincount(last["assign"], minlength=k).astype(np.int64)
    allreduce_np(sizes)
    if min(step_nonempty) < 0.5 * min(k, D_glob) or max(step_largest) > 0.5 * D_glob:
        raise SystemExit("bench.py: a timed step left a degenerate partition (fewest non-empty clusters %d of %d, largest cluster %d of %d documents)"
                         % (min(step_nonempty), k, max(step_largest), D_glob))
    cfg = {
        "workload": "synthetic planted-topic Zipf corpus (%s = BASELINE.json configs[%d]%s): vocab=%d, docs=%d (%d on rank 0), nnz(A)=%d, "
                    "nnz(B)=%d, num_topics=%d, %s; hot path = block-KS SVD + k-means++ + Lloyd(projected) + lift + Lloyd(sparse)%s"
                    % (workload, CONFIG_INDEX.get(workload, -1), ", all of it on one GPU" if strong and world == 1 else "", V, D_glob,
                       D_loc, int(tot[1]), nnz_glob, k,
                       "sample=1 sample_rate=%.2f: B keeps %d of the %d documents of A, docs/sec counts the %d" % (sample_rate, D_glob, D_A_total, D_A_total)
                       if sample_rate else "sample=0",
                       "; edge_topics=1 max_edge_topics=%d (catchwords + topic model + edge topics run behind the timed region: other_stages)" % edge_topics
                       if edge_topics else ""),
        "block_ks": {"nev": k, "ncv": 2 * k + 10, "blk": b, "tol": 1e-4, "maxit": 100,
                     "restarts": last["ks"]["restarts"], "applies": last["ks"]["napplies"], "nconv": last["ks"]["nconv"],
                     "converged": bool(last["ks"]["rc"] == 0 and last["ks"]["nconv"] == k)},
        "kmeans": {"kmpp_rounds": last["kmpp_rounds"], "lloyd_projected_iters": last["lp_iters"],
                   "lloyd_sparse_iters": last["ls_iters"], "nonempty_clusters": int((sizes > 0).sum()),
                   "over_all_timed_steps": {"fewest_nonempty_clusters": min(step_nonempty), "largest_cluster": max(step_largest),
                                            "slowest_step_ms": round(1e3 * max(step_wall), 1), "fastest_step_ms": round(1e3 * min(step_wall), 1)}},
        "parallelism": ("REHEARSAL (not a measurement): %d ranks sharing GPU 0, host-staged collectives" % world if rehearse
                        else "docs column-sharded x%d, RCCL all-reduce" % world if world > 1 else "single GPU"),
        "centers_fetched": bool(args.fetch_centers),
        # the two D x k x k dot-product matrices of the assignment steps (full pass of Lloyd in span(U), first assignment of Lloyd on B): which
        # matrix cores computed them — same rule as k_gemm_nn_assign (isle_amd/csrc/dense.hip); everything else of the path is plain f32
        "assignment_products": ("f32 (v_mfma_f32_32x32x2_f32)" if os.environ.get("ISLE_GEMM_BF16X3") == "0" or k < 64
                                or ((D_loc + 255) // 256) * ((k + 255) // 256) < 512
                                else "bf16x3 (both operands split in three bf16 terms, six of the nine partial products kept on v_mfma_f32_32x32x16_bf16, f32 "
                                     "accumulation; error against fp64 5.6e-8 of sum|a b| vs 8.6e-8 for the f32 matrix cores; gemm_bf16x3.h)"
                                if os.environ.get("ISLE_GEMM_TERMS") == "3" or os.environ.get("ISLE_GEMM_EPILOGUE") == "0" else
                                "bf16x2 then bf16x3 (two bf16 terms per operand first: three partial products, every distance within 8.2e-5 (|row|^2 + max |c|^2) "
                                "of the three-term value, bounds widened by that; the rows whose two smallest distances are closer than twice that — "
                                "0.06 % at config 3 — are run again with three terms (six products, error against fp64 5.6e-8 of sum|a b|): the assignment "
                                "is the three-term product's, bit for bit; gemm_bf16x3.h, dense.hip gemm_assign_two_pass)"),
    }
    out = {
        "metric": "docs/sec end-to-end ISLETrain (SVD+k-means), k=%d; top-k σ rel-err" % k,
        "value": round(value, 1),
        "unit": "docs/sec",
        "n_gpus": world,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "strong" if strong and world > 1 else "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": cfg,
        "roofline": roofline,
        "host_wall_ms_per_step": {n: round(v * 1e3 / steps, 3) for n, v in phase_wall.items()},
    }
    if breakdown:
        out.update(roofline_by_family=by_family, step_traffic=step_traffic, device_ms_per_step=device_ms, timed_scopes_per_step=scopes_per_step)
    if stage_in is not None:
        out["other_stages"] = {"note": "stage upstream of the hot path, run on the device OUTSIDE the timed region at the workload's own size", "input": stage_in}
    if not full:
        hp.close()
        return out if rank == 0 else None

    # ---------------- accuracy (outside the timed region) -----------------------------------------------------------------
    # sigma: |lambda_i - lambda_true| <= ||A u_i - lambda_i u_i||  =>  sigma rel-err <= resid_i / (2 lambda_i), with A u_i computed by the
    # CPU oracle's operator (an independent implementation: a self-consistent but wrong HIP operator would not pass).  Small inputs on
    # one GPU: all k Ritz pairs; otherwise 48 pairs spread over the spectrum (the leading 16, the trailing 8 — the last to converge —
    # and 24 in between); several ranks: each rank applies its shard on the CPU, partial products are summed.
    from oracle.oracle import OracleCsc
    ev = last["ks"]["evals"].astype(np.float64)
    U = hp.get_U(k)
    t_acc0 = time.time()
    o_full = OracleCsc(V, D_loc, B["vals"], B["rows"], B["offs"])
    if world == 1 and not big:
        pick = np.arange(k)
    else:
        pick = np.unique(np.concatenate([np.arange(min(16, k)), np.arange(max(k - 8, 0), k), np.linspace(0, k - 1, 24).astype(np.int64)]))
    resid = np.empty(len(pick))
    for j0 in range(0, len(pick), 50):
        cols = pick[j0:j0 + 50]
        AU = o_full.gram_apply(np.asfortranarray(U[:, cols])).astype(np.float64)
        if dist is not None:
            AU = np.ascontiguousarray(AU)
            allreduce_np(AU)
        resid[j0:j0 + len(cols)] = np.linalg.norm(AU - U[:, cols].astype(np.float64) * ev[cols], axis=0) / ev[cols]
    ortho = float(np.abs(U[:, :min(k, 200)].astype(np.float64).T @ U[:, :min(k, 200)] - np.eye(min(k, 200))).max())
    t_acc = time.time() - t_acc0
    log("[rank %d] accuracy leg: %.1f s" % (rank, t_acc))
    # k-means quality of the timed run's partition: agreement with the planted dominant topics (majority label per cluster; the
    # reference itself reaches 0.81-0.87 on this kind of corpus)
    maj = np.zeros((k, k), np.int64)
    np.add.at(maj, (last["assign"].astype(np.int64), planted.astype(np.int64) % k), 1)
    allreduce_np(maj)
    purity = float(maj.max(1).sum() / max(D_glob, 1))

    if rank != 0:
        hp.close()  # the communicator and the device memory go here, not whenever the interpreter gets to it
        return None

    # ---------------- k-means parity on a sub-sample: the HIP path and the CPU oracle from the same U and the same injected seeds ------
    km = None
    if world == 1 and not args.no_cpu_baseline:
        from oracle.oracle import lift
        n_sub = min(D_loc, 50_000 if k <= 200 else 30_000)
        cols = np.sort(np.random.default_rng(7).choice(D_loc, n_sub, replace=False)) if n_sub < D_loc else np.arange(D_loc)
        Bs = csc_columns(B, cols)
        o_sub = OracleCsc(V, n_sub, Bs["vals"], Bs["rows"], Bs["offs"])
        t1 = time.time()
        ko = o_sub.kmeanspp(U, k, seed=11)
        lo = o_sub.lloyds_projected(U, ko["C_lowd"])
        so = o_sub.lloyds_sparse(lift(U, lo["C_lowd"]))
        t_cpu_km = time.time() - t1
        hp2 = HotPath(local_rank)
        hp2.upload_csc(V, Bs["vals"], Bs["rows"], Bs["offs"])
        hp2.set_U(U)
        g2 = hp2.kmeans_init_on_projected_space(k, inject_seeds=ko["seeds"])
        lp2 = hp2.run_lloyds_on_projected_space(k, g2["C_lowd"])
        hp2.left_multiply_by_U(lp2["C_lowd"], fetch=False)
        ls2 = hp2.run_lloyds(k)
        hp2.close()

        def objective(assign, centers):  # sum_d |b_d - c_a(d)|^2 in fp64
            import scipy.sparse as sp
            S = sp.csc_matrix((Bs["vals"].astype(np.float64), Bs["rows"], Bs["offs"]), shape=(V, n_sub))
            Cn = centers.astype(np.float64)
            cn2 = (Cn ** 2).sum(0)
            tot_ = 0.0
            for c0 in range(0, n_sub, 8192):
                a = assign[c0:c0 + 8192].astype(np.int64)
                Sb = S[:, c0:c0 + 8192]
                d2 = np.asarray(Sb.multiply(Sb).sum(0)).ravel() + cn2[a] - 2.0 * np.asarray(Sb.multiply(Cn[:, a]).sum(0)).ravel()
                tot_ += float(d2.sum())
            return tot_

        pl = planted[cols].astype(np.int64) % k

        def purity_of(a):
            m = np.zeros((k, k), np.int64)
            np.add.at(m, (a.astype(np.int64), pl), 1)
            return float(m.max(1).sum() / n_sub)

        km = {"sample": "%d documents of B drawn at random (seed 7), U of the timed run, seeds drawn by the oracle's k-means++ and injected "
                        "into the HIP path" % n_sub,
              "partition_agreement_projected": round(float((lp2["assign"] == lo["assign"]).mean()), 5),
              "partition_agreement_word_space": round(float((ls2["assign"] == so["assign"]).mean()), 5),
              "iterations_hip": [lp2["iters"], ls2["iters"]], "iterations_oracle": [lo["iters"], so["iters"]],
              "objective_hip": objective(ls2["assign"], ls2["centers"]), "objective_oracle": objective(so["assign"], so["centers"]),
              "planted_topic_agreement_hip": round(purity_of(ls2["assign"]), 4), "planted_topic_agreement_oracle": round(purity_of(so["assign"]), 4),
              "oracle_seconds": round(t_cpu_km, 1)}
        log("k-means sample leg: oracle %.1f s" % t_cpu_km)
        del o_sub, Bs

    # ---------------- CPU baseline: the oracle ("port") on a bounded sample of the same work --------------
    # Unit costs (one Gram application, one k-means++ round, one iteration of each Lloyd loop) are measured and scaled by the counts the
    # GPU run executed.  Small inputs: measured on the full matrix.  Big inputs (config 3): measured on the first 1/32 of the columns
    # and scaled by 32 — every unit cost is linear in the number of documents / nonzeros at fixed V and k.
    cpu = None
    if world == 1 and not args.no_cpu_baseline:
        cores = effective_cpus()
        tc0 = time.time()
        frac = 32 if big else 1
        if frac == 1:
            o, n_o = o_full, D_loc
        else:
            n_o = D_loc // frac
            e_o = int(B["offs"][n_o])
            del o_full
            o = OracleCsc(V, n_o, B["vals"][:e_o], B["rows"][:e_o], B["offs"][:n_o + 1])
        X = np.random.default_rng(0).standard_normal((V, b)).astype(np.float32)
        o.gram_apply(X)
        t1 = time.time()
        reps = 2
        for _ in range(reps):
            o.gram_apply(X)
        t_apply_cpu = (time.time() - t1) / reps
        t1 = time.time()
        kr = o.kmeanspp(U, k, seed=1, max_rounds=3)
        t_round_cpu = (time.time() - t1) / max(kr["rounds"], 1)
        C0 = np.ascontiguousarray(o.project(U)[0][:k])  # any k points as centres: cost per iteration is data-independent
        t1 = time.time()
        o.lloyds_projected(U, C0, max_reps=1)
        ta = time.time() - t1
        t1 = time.time()
        o.lloyds_projected(U, C0, max_reps=2)
        t_lp_cpu = max(time.time() - t1 - ta, 1e-9)
        from oracle.oracle import lift
        cen = lift(U, C0)
        t1 = time.time()
        o.lloyds_sparse(cen, max_reps=1)
        ta = time.time() - t1
        t1 = time.time()
        o.lloyds_sparse(cen, max_reps=2)
        t_ls_cpu = max(time.time() - t1 - ta, 1e-9)
        n_app = last["ks"]["napplies"]
        # The dense half of the CPU eigensolver (BlockKs::expand / compute_qr / truncate, block-ks/restarted_block_ks.h:62-187): its cost
        # depends on V, k and the block size, not on the number of documents, so it is measured at full V and NOT scaled by `frac`.
        # One CGS2 step (two rounds of H = V_m^T F, F -= V_m H) and one Ritz rotation as BLAS products on these cores (numpy: what the
        # reference does through Armadillo / MKL), one fp64-MGS panel QR and one eig_sym by the oracle; the EVD at n <= 640 and scaled by n^3.
        ncv_ = 2 * k + b if k > 10 else 2 * k + 10
        rst = last["ks"]["restarts"]
        widths = list(range(2 * b, ncv_, b)) + rst * list(range(k + b, ncv_, b)) if k > b else [b] * max(n_app - 1, 0)
        rngd = np.random.default_rng(1)
        m_mid = max(b, min(ncv_ - b, int(np.mean(widths)) if widths else b))
        Vm = rngd.standard_normal((V, m_mid), dtype=np.float32)
        Fb = rngd.standard_normal((V, b), dtype=np.float32)
        t1 = time.time()
        for _ in range(2):
            Hc = Vm.T @ Fb
            Fb -= Vm @ Hc
        t_cgs2_mid = time.time() - t1
        t_ortho_cpu = t_cgs2_mid * (sum(widths) / m_mid) if widths else 0.0
        from oracle import oracle as orc_d
        t1 = time.time()
        orc_d.qr(np.asfortranarray(Fb))
        t_qr_cpu = (time.time() - t1) * n_app
        n_evd = ncv_ - b
        n_meas = min(n_evd, 640)
        Sm = rngd.standard_normal((n_meas, n_meas)).astype(np.float32)
        t1 = time.time()
        orc_d.eig_sym((Sm + Sm.T) / 2)
        t_evd_cpu = (time.time() - t1) * (n_evd / n_meas) ** 3 * (rst + 1)
        kc = max(1, k // 8)
        Wr = rngd.standard_normal((n_evd if n_evd <= Vm.shape[1] else Vm.shape[1], kc), dtype=np.float32)
        t1 = time.time()
        _ = Vm[:, :Wr.shape[0]] @ Wr
        t_rot_cpu = (time.time() - t1) * (n_evd / Wr.shape[0]) * (k / kc) * (rst + 1)
        t_dense_cpu = t_ortho_cpu + t_qr_cpu + t_evd_cpu + t_rot_cpu
        del Vm, Fb
        est = frac * (n_app * t_apply_cpu + last["kmpp_rounds"] * t_round_cpu + last["lp_iters"] * t_lp_cpu +
                      last["ls_iters"] * t_ls_cpu) + t_dense_cpu
        cpu = {
            "value": round((docs_metric if world == 1 else D_loc) / est, 1), "unit": "docs/sec", "cores": cores, "kind": "port",
            "cpu_model": cpu_model_name(), "cpus_online": os.cpu_count(),
            "sample": ("same-work extrapolation on %s: measured 1 Gram-apply (%.3fs), 1 k-means++ round "
                       "(%.3fs), 1 projected-Lloyd iteration (%.3fs), 1 sparse-Lloyd iteration (%.3fs) of oracle/ "
                       "(OpenMP, %d threads), scaled by the counts the GPU run executed (%d applies, %d rounds, %d+%d "
                       "iterations)%s; plus the dense half of the CPU eigensolver at full V, not scaled by the sample: orthogonalisation %.1fs (one CGS2 "
                       "step at basis width %d as BLAS products, scaled by the sum of the widths), panel QR %.1fs (oracle's fp64 MGS x %d), "
                       "small EVD %.1fs (oracle's eig_sym at n = %d, scaled by n^3 to %d, x %d), Ritz rotation %.1fs; sampling took %.0fs" %
                       ("the full-size matrix" if frac == 1 else "the first 1/%d of the columns (%d documents, all %d words, k = %d)" % (frac, n_o, V, k),
                        t_apply_cpu, t_round_cpu, t_lp_cpu, t_ls_cpu, cores, n_app, last["kmpp_rounds"], last["lp_iters"],
                        last["ls_iters"], "" if frac == 1 else " and by %d for the size" % frac, t_ortho_cpu, m_mid, t_qr_cpu, n_app,
                        t_evd_cpu, n_meas, n_evd, rst + 1, t_rot_cpu, time.time() - tc0)),
            "dense_eigensolver_seconds": {"ortho": round(t_ortho_cpu, 2), "qr": round(t_qr_cpu, 2), "evd": round(t_evd_cpu, 2), "rotate": round(t_rot_cpu, 2)},
        }
        try:  # the port's speed against the reference's own MKL path, unit by unit (tools/cpu_calibration.py, run in the build container)
            with open(os.path.join(ROOT, "profiles", "cpu_port_calibration.json")) as f:
                cal = json.load(f)
            cpu["port_over_reference"] = dict(cal["port_over_reference"], measured_at="V=%d, D=%d, k=%d, %d threads: port unit seconds %s against "
                                              "the reference's %s (%s)" % (cal["shape"]["V"], cal["shape"]["D"], cal["shape"]["k"], cal["threads"],
                                                                           cal["port_unit_seconds"], cal["reference_unit_seconds"], cal["reference_source"]))
        except Exception:
            cpu["port_over_reference"] = None
        log("cpu_baseline leg: %.1f s" % (time.time() - tc0))
        del o

    # ---------------- stages either side of the path (outside the timed region), each checked at full size --------
    up = None
    if upstream:
        cntA, rowsA, offsA = A_host
        hp.timing_enable(True)
        hp.timing_reset()
        t1 = time.perf_counter()
        hp.ingest_tdf(tdf_text, V, D_per, max_entries=len(cntA))   # tdf text -> A on the device
        t_up = time.perf_counter() - t1
        ingest_dev_ms = hp.timing_get()["ingest"][0]
        gA = hp.get_A()
        same_A = bool(np.array_equal(gA[0], cntA) and np.array_equal(gA[1], rowsA) and np.array_equal(gA[2], offsA))
        ingest = {"stage": "tdf text -> count matrix on the device (parse + radix sort + de-duplication + CSC)",
                  "text_bytes": int(tdf_text.size), "lines": int(len(cntA)), "wall_ms_incl_h2d": round(t_up * 1e3, 1),
                  "device_ms": round(ingest_dev_ms, 3), "identical_to_generator_csc": same_A}
        del gA, tdf_text
        hp.timing_reset()
        t1 = time.perf_counter()
        hp.threshold(k)
        hp.synchronize()
        t_thr = time.perf_counter() - t1
        tm2 = hp.timing_get()
        hp.timing_enable(False)
        got = hp.get_B()
        same = all(np.array_equal(got[x], B[x]) for x in ("vals", "rows", "offs", "original_cols", "zetas"))
        up = {"stage": "thresholding A -> B on the device (normalize_docs + compute_thresholds + threshold_and_copy)",
              "wall_ms": round(t_thr * 1e3, 3), "device_ms": round(tm2["threshold"][0], 3),
              "GB_per_s_over_A": round(12.0 * nnz_A / max(tm2["threshold"][0], 1e-9) / 1e6, 1),
              "cpu_port_ms": round(t_thr_cpu * 1e3, 1), "cpu_cores": effective_cpus(),
              "identical_to_cpu": bool(same)}
        del got
        # downstream stage on the partition the last timed step left on the device ... after re-running the hot path on the
        # device-built B (identical to the uploaded one), outside the timed region
        from isle_amd.hot_path import catchword_rank, model_rank_threshold  # the trainer's formulae live in the binding
        step(-100, wall=False)
        hp.timing_enable(True)
        hp.timing_reset()
        t1 = time.perf_counter()
        cw = hp.find_catchwords(k, catchword_rank(D_per, k), fetch_thresholds=False)
        t_cw = time.perf_counter() - t1
        t1 = time.perf_counter()
        tmo = hp.construct_topic_model(k, model_rank_threshold(D_per, k), D_per, fetch_sums=False)
        t_tm = time.perf_counter() - t1
        tm3 = hp.timing_get()
        hp.timing_enable(False)
        down = {"stage": "catchwords + topic model on the device (src/trainer.cpp:577-654)",
                "catchwords_wall_ms": round(t_cw * 1e3, 3), "topic_model_wall_ms": round(t_tm * 1e3, 3),
                "device_ms": round(tm3["post"][0], 3), "num_catchwords": cw["num_catchwords"],
                "doc_topic_sums": tmo["num_sums"], "model_columns_sum_to_one": bool(np.allclose(np.abs(tmo["model"]).sum(0), 1.0, rtol=1e-3))}
        # inference (next-4): ISLEInfer of all documents of A under the model just built; the CPU restatement on a sample
        from oracle import oracle as orc
        model_by_word = np.ascontiguousarray(np.nan_to_num(tmo["model"]), np.float32)  # V x k, element (word, topic): row-major
        hp.timing_enable(True)
        hp.timing_reset()
        t1 = time.perf_counter()
        inf = hp.infer(model_by_word, offsA, rowsA, cntA, want_weights=False)
        t_inf = time.perf_counter() - t1
        tm4 = hp.timing_get()
        hp.timing_enable(False)
        ns = min(D_per, 20000)  # bounded CPU sample: the first ns documents
        t1 = time.perf_counter()
        oi = orc.infer(model_by_word, offsA[:ns + 1], rowsA[:offsA[ns]], cntA[:offsA[ns]], avg_doc_sz=inf["avg_doc_sz"])
        t_inf_cpu = time.perf_counter() - t1
        conv = oi["llh"][:, 0] != 0
        llh_ok = bool(np.allclose(inf["llh"][:ns], oi["llh"], rtol=2e-4, atol=1e-4))
        top_ok = float(np.mean(inf["top_topic"][:ns][conv, 0] == np.argmax(oi["weights"][conv], axis=1))) if conv.any() else 1.0
        infer_stage = {"stage": "ISLEInfer on the device (drivers/ISLEInfer.cpp, src/infer.cpp:361-492): all documents of A, 15 iterations",
                       "docs": int(D_per), "wall_ms_incl_transfers": round(t_inf * 1e3, 1), "device_ms": round(tm4["infer"][0], 3),
                       "docs_per_sec_device": round(D_per / max(tm4["infer"][0], 1e-9) * 1e3, 1), "converged": inf["nconverged"],
                       "cpu_port_docs_per_sec": round(ns / t_inf_cpu, 1), "cpu_cores": effective_cpus(), "cpu_sample_docs": int(ns),
                       "llh_matches_cpu_on_sample": llh_ok, "heaviest_topic_agreement_on_sample": round(top_ok, 5)}
        up = {"note": "stages either side of the hot path, run OUTSIDE the timed region at the same size, each checked at full size",
              "ingest": ingest, "threshold": up, "downstream": down, "inference": infer_stage}
        del A_host
    elif device_stage:
        up = {"note": "stages either side of the hot path, run on the device OUTSIDE the timed region at the workload's own size", "input": stage_in}
        if edge_topics and world == 1:
            # configs[4]: what train_edge_topics adds behind a config-3 hot path (src/trainer.cpp:577-685, :1116-1167) — catchwords and the topic
            # model from the partition the last timed step left on the device, the pair selection on the host (as fpsparse_hip.h does it), the
            # two FPaxpy per edge topic on the device, the V x #edge model back on the host.  Checker: oracle/isle_post_oracle.cpp for the pair
            # selection (all pairs) and for a sample of the edge columns.
            from isle_amd.hot_path import EDGE_TOPIC_PRIMARY_RATIO, catchword_rank, model_rank_threshold, select_edge_pairs
            from oracle import oracle as orc
            D_A = int(WORKLOADS[workload][1])
            hp.timing_enable(True)
            hp.timing_reset()
            t1 = time.perf_counter()
            cw = hp.find_catchwords(k, catchword_rank(D_A, k), fetch_thresholds=False)
            t_cw = time.perf_counter() - t1
            t1 = time.perf_counter()
            tmo = hp.construct_topic_model(k, model_rank_threshold(D_A, k), D_A, fetch_sums=False)
            t_tm = time.perf_counter() - t1
            t1 = time.perf_counter()
            pairs = select_edge_pairs(tmo["top1"], tmo["top2"], edge_topics)
            t_sel = time.perf_counter() - t1
            t1 = time.perf_counter()
            E = hp.edge_topics(pairs[:, :2])
            t_edge = time.perf_counter() - t1
            post_ms = hp.timing_get()["post"][0]
            hp.timing_enable(False)
            model = tmo["model"]
            ref_pairs, _ = orc.post_edge_topics(model, tmo["top1"], tmo["top2"], edge_topics, want_edge=False)
            pick_e = np.unique(np.linspace(0, max(len(pairs) - 1, 0), 64).astype(np.int64)) if len(pairs) else np.zeros(0, np.int64)
            worst = 0.0
            for t_ in pick_e:
                want = (np.float32(EDGE_TOPIC_PRIMARY_RATIO) * model[:, pairs[t_, 0]].astype(np.float64)
                        + np.float32(1.0 - EDGE_TOPIC_PRIMARY_RATIO) * model[:, pairs[t_, 1]].astype(np.float64))
                okc = np.isfinite(want)
                if okc.any():
                    worst = max(worst, float(np.max(np.abs(E[okc, t_] - want[okc]) / np.maximum(np.abs(want[okc]), 1e-12))))
            up["edge_topics"] = {"stage": "catchwords + topic model + edge topics (src/trainer.cpp:577-685, construct_edge_topics_v2 :1116-1167), max_edge_topics=%d"
                                          % edge_topics,
                                 "catchwords_wall_ms": round(t_cw * 1e3, 1), "topic_model_wall_ms": round(t_tm * 1e3, 1),
                                 "pair_selection_host_ms": round(t_sel * 1e3, 1), "edge_model_wall_ms_incl_d2h": round(t_edge * 1e3, 1),
                                 "device_ms": round(post_ms, 3), "num_catchwords": cw["num_catchwords"],
                                 "documents_with_two_topics": int(((tmo["top1"] >= 0) & (tmo["top2"] >= 0)).sum()),
                                 "num_edge_topics": int(len(pairs)), "edge_model_bytes": int(E.nbytes),
                                 "pairs_identical_to_oracle": bool(np.array_equal(pairs, ref_pairs)),
                                 "edge_columns_checked": int(len(pick_e)), "edge_columns_worst_rel_err": worst,
                                 "model_columns_sum_to_one": bool(np.allclose(np.nansum(np.abs(model), 0)[np.isfinite(model).all(0)], 1.0, rtol=1e-3))}
            if not up["edge_topics"]["pairs_identical_to_oracle"] or worst > 1e-5:
                raise SystemExit("bench.py: edge-topic stage differs from the CPU restatement: %s" % up["edge_topics"])
            del E, model, tmo
    elif full and world == 1 and big and not args.no_upstream:
        up = {"note": "not run at this size: the corpus is generated directly as CSC (a 1.1 B-line tdf file is 15 GB of text, SURVEY §8d); "
                      "`--workload c2` runs ingest, thresholding, catchwords + topic model and inference at 1 M documents, each checked at "
                      "full size"}
    hp.close()

    out["accuracy"] = {"sigma_rel_err_bound": float(np.max(resid) / 2.0), "checked_pairs": int(len(pick)), "of": k,
                       "U_orthonormality_defect": ortho, "seconds": round(t_acc, 1),
                       "note": "|sigma-sigma_true|/sigma <= ||A u - lambda u|| / (2 lambda); A u computed by the CPU ORACLE's operator "
                               "(oracle/isle_oracle.cpp, fp32 OpenMP), not by the library under test",
                       "planted_topic_agreement": round(purity, 4), "kmeans_vs_oracle": km}
    out["cpu_baseline"] = cpu
    out["other_stages"] = up
    # the accuracy figures are a GATE, not a report: a run outside the contract (top-k sigma within 1e-4, BASELINE.json north_star; partitions
    # equal to the oracle's up to near-ties) still prints its line, marked, and exits non-zero
    failed = []
    if not out["accuracy"]["sigma_rel_err_bound"] <= SIGMA_GATE:
        failed.append("sigma_rel_err_bound %.3g > %.0e" % (out["accuracy"]["sigma_rel_err_bound"], SIGMA_GATE))
    if km is not None:
        for key in ("partition_agreement_projected", "partition_agreement_word_space"):
            if not km[key] >= PARTITION_GATE:
                failed.append("%s %.5f < %.3f" % (key, km[key], PARTITION_GATE))
    out["accuracy"]["gate"] = {"sigma_rel_err_bound_max": SIGMA_GATE, "partition_agreement_min": PARTITION_GATE, "passed": not failed, "failed": failed}
    return out


if __name__ == "__main__":
    main()
