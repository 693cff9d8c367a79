"""bench.py's arithmetic that needs no GPU: the per-family rooflines (SURVEY.md 8(d) figures x the counts a run executed), the k-means++
draw schedule (src/sparseMatrix.cpp:2183), the key under which a counter pass stays valid, and the host half of the edge-topic stage
(src/trainer.cpp:1116-1145) against the CPU restatement."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_kmpp_draw_schedule():
    d = bench.kmpp_draws(1000)
    assert d[:8] == [1, 1, 1, 1, 1, 2, 3, 4] and sum(d) == 999 and len(d) == 60  # 60 rounds at k = 1000 (what the device reports)
    assert sum(bench.kmpp_draws(200)) == 199 and bench.kmpp_draws(1) == []


def test_family_rooflines_reproduce_the_round_5_review():
    """The judge's hand computation from BENCH_r05.json's device_ms_per_step: ortho 0.54, k-means++ 0.25, sparse Lloyd
    0.12, projection 0.03 of HBM, rotation 0.58 of the f32 matrix cores."""
    dev = {"gram_pass1": 437.147, "gram_pass2": 604.149, "ortho": 130.958, "rotate": 8.756, "project": 183.006, "kmpp": 246.304,
           "lloyd_proj": 207.273, "sparse_assign": 158.311, "sparse_update": 12.971, "lift": 2.6}
    r = bench.family_rooflines(100_000, 10_000_000, 1_006_280_745, 1000, 10, 2010, 1, 300, 60, 10, 10, dev)
    want = {"gram": 0.293, "ortho": 0.54, "kmpp": 0.25, "sparse": 0.12, "project": 0.033, "rotate": 0.58, "lift": 0.49}
    for f, v in want.items():
        assert abs(r[f]["frac"] - v) <= 0.01, (f, r[f]["frac"])
        assert abs(r[f]["frac"] - r[f]["achieved"] / r[f]["peak"]) < 1e-3
    assert r["gram"]["bound"] == "hbm" and r["rotate"]["bound"] == "mfma" and r["ortho"]["unit"] == "GB/s"
    assert abs(r["ortho"]["algorithmic_bytes_per_step"] - 567e9) < 2e9 and abs(r["sparse"]["algorithmic_bytes_per_step"] - 169e9) < 1e9
    assert "qr" not in r and "evd" not in r  # latency chains: no SURVEY 8(d) figure
    # families without a device time are left out, not reported as zero
    assert set(bench.family_rooflines(1000, 1000, 10_000, 10, 1, 30, 0, 20, 5, 3, 3, {"gram_pass1": 1.0})) == {"gram"}


def test_counter_pass_is_keyed_by_the_kernel_source():
    sha = bench.gram_kernel_sha16()
    assert sha is not None and len(sha) == 16
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        ent = json.load(f)
    for key in ("c3full", "c2"):
        assert "kernel_source_sha16" in ent[key], key  # a pass without the key can no longer be reported as this build's traffic


def test_edge_pair_selection_matches_the_cpu_restatement():
    from isle_amd.hot_path import select_edge_pairs
    from oracle import oracle as O
    rng = np.random.default_rng(0)
    k, D = 30, 20_000
    t1 = rng.integers(-1, k, D).astype(np.int32)
    t2 = rng.integers(-1, k, D).astype(np.int32)
    M = np.asfortranarray(rng.random((50, k)).astype(np.float32))
    for cap in (1, 10, 200, 5000):
        ref, _ = O.post_edge_topics(M, t1, t2, cap, want_edge=False)
        assert np.array_equal(select_edge_pairs(t1, t2, cap), ref)
    assert select_edge_pairs(np.full(5, -1), np.full(5, -1), 10).shape == (0, 3)


def test_dumped_outputs_are_a_fixed_sample_within_the_cap(tmp_path):
    """--dump-outputs: the same seeded sample on every run, float32 / float64 files only, 64 MB at most in all."""
    a = bench.dump_sample(10_000_000, 1 << 19, 1)
    assert np.array_equal(a, bench.dump_sample(10_000_000, 1 << 19, 1)) and len(a) == 1 << 19 and np.all(np.diff(a) > 0)
    assert np.array_equal(bench.dump_sample(100, 2048, 2), np.arange(100))
    d = str(tmp_path / "out")
    bench.dump_outputs(d, {"x": np.arange(3, dtype=np.float32), "y": np.ones((2, 2))})
    assert np.array_equal(np.load(os.path.join(d, "x.npy")), [0, 1, 2]) and np.load(os.path.join(d, "y.npy")).dtype == np.float64
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((64 << 20) // 8 + 1)})
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "int"), {"x": np.zeros(3, np.int32)})
