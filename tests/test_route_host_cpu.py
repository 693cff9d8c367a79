"""isle_amd/csrc/route_host.h, every rule that chooses a kernel form, without the library and without a GPU: route_host_main is built here
with the address and undefined-behaviour sanitizers (a stand-alone program) and answers a script that this file sends on stdin.  The
switches go in as the strings the environment would hold; a double crosses as its 64 bits.  Every expected answer is stated here in Python
from the expressions the routes had while they stood inline in the eight source files (integers, IEEE doubles and C's atoi); nothing here
reads the header, so no case can pass by agreement of the code with itself.  Cases sit on both sides of every edge."""
import json
import math
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = [t.strip()[3:] for t in re.search(r"enum IsleKnob \{(.*?)\};", open(os.path.join(ROOT, "isle_amd", "csrc", "knobs.h")).read(),
                                           flags=re.S).group(1).replace("\n", " ").split(",") if t.strip()][:-1]
MI355X = 288 * 10 ** 9  # bytes of a 288 GB device


def d2b(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def b(v):
    return int(bool(v))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("route_host") / "route_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "route_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def env_line(env):
    """env: {switch name without ISLE_ / KN_: string}"""
    return ["env", len(env)] + [t for n, v in env.items() for t in (KNOBS.index(n), v.encode().hex() or "-")]


def run(exe, env, script):
    """The script's commands under the given switches -> one dict per command"""
    lines = [env_line(env)] + script
    text = "\n".join(" ".join(str(t) for t in line) for line in lines) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o.pop("cmd") for o in out] == [line[0] for line in lines]
    return out[1:]


# ---- the switches, as the sources read them -----------------------------------------------------------------------------------------------
def atoi(s):
    m = re.match(r"[ \t\n\v\f\r]*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


class Env:
    """knob / knob_on / knob_is / knob_zero of the context, on a dict of strings"""

    def __init__(self, env):
        self.v = env

    def on(self, n):
        return n in self.v

    def zero(self, n):
        return n in self.v and atoi(self.v[n]) == 0

    def is_(self, n, word):
        return self.v.get(n) == word

    def get(self, n):
        return self.v.get(n)


def env_py(env):
    """Every typed value, switch by switch, as its call sites computed it from the string."""
    e = Env(env)
    word = lambda n, words, other: (words.index(e.get(n)) if e.get(n) in words else other)  # noqa: E731
    forced_g = lambda n: max(4, min(8, atoi(e.get(n)))) if e.on(n) else 0  # noqa: E731
    return dict(
        gram_lds=b(not (e.on("GRAM_LDS") and atoi(e.get("GRAM_LDS")) == 0)), gl_g1=forced_g("GL_G1"), gl_g2=forced_g("GL_G2"),
        gl_place=b(not e.zero("GL_PLACE")), gl_fill_buckets=b(not e.zero("GL_FILL_BUCKETS")), gl_rounds=b(not e.zero("GL_ROUNDS")),
        gl_columns=b(not e.zero("GL_COLUMNS")), gl_panel=atoi(e.get("GL_PANEL")) if e.on("GL_PANEL") and atoi(e.get("GL_PANEL")) in (8, 10) else 0,
        gl_wide_grouped=b(not e.zero("GL_WIDE_GROUPED")), wide_gather=b(e.on("WIDE_GATHER")), wide_lds=b(e.on("WIDE_LDS")),
        ks_rowshard=b(not e.zero("KS_ROWSHARD")), ks_sync=b(e.on("KS_SYNC")),
        ks_ortho_passes=max(2, min(3, atoi(e.get("KS_ORTHO_PASSES")))) if e.on("KS_ORTHO_PASSES") else 2,
        update_mfma=b(not e.zero("UPDATE_MFMA")), evd_jacobi=b(e.on("EVD_JACOBI")), td_chain=b(e.on("TD_CHAIN")), td_bar=word("TD_BAR", ["flat", "hier"], 2),
        td_back=b(e.on("TD_BACK") and e.get("TD_BACK")[:1] == "s"), evd_split=b(e.on("EVD_SPLIT") and not e.zero("EVD_SPLIT")),
        kmpp_host_dice=b(e.on("KMPP_HOST_DICE")), kmpp_sparse=b(atoi(e.get("KMPP_SPARSE")) != 0) if e.on("KMPP_SPARSE") else -1,
        kmpp_track=b(not e.zero("KMPP_TRACK")), no_hamerly=b(e.on("NO_HAMERLY")), kmeans_bounds=word("KMEANS_BOUNDS", [None, "hamerly", "none"], 0),
        proj_bounds=b(e.is_("PROJ_BOUNDS", "hamerly")), proj_full=word("PROJ_FULL", [None, "gemm", "fused"], 0),
        first_assign=word("FIRST_ASSIGN", [None, "sparse", "projection"], 0), gemm_bf16x3=b(not e.zero("GEMM_BF16X3")),
        gemm_epilogue=b(not e.zero("GEMM_EPILOGUE")), gemm_terms=3 if e.on("GEMM_TERMS") and atoi(e.get("GEMM_TERMS")) == 3 else 2,
        gemm_dma=b(not e.zero("GEMM_DMA")), yy_mode=word("YY_MODE", ["doc", "docg", "group"], -1), yy_fused=b(not e.zero("YY_FUSED")),
        yy_movers=b(not e.zero("YY_MOVERS")), yy_regroup=b(not e.zero("YY_REGROUP")), yy_order=(b(e.get("YY_ORDER") != "doc") if e.on("YY_ORDER") else -1),
        pt_sort=b(not e.zero("PT_SORT")), proj_active=b(e.get("PROJ_ACTIVE") == "gemm" if e.on("PROJ_ACTIVE") else True), proj_sums=b(e.is_("PROJ_SUMS", "fresh")),
        centers_fresh=b(e.on("CENTERS_FRESH")), infer_cap_rows=atoi(e.get("INFER_CAP_ROWS")) & 0xFFFFFFFF if e.on("INFER_CAP_ROWS") else 0,
        chunk_cols=atoi(e.get("CHUNK_COLS")) & 0xFFFFFFFF if e.on("CHUNK_COLS") else 0, comm_timeout_set=b(e.on("COMM_TIMEOUT")),
        comm_timeout=d2b(float(e.get("COMM_TIMEOUT")) if e.on("COMM_TIMEOUT") else 0.0),
        comm_selftest=b(not e.zero("COMM_SELFTEST")) if e.on("COMM_SELFTEST") else -1)


ROUTED = ["GRAM_LDS", "GL_G1", "GL_G2", "GL_PLACE", "GL_FILL_BUCKETS", "GL_ROUNDS", "GL_COLUMNS", "GL_PANEL", "GL_WIDE_GROUPED", "WIDE_GATHER", "WIDE_LDS",
          "KS_ROWSHARD", "KS_SYNC", "KS_ORTHO_PASSES", "UPDATE_MFMA", "EVD_JACOBI", "TD_CHAIN", "TD_BAR", "TD_BACK", "EVD_SPLIT", "KMPP_HOST_DICE",
          "KMPP_SPARSE", "KMPP_TRACK", "NO_HAMERLY", "KMEANS_BOUNDS", "PROJ_BOUNDS", "PROJ_FULL", "FIRST_ASSIGN", "GEMM_BF16X3", "GEMM_EPILOGUE",
          "GEMM_TERMS", "GEMM_DMA", "YY_MODE", "YY_FUSED", "YY_MOVERS", "YY_REGROUP", "YY_ORDER", "PT_SORT", "PROJ_ACTIVE", "PROJ_SUMS", "CENTERS_FRESH",
          "INFER_CAP_ROWS", "CHUNK_COLS", "COMM_SELFTEST"]
VALUES = ["", "0", "1", "2", "3", "4", "5", "8", "9", "10", "12", "-1", " 0", "00", "0x", "x", "doc", "docg", "group", "member", "hamerly", "none", "gemm", "fused",
          "tiles", "sparse", "projection", "fresh", "flat", "hier", "seq", "s", "wy", "Seq", "unknown", "docs", "grou"]


def test_the_switch_list_is_the_one_this_file_knows():
    """every switch of kind form or tuning has a typed value; the rest are diagnostics and test hooks, read where they are used"""
    rest = {"FORCE_COMM", "TEST_STALL_MS", "ROCTX", "HOST_TRACE", "DEBUG_HAMERLY", "DEBUG_EVD", "GL_VERBOSE", "TD_FORCE_BAIL_RANK",
            "GL_TEST_CUS", "GL_ABLATE_SKIP"}
    assert set(KNOBS) == set(ROUTED) | {"COMM_TIMEOUT"} | rest and not set(ROUTED) & rest and len(set(KNOBS)) == len(KNOBS)  # (test_comm_timeout)


def test_nothing_set(exe):
    o = run(exe, {}, [env_line({})])
    assert o[0] == env_py({})
    assert env_py({}) == dict(env_py({}), gram_lds=1, gl_g1=0, gl_panel=0, ks_ortho_passes=2, td_bar=2, td_back=0, kmpp_sparse=-1, kmeans_bounds=0, gemm_terms=2,
                              yy_mode=-1, yy_order=-1, proj_active=1, comm_selftest=-1, comm_timeout_set=0, infer_cap_rows=0, chunk_cols=0, kmpp_track=1)


@pytest.mark.parametrize("name", ROUTED)
def test_every_switch_alone_at_every_value(exe, name):
    """unset, empty, 0, 1, every word any switch knows and words none knows: the one switch set, every field stated"""
    out = run(exe, {}, [env_line({name: v}) for v in VALUES])
    for v, o in zip(VALUES, out):
        assert o == env_py({name: v}), (name, v)
    changed = {f for v in VALUES for f, x in env_py({name: v}).items() if x != env_py({})[f]}
    assert changed == {name.lower()}, "a switch moves its own field and no other"


def test_comm_timeout(exe):
    for v in ["", "0", "120", "2.5", "-1", "1e3", "abc"]:
        m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", v)
        want = float(m.group(0)) if m else 0.0
        o = run(exe, {"COMM_TIMEOUT": v}, [env_line({"COMM_TIMEOUT": v}), ["comm", 0, d2b(300.0)]])
        assert (o[0]["comm_timeout_set"], o[0]["comm_timeout"], o[1]["timeout"]) == (1, d2b(want), d2b(want)), v
    assert run(exe, {}, [["comm", 0, d2b(300.0)]])[0]["timeout"] == d2b(300.0)


def test_all_switches_together(exe):
    env = {"NO_HAMERLY": "0", "YY_MODE": "docg", "GEMM_TERMS": "3", "TD_BACK": "seq", "GL_PANEL": "8", "KMPP_SPARSE": "0", "COMM_TIMEOUT": "7", "GL_G1": "9",
           "FORCE_COMM": "1", "DEBUG_EVD": "1"}
    assert run(exe, {}, [env_line(env)])[0] == env_py(env)


# ---- api.cpp: scratch, self-test ------------------------------------------------------------------------------------------------------------
def scratch_py(nbytes, total):
    """-> (ok, asks the device): isle_scratch_ok, whose query ran where total_mem was still 0"""
    if nbytes <= 8e9:
        return 1, 0
    if total == 0:
        return 0, 1
    return b(nbytes <= 0.2 * float(total)), 0


def test_scratch(exe):
    fifth = 0.2 * float(MI355X)
    sizes = [0.0, 8e9, math.nextafter(8e9, math.inf), fifth, math.nextafter(fifth, math.inf), math.nextafter(fifth, 0.0), 4e10, 1e12]
    script = [["scratch", d2b(x), t] for x in sizes for t in (0, MI355X, 1)]
    want = [scratch_py(x, t) for x in sizes for t in (0, MI355X, 1)]
    assert [(o["ok"], o["ask"]) for o in run(exe, {}, script)] == want
    assert scratch_py(8e9, 0) == (1, 0) and scratch_py(math.nextafter(8e9, math.inf), 0) == (0, 1)
    assert scratch_py(fifth, MI355X) == (1, 0) and scratch_py(math.nextafter(fifth, math.inf), MI355X) == (0, 0) and 57.5e9 < fifth < 57.7e9


@pytest.mark.parametrize("v", [None, "", "0", "1", "yes"])
def test_comm_selftest(exe, v):
    env = {} if v is None else {"COMM_SELFTEST": v}
    e = Env(env)
    for dflt, o in zip((0, 1), run(exe, env, [["comm", 0, d2b(300.0)], ["comm", 1, d2b(300.0)]])):
        assert o["selftest"] == b((not e.zero("COMM_SELFTEST")) if e.on("COMM_SELFTEST") else dflt)


# ---- api_ks.cpp -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KS_ROWSHARD": "0"}, {"KS_ROWSHARD": "1"}, {"KS_ROWSHARD": ""}, {"KS_SYNC": "0"}, {"KS_ORTHO_PASSES": "3"}])
def test_krylov_schur(exe, env):
    e = Env(env)
    cases = [(m, d) for m in (0, 1) for d in (0, 1)]
    for (multi, dense), o in zip(cases, run(exe, env, [["ks", m, d] for m, d in cases])):
        assert o == dict(shard=b(multi and not dense and not e.zero("KS_ROWSHARD")), pipelined=b(not e.on("KS_SYNC")))


# ---- dense.hip ------------------------------------------------------------------------------------------------------------------------------
def tiles(M, N):
    return (M + 255) // 256 * ((N + 255) // 256)


def fused_ok_py(e, M, K, N):
    return not e.zero("GEMM_BF16X3") and not e.zero("GEMM_EPILOGUE") and N >= 64 and K >= 32 and tiles(M, N) >= 512 and M < (1 << 32)


GEMM_SHAPES = [(200000, 64, 64), (200000, 64, 63), (200000, 31, 64), (200000, 32, 64), (200000, 32, 63),
               (130816, 256, 256), (130817, 256, 256), (130816, 64, 64), (130817, 64, 64), (65280, 257, 257), (65281, 257, 257), (130816, 257, 257),
               (2 ** 32 - 1, 1000, 1000), (2 ** 32, 1000, 1000), (0, 64, 64), (1, 1, 1)]


@pytest.mark.parametrize("env", [{}, {"GEMM_BF16X3": "0"}, {"GEMM_BF16X3": "1"}, {"GEMM_BF16X3": ""}, {"GEMM_EPILOGUE": "0"}, {"GEMM_TERMS": "3"},
                                 {"GEMM_TERMS": "2"}, {"GEMM_TERMS": ""}, {"GEMM_DMA": "0"}, {"GEMM_DMA": "1"}])
def test_assignment_product(exe, env):
    e = Env(env)
    script = [["gemm", M, K, N, r, s] for M, K, N in GEMM_SHAPES for r in (0, 1) for s in (0, 1)]
    three = e.on("GEMM_TERMS") and atoi(e.get("GEMM_TERMS")) == 3
    for (_, M, K, N, r, s), o in zip(script, run(exe, env, script)):
        want = dict(tiles=tiles(M, N), bf16x3=b(not (e.zero("GEMM_BF16X3") or N < 64 or K < 32 or tiles(M, N) < 512)), fused_ok=b(fused_ok_py(e, M, K, N)),
                    two_terms=b(not three and r), dma=b(s and not e.zero("GEMM_DMA")))
        assert o == want, (M, K, N, r, s)
    assert (tiles(130816, 256), tiles(130817, 256), tiles(65280, 257), tiles(65281, 257)) == (511, 512, 510, 512)
    a2 = [(0, 64), (130816, 64), (130817, 64), (130817, 63), (2 ** 32, 1000)]
    for (D, k), o in zip(a2, run(exe, env, [["a2", D, k] for D, k in a2])):
        assert o["want_a2"] == b(D and fused_ok_py(e, D, k, k) and not e.zero("GEMM_DMA") and not three), (D, k)


@pytest.mark.parametrize("env", [{}, {"UPDATE_MFMA": "0"}, {"UPDATE_MFMA": "1"}, {"UPDATE_MFMA": ""}])
def test_update_on_the_matrix_cores(exe, env):
    e = Env(env)
    script = [["update", bb, m, ld, al] for bb in (1, 16, 17) for m in (31, 32, 2010) for ld in (100000, 100001, 100002, 100004, 2 ** 33 + 2) for al in (0, 1)]
    for (_, bb, m, ld, al), o in zip(script, run(exe, env, script)):
        assert o["mfma"] == b(bb <= 16 and m >= 32 and (ld & 3) == 0 and al and not e.zero("UPDATE_MFMA")), (bb, m, ld, al)


@pytest.mark.parametrize("env", [{}, {"EVD_JACOBI": "1"}, {"EVD_JACOBI": "0"}, {"EVD_JACOBI": ""}])
def test_small_evd_solver(exe, env):
    ns = [1, 15, 16, 17, 2010]
    for n, o in zip(ns, run(exe, env, [["evd", n] for n in ns])):
        assert o["tridiag"] == b(n >= 16 and not Env(env).on("EVD_JACOBI"))


# ---- k-means++ --------------------------------------------------------------------------------------------------------------------------
KS_TILES = [1, 64, 224, 225, 1000, 1024, 1025, 2048]


@pytest.mark.parametrize("env", [{}, {"KMPP_TRACK": "0"}, {"KMPP_TRACK": "1"}, {"KMPP_TRACK": ""}, {"KMPP_HOST_DICE": "0"}, {"KMPP_HOST_DICE": ""}])
def test_kmeanspp_plan(exe, env):
    e = Env(env)
    script = [["kmpp", k, m, i] for k in KS_TILES for m in (0, 1) for i in (0, 1)]
    for (_, k, multi, inj), o in zip(script, run(exe, env, script)):
        want = dict(track=b(k > 224 and (k + 31) // 32 <= 32 and not e.zero("KMPP_TRACK")), maxdraw=2 + math.ceil(math.sqrt(float(k))),
                    device_dice=b(not multi and not inj and not e.on("KMPP_HOST_DICE")))
        assert o == want, (k, multi, inj)
    assert [2 + math.ceil(math.sqrt(float(k))) for k in (1, 224, 225, 1024, 1025)] == [3, 17, 17, 34, 35]


def kmpp_sparse_py(e, can, nnz, D, ldk, nc, PW):
    passes = (nc + PW - 1) // PW
    sparse = can and 15.4 * float(nnz) * passes < 4.0 * float(ldk) * float(D) * (1.0 if nc <= 16 else 2.3)
    if e.on("KMPP_SPARSE"):
        sparse = atoi(e.get("KMPP_SPARSE")) != 0 and can
    return b(sparse)


def first_true(pred, lo, hi):
    """the smallest integer in (lo, hi] at which the monotone predicate holds"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


@pytest.mark.parametrize("nc", [16, 17])
def test_kmeanspp_through_thin_products_by_cost(exe, nc):
    """nnz either side of 15.4 nnz passes = 4 ldk D (1 | 2.3): the largest count that still pays and the next one"""
    D, ldk = 1250000, 1000
    free = Env({})
    for PW in (8, 10):
        edge = first_true(lambda n: not kmpp_sparse_py(free, 1, n, D, ldk, nc, PW), 1, 10 ** 13)
        ratio = edge * 15.4 * ((nc + PW - 1) // PW) / (4.0 * ldk * D * (1.0 if nc <= 16 else 2.3))
        assert abs(ratio - 1.0) < 1e-7  # (one nonzero is 6e-9 of the edge)
        for env in ({}, {"KMPP_SPARSE": "0"}, {"KMPP_SPARSE": "1"}, {"KMPP_SPARSE": ""}, {"KMPP_SPARSE": "2"}):
            script = [["kmpp_sparse", can, nnz, D, ldk, nc, PW] for can in (0, 1) for nnz in (edge - 1, edge, 0, 10 ** 13)]
            got = [o["sparse"] for o in run(exe, env, script)]
            assert got == [kmpp_sparse_py(Env(env), can, nnz, D, ldk, nc, PW) for _, can, nnz, _, _, _, _ in script], (env, PW)
            if not env:
                assert got == [0, 0, 0, 0, 1, 0, 1, 0]
    # equality does not pay: 15.4 x 10 nonzeros x 2 passes = 308 = 4 x 7 x 11, exactly in doubles
    assert 15.4 * 10.0 * 2 == 4.0 * 7.0 * 11.0 * 1.0
    assert [o["sparse"] for o in run(exe, {}, [["kmpp_sparse", 1, nnz, 11, 7, 16, 10] for nnz in (9, 10, 11)])] == [1, 0, 0]
    # the same count of nonzeros is on either side for 16 and for 17 new seeds
    mid = 2 * 10 ** 8
    assert (kmpp_sparse_py(free, 1, mid, D, ldk, 16, 10), kmpp_sparse_py(free, 1, mid, D, ldk, 17, 10)) == (0, 1)


# ---- Lloyd in span(U) ----------------------------------------------------------------------------------------------------------------------
def proj_py(e, f, k):
    D, Pt, Pt2, P, track_k, same_P, seeds = f
    p = {}
    p["hamerly"] = not e.on("NO_HAMERLY") and (Pt or Pt2)
    p["T"] = (k + 31) // 32
    p["TL"] = (p["T"] + 3) & ~3
    p["tiles"] = p["hamerly"] and k > 224 and p["T"] <= 32 and not e.is_("PROJ_BOUNDS", "hamerly")
    p["from_kmpp"] = p["tiles"] and track_k == k and same_P and P and not e.zero("KMPP_TRACK") and seeds
    p["pt_sorted"] = not e.zero("PT_SORT")
    p["delta_sums"] = not e.is_("PROJ_SUMS", "fresh") and D < (1 << 31)
    p["movers"] = not e.zero("YY_MOVERS") and D > 0
    return {n: int(v) for n, v in p.items()}


PROJ_ENVS = [{}, {"NO_HAMERLY": "0"}, {"PROJ_BOUNDS": "hamerly"}, {"PROJ_BOUNDS": "tiles"}, {"KMPP_TRACK": "0"}, {"PT_SORT": "0"}, {"PT_SORT": "1"},
             {"PROJ_SUMS": "fresh"}, {"PROJ_SUMS": "delta"}, {"YY_MOVERS": "0"}, {"YY_MOVERS": ""}]


@pytest.mark.parametrize("env", PROJ_ENVS)
def test_projected_plan(exe, env):
    e = Env(env)
    cases = [((D, 1, 0, 1, k, 1, 1), k) for D in (0, 4000, 2 ** 31 - 1, 2 ** 31) for k in KS_TILES]
    cases += [((4000, Pt, Pt2, 1, 225, 1, 1), 225) for Pt in (0, 1) for Pt2 in (0, 1)]
    cases += [((4000, 1, 1, P, tk, sp, sd), k) for P in (0, 1) for tk in (224, 225) for k in (224, 225) for sp in (0, 1) for sd in (0, 1)]
    script = [["proj"] + list(f) + [k] for f, k in cases]
    for line, o in zip(script, run(exe, env, script)):
        assert o == proj_py(e, line[1:8], line[8]), line
    free = proj_py(Env({}), (4000, 1, 0, 1, 225, 1, 1), 225)
    assert (free["tiles"], free["from_kmpp"], free["T"], free["TL"]) == (1, 1, 8, 8) and not proj_py(Env({}), (4000, 1, 0, 1, 224, 1, 1), 224)["tiles"]
    assert proj_py(Env({}), (4000, 1, 0, 1, 1024, 1, 1), 1024)["tiles"] and not proj_py(Env({}), (4000, 1, 0, 1, 1025, 1, 1), 1025)["tiles"]
    assert proj_py(Env({}), (2 ** 31 - 1, 1, 0, 1, 64, 1, 1), 64)["delta_sums"] and not proj_py(Env({}), (2 ** 31, 1, 0, 1, 64, 1, 1), 64)["delta_sums"]


@pytest.mark.parametrize("env", [{}, {"PT_SORT": "0"}, {"PT_SORT": "1"}, {"PT_SORT": ""}])
def test_sort_of_the_active_list(exe, env):
    script = [["pt_sort", h, n] for h in (0, 1) for n in (0, 256, 257, 2 ** 32 - 1)]
    for (_, h, n), o in zip(script, run(exe, env, script)):
        assert o["sort"] == b(h and n > 256 and not Env(env).zero("PT_SORT"))


def full_by_gemm_py(e, Pt, Pt2, D, k, total):
    pf = e.get("PROJ_FULL")
    ask = 0
    room = fused_ok_py(e, D, k, k)
    if (Pt or Pt2) and D > 0 and k >= 64 and not room:
        room, ask = scratch_py(float(D) * k * 4, total)
    ok = (Pt or Pt2) and D > 0 and k >= 64 and room and ((2.0 * float(D) * k * k >= 2e10 and not pf == "fused") or pf == "gemm")
    return b(ok), ask


@pytest.mark.parametrize("env", [{}, {"PROJ_FULL": "gemm"}, {"PROJ_FULL": "fused"}, {"PROJ_FULL": "other"}, {"PROJ_FULL": ""}, {"GEMM_EPILOGUE": "0"}])
def test_full_pass_by_gemm(exe, env):
    """2 D k^2 = 2e10 at k = 100: D = 10^6 takes the product, D = 999 999 the register kernel"""
    e = Env(env)
    cases = [(Pt, Pt2, D, k, t) for Pt, Pt2 in ((1, 0), (0, 1), (0, 0)) for D, k in ((0, 100), (999999, 100), (1000000, 100), (10 ** 7, 63), (10 ** 7, 64),
                                                                                   (4000, 1000), (10 ** 7, 1000), (6 * 10 ** 7, 1000)) for t in (0, MI355X)]
    for c, o in zip(cases, run(exe, env, [["full"] + list(c) for c in cases])):
        assert (o["by_gemm"], o["ask"]) == full_by_gemm_py(e, *c), c
    assert 2.0 * 1000000.0 * 100 * 100 >= 2e10 > 2.0 * 999999.0 * 100 * 100
    if not env:
        assert full_by_gemm_py(e, 1, 0, 1000000, 100, 0) == (1, 0) and full_by_gemm_py(e, 1, 0, 999999, 100, 0) == (0, 0)
    if env == {"GEMM_EPILOGUE": "0"}:  # the 40 GB scratch of config 3: a fifth of the device holds it, and it is the device that is asked
        assert full_by_gemm_py(e, 1, 0, 10 ** 7, 1000, 0) == (0, 1) and full_by_gemm_py(e, 1, 0, 10 ** 7, 1000, MI355X) == (1, 0)
        assert full_by_gemm_py(e, 1, 0, 6 * 10 ** 7, 1000, MI355X) == (0, 0)


@pytest.mark.parametrize("env", [{}, {"PROJ_ACTIVE": "gemm"}, {"PROJ_ACTIVE": "tiles"}, {"PROJ_ACTIVE": ""}, {"GEMM_BF16X3": "0"}])
def test_active_rows(exe, env):
    e = Env(env)
    cases = [(130816, 256), (130817, 256), (65281, 257), (10, 1000)]
    for (n, k), o in zip(cases, run(exe, env, [["active", n, k] for n, k in cases])):
        assert o["by_gemm"] == b((e.get("PROJ_ACTIVE") == "gemm" if e.on("PROJ_ACTIVE") else True) and fused_ok_py(e, n, k, k)), (n, k)


# ---- Lloyd on B -----------------------------------------------------------------------------------------------------------------------------
def sparse_py(e, f, k, ld, total):
    D, nnz, lift_valid, lift_k, U_k, ldk, P, Pt, Pt2 = f
    p, ask = {}, 0
    p["hamerly"] = not e.on("NO_HAMERLY") and not e.is_("KMEANS_BOUNDS", "none")
    p["yinyang"] = p["hamerly"] and not e.is_("KMEANS_BOUNDS", "hamerly")
    p["G"] = G = (k + 7) // 8
    m = e.get("YY_MODE")
    yy_env = {"doc": 0, "docg": 1, "group": 2}.get(m, -1)
    p["yy_mode"] = 0 if not p["yinyang"] else 0 if G > 256 else yy_env if yy_env >= 0 else (2 if G >= 32 else 0)
    p["fused"] = p["yy_mode"] == 2 and not e.zero("YY_FUSED")
    yord = e.get("YY_ORDER")
    p["by_members"] = not p["yinyang"] or not p["yy_mode"] or ((yord != "doc") if yord is not None else not p["fused"])
    p["movers"] = p["fused"] and not e.zero("YY_MOVERS")
    t_dense, t_sparse = 2.0 * float(D) * k * k / 130e12, float((k + 7) // 8) * float(nnz) * 2.8e-12
    p["fused_first"] = p["yinyang"] and fused_ok_py(e, D, k, k)
    dense_pays = k <= 384
    if not dense_pays and t_dense < t_sparse:
        dense_pays = p["fused_first"]
        if not dense_pays:
            dense_pays, ask = scratch_py(float(D) * k * 4, total)
    p["via_projection"] = (lift_valid and lift_k == k and U_k == k and P and (Pt or Pt2) and ldk == ld and D > 0 and
                           (dense_pays or e.is_("FIRST_ASSIGN", "projection")) and not e.is_("FIRST_ASSIGN", "sparse"))
    p["regroup"] = p["yinyang"] and p["yy_mode"] == 2 and p["via_projection"] and p["fused_first"] and not e.zero("YY_REGROUP")
    p["ask"] = ask
    return {n: int(v) for n, v in p.items()}


def facts(D, nnz, k, **kw):
    f = dict(D=D, nnz=nnz, lift_valid=1, lift_k=k, U_k=k, ldk=(k + 3) & ~3, P=1, Pt=0, Pt2=1)
    f.update(kw)
    return [f[n] for n in ("D", "nnz", "lift_valid", "lift_k", "U_k", "ldk", "P", "Pt", "Pt2")]


SPARSE_ENVS = [{}, {"NO_HAMERLY": ""}, {"KMEANS_BOUNDS": "hamerly"}, {"KMEANS_BOUNDS": "none"}, {"KMEANS_BOUNDS": "yinyang"}, {"YY_MODE": "doc"}, {"YY_MODE": "docg"},
               {"YY_MODE": "group"}, {"YY_MODE": "groups"}, {"YY_FUSED": "0"}, {"YY_MOVERS": "0"}, {"YY_REGROUP": "0"}, {"YY_ORDER": "doc"}, {"YY_ORDER": "member"},
               {"YY_ORDER": ""}, {"YY_ORDER": "doc", "YY_FUSED": "0"}, {"FIRST_ASSIGN": "sparse"}, {"FIRST_ASSIGN": "projection"}, {"FIRST_ASSIGN": "dense"},
               {"GEMM_EPILOGUE": "0"}]


@pytest.mark.parametrize("env", SPARSE_ENVS)
def test_sparse_plan(exe, env):
    e = Env(env)
    cases = []
    for k in (8, 248, 249, 256, 384, 385, 1000, 2048, 2049):
        for D, nnz in ((0, 0), (4000, 400000), (1250000, 125 * 10 ** 6), (10 ** 7, 10 ** 9), (6 * 10 ** 7, 6 * 10 ** 9)):
            for total in (0, MI355X):
                cases.append((facts(D, nnz, k), k, (k + 3) & ~3, total))
    k = 249
    for kw in (dict(lift_valid=0), dict(lift_k=248), dict(U_k=248), dict(ldk=256), dict(P=0), dict(Pt2=0), dict(Pt2=0, Pt=1)):
        cases.append((facts(1250000, 125 * 10 ** 6, k, **kw), k, 252, 0))
    for (f, k, ld, total), o in zip(cases, run(exe, env, [["sparse"] + f + [k, ld, total] for f, k, ld, total in cases])):
        assert o == sparse_py(e, f, k, ld, total), (f, k, ld, total)
    if not env:
        at = lambda k, D=1250000, nnz=125 * 10 ** 6: sparse_py(e, facts(D, nnz, k), k, (k + 3) & ~3, 0)  # noqa: E731
        assert [(at(k)["G"], at(k)["yy_mode"], at(k)["by_members"], at(k)["regroup"]) for k in (248, 249, 2048, 2049)] == \
            [(31, 0, 1, 0), (32, 2, 0, 1), (256, 2, 0, 1), (257, 0, 1, 0)]
        assert at(384, D=4000, nnz=1)["via_projection"] and not at(385, D=4000, nnz=1)["via_projection"]  # no nonzeros to speak of: the sparse product is free


def test_first_assignment_by_cost(exe):
    """k = 1000 on the shard of config 3: nnz either side of 2 D k^2 / 130e12 = ceil(k / 8) nnz 2.8e-12"""
    k, D = 1000, 1250000
    e = Env({})
    pays = lambda nnz: sparse_py(e, facts(D, nnz, k), k, 1000, 0)["via_projection"]  # noqa: E731
    edge = first_true(pays, 1, 10 ** 12)
    assert abs(125 * edge * 2.8e-12 / (2.0 * D * k * k / 130e12) - 1.0) < 1e-6  # (one nonzero is 2e-8 of the edge)
    script = [["sparse"] + facts(D, nnz, k) + [k, 1000, 0] for nnz in (edge - 1, edge)]
    assert [o["via_projection"] for o in run(exe, {}, script)] == [0, 1]
    # beyond the fused product (epilogue off) the 5 GB scratch is taken without asking, the 40 GB of all of config 3 after asking
    env = {"GEMM_EPILOGUE": "0"}
    script = [["sparse"] + facts(D_, 100 * D_, k) + [k, 1000, t] for D_ in (1250000, 10 ** 7, 6 * 10 ** 7) for t in (0, MI355X)]
    got = [(o["via_projection"], o["ask"]) for o in run(exe, env, script)]
    assert got == [(1, 0), (1, 0), (0, 1), (1, 0), (0, 1), (0, 0)]
    assert got == [tuple(sparse_py(Env(env), line[1:10], k, 1000, line[12])[n] for n in ("via_projection", "ask")) for line in script]


@pytest.mark.parametrize("env", [{}, {"CENTERS_FRESH": "1"}, {"CENTERS_FRESH": "0"}, {"CENTERS_FRESH": ""}])
def test_centroid_counts(exe, env):
    fresh = Env(env).on("CENTERS_FRESH")
    script = [["centres", it, bm, gl, first] for it in (0, 1, 5) for bm in (0, 1) for gl in (-1, 0, 1) for first in (0, 1)]
    for (_, it, bm, gl, first), o in zip(script, run(exe, env, script)):
        assert o == dict(lists=b(it == 0 or bm or gl != 1 or fresh), fresh=b(first or fresh)), (it, bm, gl, first)


# ---- spmm.hip, gram_lds.hip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"WIDE_GATHER": "0"}, {"WIDE_LDS": "0"}, {"WIDE_GATHER": "", "WIDE_LDS": ""}])
def test_wide_products(exe, env):
    e = Env(env)
    script = [["wide", V, ldk] for V in (1, 109184, 109185, 2 ** 33) for ldk in (4, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)]
    for (_, V, ldk), o in zip(script, run(exe, env, script)):
        nit = (ldk // 4 + 63) // 64
        want_nit = 1 if nit <= 1 else 2 if nit <= 2 else 4 if nit <= 4 else 8 if nit <= 8 else 0  # 0: refused (k > 2048)
        assert o == dict(lds=b(False if e.on("WIDE_GATHER") else True if e.on("WIDE_LDS") else V <= 32 * 3412), nit=want_nit), (V, ldk)
    assert 32 * 3412 == 109184


GL_ENVS = [{}, {"GRAM_LDS": "0"}, {"GRAM_LDS": "1"}, {"GRAM_LDS": ""}, {"GRAM_LDS": "x"}, {"GL_G1": "3", "GL_G2": "9"}, {"GL_G1": "6"}, {"GL_ROUNDS": "0"},
           {"GL_COLUMNS": "0"}, {"GL_FILL_BUCKETS": "0"}, {"GL_PANEL": "8"}, {"GL_PANEL": "10"}, {"GL_PANEL": "12"}, {"GL_PANEL": ""}, {"GL_TEST_CUS": "3"}]


@pytest.mark.parametrize("env", GL_ENVS)
def test_banded_operator(exe, env):
    e = Env(env)
    lim = 0xfffffff0
    cases = [(nnz, D, V, n_out, G) for nnz, D, V in ((0, 5, 5), (9, 0, 5), (9, 5, 0), (9, 5, 5), (9, lim - 1, 5), (9, lim, 5), (9, 5, lim - 1), (9, 5, lim))
             for n_out, G in ((2 ** 20, 7), (2 ** 20 + 1, 8))] + [(9, 5, 5, 100, G) for G in (4, 5, 6)]
    panel = atoi(e.get("GL_PANEL")) if e.on("GL_PANEL") else None
    for (nnz, D, V, n_out, G), o in zip(cases, run(exe, env, [["gl"] + list(c) for c in cases])):
        want = dict(eligible=b(not (e.on("GRAM_LDS") and atoi(e.get("GRAM_LDS")) == 0) and nnz > 0 and D > 0 and V > 0 and D < lim and V < lim),
                    g1=max(4, min(8, atoi(e.get("GL_G1")))) if e.on("GL_G1") else 0, g2=max(4, min(8, atoi(e.get("GL_G2")))) if e.on("GL_G2") else 0,
                    rounds=b(not e.zero("GL_ROUNDS")), columns=b(not e.zero("GL_COLUMNS")), test_cus=0,  # the test hook stays with the build
                    bucketed=b(n_out <= (1 << 20) and nnz and not e.zero("GL_FILL_BUCKETS")),
                    panel=10 if panel == 10 else 8 if panel == 8 else (10 if G <= 7 else 8))
        assert o == want, (nnz, D, V, n_out, G)


@pytest.mark.parametrize("env", [{}, {"GL_WIDE_GROUPED": "0"}, {"GL_WIDE_GROUPED": "1"}, {"GL_WIDE_GROUPED": ""}])
def test_grouped_wide_form(exe, env):
    """k = 159 / 160, D = 16 383 / 16 384, panels of 8 (8 items per lane in pass 1) against 10 (7), and the slabs against the scratch rule"""
    e = Env(env)
    widths = [o["panel"] for o in run(exe, {}, [["gl", 9, 5, 5, 100, G] for G in (7, 8)])]
    assert widths == [10, 8]
    cases = [(n, PW, k, D, 16, t) for n in (0, 1) for PW in widths for k in (159, 160, 1000) for D in (16383, 16384, 10 ** 7, 2 * 10 ** 7, 10 ** 8)
             for t in (0, MI355X)]
    for (n, PW, k, D, wg, t), o in zip(cases, run(exe, env, [["grouped"] + list(c) for c in cases])):
        ngroups = (k + PW * wg - 1) // (PW * wg)
        ok, ask = 0, 0
        if n and PW == 10 and k >= 160 and D >= 16384 and not e.zero("GL_WIDE_GROUPED"):
            ok, ask = scratch_py(float(D * 12 * wg + ngroups * D) * 4, t)
        assert (o["grouped"], o["ask"]) == (ok, ask), (n, PW, k, D, t)
    assert scratch_py(float(10 ** 7 * 12 * 16 + 7 * 10 ** 7) * 4, 0) == (1, 0) and scratch_py(float(2 * 10 ** 7 * 12 * 16 + 7 * 2 * 10 ** 7) * 4, 0) == (0, 1)


# ---- evd_tridiag.hip --------------------------------------------------------------------------------------------------------------------
TD_P_LDS, TD_P_GSMALL, TD_NMAX_BACK = 160 * 1024 - 512, 32, 2048


def td_py(e, n, lds, gsmall, nmax, cus, failed):
    ncl_max = lds // 8 // n - 2
    pG = max(gsmall, (n + ncl_max - 1) // ncl_max) if ncl_max >= 1 else 1 << 30
    return dict(pG=pG, persist=b(pG <= cus and n <= nmax and not e.on("TD_CHAIN") and not failed))


@pytest.mark.parametrize("env", [{}, {"TD_CHAIN": "1"}, {"TD_CHAIN": "0"}, {"TD_CHAIN": ""}])
def test_persistent_tridiagonalisation(exe, env):
    e = Env(env)
    free = Env({})
    # the largest n whose LDS-derived workgroup count still fits 256 CUs, and the next
    n_fit = first_true(lambda n: td_py(free, n, TD_P_LDS, TD_P_GSMALL, TD_NMAX_BACK, 256, 0)["pG"] > 256, 16, 4096) - 1
    assert td_py(free, n_fit, TD_P_LDS, 32, 2048, 256, 0)["persist"] and not td_py(free, n_fit + 1, TD_P_LDS, 32, 2048, 256, 0)["persist"] and n_fit < 2048
    ns = [16, 410, 512, 2010, n_fit, n_fit + 1, 2048, 2049, 6805, 6806, 20000, 30000]
    cases = [(n, lds, 32, nmax, cus, f) for n in ns for lds, nmax in ((TD_P_LDS, 2048), (4 * TD_P_LDS, 2048), (4 * TD_P_LDS, 4096)) for cus in (255, 256, 304)
             for f in (0, 1)]
    for c, o in zip(cases, run(exe, env, [["td"] + list(c) for c in cases])):
        assert o == td_py(e, *c), c
    # with LDS to spare, n decides at TD_NMAX_BACK; at n = 410 the 32 workgroups of the small sizes; n beyond the LDS: no persistent form
    wide = lambda n: td_py(free, n, 4 * TD_P_LDS, 32, 2048, 256, 0)  # noqa: E731
    assert wide(2048)["persist"] and not wide(2049)["persist"] and wide(2049)["pG"] <= 256
    assert td_py(free, 410, TD_P_LDS, 32, 2048, 256, 0)["pG"] == 32 and td_py(free, 6806, TD_P_LDS, 32, 2048, 256, 0)["pG"] == 1 << 30 > td_py(free, 6805, TD_P_LDS, 32, 2048, 256, 0)["pG"]


@pytest.mark.parametrize("env", [{}, {"EVD_SPLIT": "1"}, {"EVD_SPLIT": "0"}, {"EVD_SPLIT": ""}, {"EVD_SPLIT": "2"}])
def test_vector_split(exe, env):
    e = Env(env)
    on = e.on("EVD_SPLIT") and not e.zero("EVD_SPLIT")
    cases = [(m, w, r, nvec, n) for m in (0, 1) for w, nvec, n in ((8, 2000, 2010), (8, 2010, 2010), (8, 250, 255), (8, 250, 256), (8, 9, 63), (8, 9, 64), (2, 5, 16),
                                                                   (2, 5, 15), (1, 100, 200), (3, 100, 200)) for r in range(w)]
    for (m, w, r, nvec, n), o in zip(cases, run(exe, env, [["td_split"] + list(c) for c in cases])):
        v0, v1, kc = 0, nvec, 0
        if m and on:
            kc = ((nvec + w - 1) // w + 7) & ~7
            if kc * w <= n:
                v0 = min(nvec, r * kc)
                v1 = min(nvec, v0 + kc)
            else:
                kc = 0
        assert o == dict(v0=v0, v1=v1, kc=kc), (m, w, r, nvec, n)
    if env == {"EVD_SPLIT": "1"}:  # kc * world <= n: 8 x 32 = 256 columns fit n = 256, not n = 255
        got = run(exe, env, [["td_split", 1, 8, 7, 250, 255], ["td_split", 1, 8, 7, 250, 256]])
        assert got == [dict(v0=0, v1=250, kc=0), dict(v0=224, v1=250, kc=32)]


@pytest.mark.parametrize("env", [{}, {"TD_BACK": "seq"}, {"TD_BACK": "s"}, {"TD_BACK": "wy"}, {"TD_BACK": ""}, {"TD_BACK": "Seq"}])
def test_back_transformation(exe, env):
    e = Env(env)
    seq = e.on("TD_BACK") and e.get("TD_BACK")[:1] == "s"
    cases = [(nvec, cus, kc) for nvec in (1, 1016, 1024, 1025, 1032, 2010) for cus in (255, 256, 257) for kc in (0, 32)]
    for (nvec, cus, kc), o in zip(cases, run(exe, env, [["td_back"] + list(c) for c in cases])):
        assert o["back"] == (0 if not seq else 8 if (nvec + 7) // 8 > cus // 2 and not kc else 4), (nvec, cus, kc)
    assert (1024 + 7) // 8 == 256 // 2 and (1025 + 7) // 8 > 256 // 2
