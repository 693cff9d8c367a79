"""isle_amd/csrc/gl_plan.h, the host plan of the LDS-banded operator build, without the library and without a GPU: gl_plan_main is built here
with the address and undefined-behaviour sanitizers (a stand-alone program) and prints the plan of a case as JSON.  Checked: the scalars the
project recorded on hardware (profiles/r06_r_ranked_slices_probe.log lines 2 and 13, profiles/r05_gl_apply_item3_measurements.txt line 34),
the whole-rounds rule at test scale, and for every case the conditions under which gl_apply_k computes every output item exactly once —
every slice dealt to one (wave, group), every wave reached by one workgroup, pass 2's band ranges and slabs a partition per word block."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL_RB = 4078


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gl_plan") / "gl_plan_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "gl_plan_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out


_plans = {}


def plan(exe, nnz, D, V, cus, *opts):
    key = (nnz, D, V, cus) + opts
    if key not in _plans:
        r = subprocess.run([exe, str(nnz), str(D), str(V), str(cus)] + list(opts), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        _plans[key] = json.loads(r.stdout)
        assert _plans[key]["GL_RB"] == GL_RB
    return _plans[key]


def opt(opts, name, default):
    for o in opts:
        if o.startswith(name + "="):
            return o.split("=")[1]
    return default


def check_slices(g, none):
    """slice_of has nwv x G entries; every slice of [0, nslice) appears exactly once, the rest is GL_NONE"""
    so = g["slice_of"]
    assert len(so) == g["nwv"] * g["G"]
    real = [s for s in so if s != none]
    assert sorted(real) == list(range(g["nslice"]))


def check_pass1(j, D, V, cus, opts):
    p = j["pass1"]
    eff_cus = int(opt(opts, "test_cus", cus))
    rounds_on = opt(opts, "rounds", "1") != "0"
    assert p["NB"] == -(-V // GL_RB) and p["nslice"] == -(-D // 64) and 4 <= p["G"] <= 8 and 1 <= p["wpg"] <= 16
    if opt(opts, "g1", None):
        assert p["G"] == int(opt(opts, "g1", None))
    check_slices(p, j["GL_NONE"])
    reached = []
    for wave0, wstride, nw, b0, b1, slab, pos_base, pad in p["desc"]:
        assert nw <= p["wpg"] and b0 == 0 and b1 == p["NB"] and slab == 0 and pos_base == 0 and pad == 0
        reached += [wave0 + i * wstride for i in range(nw)]
    assert sorted(reached) == list(range(p["nwv"]))  # every wave by exactly one (descriptor, i < nw)
    strided_waves = -(-p["nslice"] // p["G"])
    strided_wgs = -(-strided_waves // p["wpg"])
    assert p["adjacent"] == (strided_wgs > eff_cus and rounds_on)
    if p["adjacent"]:
        assert len(p["desc"]) % eff_cus == 0 and p["nwv"] == len(p["desc"]) * p["wpg"] and all(d[1] == 1 for d in p["desc"])
    else:
        assert p["nwv"] == strided_waves and len(p["desc"]) == strided_wgs


def check_pass2(j, D, V, opts):
    p = j["pass2"]
    NB, nblk, wpb, bitems = p["NB"], p["nblk"], p["wpg"], p["bitems"]
    assert p["error"] is None
    assert NB == -(-D // GL_RB) and p["nslice"] == -(-V // 64)
    assert p["G"] == (int(opt(opts, "g2", 0)) or (6 if NB > 1024 else 4))
    assert wpb in (1, 2, 4, 8, 16) and bitems == 64 * p["G"] * wpb and nblk == -(-p["nslice"] // (p["G"] * wpb)) and p["nwv"] == nblk * wpb
    check_slices(p, j["GL_NONE"])
    for wv in range(p["nwv"]):  # a word block's slices stay inside the block: pos - pos_base indexes its slab
        for s in p["slice_of"][wv * p["G"]:(wv + 1) * p["G"]]:
            assert s == j["GL_NONE"] or s * 64 // bitems == wv // wpb
    columns = p["columns"]
    assert columns == (NB >= 16 and opt(opts, "columns", "1") != "0")
    # per block: the band ranges partition [0, NB), the slabs are slab0 .. slab0 + nch - 1, each once
    by_block = {ob: [] for ob in range(nblk)}
    for i, (wave0, wstride, nw, b0, b1, slab, pos_base, pad) in enumerate(p["desc"]):
        if nw == 0:
            assert columns and (b0, b1) == (0, 0)  # a filler of an XCD queue: no wave is valid, no band walked
            continue
        assert wave0 % wpb == 0 and nw == wpb and wstride == 1 and pos_base == wave0 // wpb * bitems and pad == 0
        by_block[wave0 // wpb].append((b0, b1, slab, i))
    assert len(p["slab0"]) == nblk and len(p["nch"]) == nblk
    run = 0
    for ob in range(nblk):
        assert p["slab0"][ob] == run  # the exclusive prefix of nch
        run += p["nch"][ob]
        chunks = sorted(by_block[ob])
        assert [c[0] for c in chunks] == [0] + [c[1] for c in chunks[:-1]] and chunks[-1][1] == NB and all(c[0] < c[1] for c in chunks)
        assert sorted(c[2] for c in chunks) == list(range(p["slab0"][ob], p["slab0"][ob] + p["nch"][ob]))
    assert p["nslab"] == run
    if not columns:
        assert p["cut"] == []
        return
    cut = p["cut"]
    NC = len(cut) - 1
    assert NC % 8 == 0 and 8 <= NC <= NB
    assert cut[0] == 0 and cut[-1] == NB and all(a < b for a, b in zip(cut, cut[1:]))
    assert len(p["desc"]) % 8 == 0
    col_of = {}
    for cc in range(NC):
        for b in range(cut[cc], cut[cc + 1]):
            col_of[b] = cc
    for ob in range(nblk):
        for b0, b1, slab, i in by_block[ob]:
            cc = col_of[b0]
            assert b1 <= cut[cc + 1]       # no descriptor crosses a cut
            assert cc % 8 == i % 8         # a column's workgroups are queued on one XCD


def check(exe, nnz, D, V, cus, *opts):
    j = plan(exe, nnz, D, V, cus, *opts)
    check_pass1(j, D, V, cus, opts)
    check_pass2(j, D, V, opts)
    return j


# ---- the scalars recorded on hardware ---------------------------------------------------------------------------------------------------
def test_config_3_on_one_gpu(exe):
    j = check(exe, 1006280745, 10_000_000, 100_000, 256)
    p1, p2 = j["pass1"], j["pass2"]
    assert (p1["NB"], p1["G"], p1["wpg"], p1["nwv"], len(p1["desc"]), p1["adjacent"]) == (25, 7, 16, 24576, 1536, True)
    assert (p2["NB"], p2["G"], p2["nblk"]) == (2453, 6, 17)


def test_a_config_3_shard(exe):
    j = check(exe, 125925867, 1_250_000, 100_000, 256)
    p1, p2 = j["pass1"], j["pass2"]
    assert (p1["NB"], p1["G"], p1["nwv"], len(p1["desc"]), p1["adjacent"]) == (25, 5, 3907, 245, False)
    assert (p2["NB"], p2["G"], p2["nblk"]) == (307, 4, 25)


@pytest.mark.parametrize("cus,want", [(3, (4, 16, 144, 9, True)), (7, (4, 16, 224, 14, True)), (256, (4, 1, 118, 118, False))])
def test_whole_rounds_at_test_scale(exe, cus, want):
    opts = ("test_cus=%d" % cus,) if cus != 256 else ()
    p1 = check(exe, 600_000, 30_000, 3_000, 256, *opts)["pass1"]
    assert (p1["G"], p1["wpg"], p1["nwv"], len(p1["desc"]), p1["adjacent"]) == want


def test_rounds_off_is_strided(exe):
    p1 = check(exe, 600_000, 30_000, 3_000, 256, "test_cus=3", "rounds=0")["pass1"]
    assert not p1["adjacent"] and p1["nwv"] == -(-p1["nslice"] // p1["G"])


# ---- the smallest cases at which each rule can go wrong ------------------------------------------------------------------------------------
TOTS = ("tot=zero", "tot=uniform", "tot=skew")
EDGES = ([(D, 3000) for D in (1, 63, 64, 65, 4078, 4079)]        # slices of 64 documents; one and two document bands
         + [(30_000, V) for V in (1, 64, 65, 4078, 4079)])       # fewer slices than G; one and two word bands


@pytest.mark.parametrize("D,V", EDGES)
@pytest.mark.parametrize("cus", (3, 256))
def test_slice_and_band_edges(exe, D, V, cus):
    for tot in TOTS:
        check(exe, 20 * D, D, V, cus, tot)


@pytest.mark.parametrize("D", (61170, 61171))  # 15 and 16 document bands
@pytest.mark.parametrize("columns", ("columns=1", "columns=0"))
@pytest.mark.parametrize("V", (64, 3000, 100_000))  # V = 64: nblk = 1
def test_fifteen_and_sixteen_bands(exe, D, columns, V):
    for tot in TOTS:
        j = check(exe, 20 * D, D, V, 256, columns, tot)
        assert j["pass2"]["columns"] == (D == 61171 and columns == "columns=1")
    if V == 64:
        assert j["pass2"]["nblk"] == 1


@pytest.mark.parametrize("V", (3000, 100_000))
def test_1026_bands_take_six_items_per_lane(exe, V):
    for tot in TOTS:
        p2 = check(exe, 80_000_000, 4_180_000, V, 256, tot)["pass2"]
        assert p2["NB"] == 1026 and p2["G"] == 6 and p2["columns"]


@pytest.mark.parametrize("g", (4, 8))
@pytest.mark.parametrize("D,V,cus", [(30_000, 3000, 3), (30_000, 3000, 256), (61171, 100_000, 256), (65, 65, 256)])
def test_forced_items_per_lane(exe, g, D, V, cus):
    for tot in TOTS:
        j = check(exe, 20 * D, D, V, cus, "g1=%d" % g, "g2=%d" % g, tot)
        assert j["pass1"]["G"] == g and j["pass2"]["G"] == g
