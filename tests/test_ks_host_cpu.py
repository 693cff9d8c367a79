"""isle_amd/csrc/ks_host.h, the host side of the block Krylov-Schur solver, without the library and without a GPU: ks_host_main is built here
with the address and undefined-behaviour sanitizers (a stand-alone program) and replays a script that this file sends on stdin.  Every
matrix entry is a small integer held in float32, so every sum and product of the fold and of the truncation is exact and H is compared with
==; the expected values come from the numpy statement of the same rules below (slices and one matmul).  Checked besides: the argument rule at
its boundaries, the mailbox and staging layouts, the row slices of the sharded orthogonalisation, the residual test and the final counts."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ks_host") / "ks_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "ks_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, script):
    """script: a list of token lists -> one dict per command"""
    text = "\n".join(" ".join(str(t) for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["cmd"] for o in out] == [line[0] for line in script]
    return out


def cm(M):
    """column-major tokens of a matrix of whole numbers"""
    return [int(v) for v in np.asarray(M).flatten(order="F")]


def got_H(o):
    return np.array(o["a"], F32).reshape((o["r"], o["c"]), order="F")


class Replay:
    """The numpy statement of the rules next to the script that makes ks_host_main apply them: every method appends a command and the H
    (and scalars) it must answer with."""

    def __init__(self, nev, ncv, blk, seed):
        self.nev, self.ncv, self.b = nev, ncv, blk
        self.rng = np.random.default_rng(seed)
        self.script = [["nev", nev], ["ncv", ncv], ["blk", blk]]
        self.want = [None, None, None]
        self.H = None
        self.ld = self.cap_c = 0

    def ints(self, r, c):
        return self.rng.integers(-4, 5, size=(r, c)).astype(F32)

    def _expect(self, line, **kw):
        self.script.append(line)
        self.want.append(dict(H=self.H.copy(), ld=self.ld, cap_c=self.cap_c, **kw))

    def start(self, rank):
        b = self.b
        c1, c2, R = self.ints(b, b), self.ints(b, b), self.ints(rank, b)
        self.H = np.zeros((2 * b, b), F32)
        self.H[:b] = c1 + c2
        self.H[b:b + rank] = R
        self.ld = max(self.ncv, 2 * b) + b      # room for the expansion: whole blocks to at least ncv rows, and one more
        self.cap_c = b + self.ld - 2 * b
        self._expect(["start", rank] + cm(c1) + cm(c2) + cm(R))

    def tight(self, r, c):
        self.H = self.ints(r, c)
        self.ld, self.cap_c = r, c
        self._expect(["tight", r, c] + cm(self.H))

    def reserve(self):
        r, c = self.H.shape
        cap_r = max(self.ncv, r) + self.b
        cap_c = c + cap_r - r
        grew = self.ld < cap_r or self.cap_c < cap_c
        if grew:
            self.ld, self.cap_c = max(r, cap_r), max(c, cap_c)
        self._expect(["reserve"], ask_r=cap_r, ask_c=cap_c)
        return grew

    def fold(self, npass, rk):
        b = self.b
        m, hcn = self.H.shape
        coef = [self.ints(m, b) for _ in range(npass)]
        R = self.ints(rk, b)
        Hn = np.zeros((m + b, hcn + b), F32)
        Hn[:m, :hcn] = self.H
        Hn[:m, hcn:] = sum(coef[1:], coef[0])
        Hn[m:m + rk, hcn:] = R
        self.H = Hn
        self._expect(["fold", npass, rk] + [t for c_ in coef for t in cm(c_)] + cm(R))

    def truncate(self, nconv):
        nev, b, H = self.nev, self.b, self.H
        hr, hc = H.shape
        n, keep = hc - nconv, nev - nconv
        eH, vH, top = self.ints(1, n)[0], self.ints(n, keep), self.ints(nconv, keep)
        subH, blkH = H[nconv:hc, nconv:hc].copy(), H[:nconv, nconv:hc].copy()
        newrows = H[hr - b:hr, hc - b:hc] @ vH[n - b:, :]
        Hn = np.zeros((nev + b, nev), F32)
        Hn[:nev, :nconv] = H[:nev, :nconv]
        Hn[nev:nev + b, :nconv] = H[nev:nev + b, :nconv]
        Hn[np.arange(nconv, nev), np.arange(nconv, nev)] = eH[:keep]
        Hn[nev:nev + b, nconv:] = newrows
        Hn[:nconv, nconv:] = top
        self.H = Hn
        self.ld = max(self.ncv, nev + b) + b    # what the next reserve asks for
        self.cap_c = nev + self.ld - (nev + b)
        self._expect(["truncate", nconv] + cm(eH) + cm(vH) + cm(top), subH=subH, blkH=blkH)

    def check(self, exe):
        out = run(exe, self.script)
        for o, w in zip(out, self.want):
            if w is None:
                continue
            assert (o["r"], o["c"]) == w["H"].shape and (got_H(o) == w["H"]).all(), (o["cmd"], got_H(o), w["H"])
            assert o["rest_zero"] and (o["ld"], o["cap_c"]) == (w["ld"], w["cap_c"]) and o["alloc"] == o["ld"] * o["cap_c"], o
            if o["cmd"] == "reserve":
                assert (o["ask_r"], o["ask_c"]) == (w["ask_r"], w["ask_c"]) and o["ld"] >= o["ask_r"] and o["cap_c"] >= o["ask_c"]
            if o["cmd"] == "truncate":
                assert o["subH"] == [float(v) for v in w["subH"].flatten(order="F")]
                assert o["blkH"] == [float(v) for v in w["blkH"].flatten(order="F")]
        return out


# ---- H through whole solves ----------------------------------------------------------------------------------------------------------------
def test_ragged_case_with_deficient_steps_and_two_truncations(exe):
    """blk = 3, nev = 4, ncv = 11: H grows by whole blocks to 12 rows; steps with rk = 2 and rk = 0 write fewer rows of R; truncation
    with nothing locked, then with 0 < nconv < nev after a further expansion, then once more after a three-pass expansion."""
    p = Replay(4, 11, 3, 1)
    p.start(3)
    assert not p.reserve(), "init allocates with the room expand asks for"
    p.fold(2, 3)
    p.fold(2, 2)
    assert p.H.shape == (12, 9)
    p.truncate(0)
    assert not p.reserve(), "truncate allocates with the room the next expand asks for"
    p.fold(2, 0)
    p.fold(2, 3)
    assert p.H.shape == (13, 10)
    p.truncate(2)
    assert not p.reserve()
    p.fold(3, 3)
    p.fold(3, 1)
    p.truncate(3)
    assert not p.reserve()
    p.check(exe)


@pytest.mark.parametrize("nev,blk", [(1, 3), (3, 3), (3, 5)])
def test_block_width_one(exe, nev, blk):
    """nev = 1 and blk >= nev force the block width to 1"""
    b = run(exe, [["args", nev, nev + 3, blk, 2, 100]])[0]
    assert (b["blk"], b["counts"], b["range"]) == (1, 0, 0)
    p = Replay(nev, nev + 3, b["blk"], 2)
    p.start(1)
    p.reserve()
    for npass in (3, 2) + (2,) * (nev - 1):
        p.fold(npass, 1)
    assert p.H.shape[0] == nev + 3
    p.truncate(0)
    p.reserve()
    p.fold(2, 1)
    p.fold(3, 0)
    p.truncate(nev - 1)
    p.check(exe)


def test_deficient_start_block(exe):
    """rank < blk after init: the missing rows of R stay zero"""
    p = Replay(4, 9, 3, 3)
    p.start(2)
    assert (p.H[5] == 0).all()
    p.reserve()
    p.fold(2, 3)
    p.check(exe)


def test_reserve_reallocates_a_tight_matrix(exe):
    """HMat(r, c) has no room to grow (the path the solver itself never takes): contents kept, the new room zero, and a step fits"""
    p = Replay(2, 7, 2, 4)
    p.tight(4, 2)
    assert p.reserve()
    assert (p.ld, p.cap_c) == (9, 7)
    p.fold(2, 2)
    p.fold(3, 1)
    p.check(exe)


# ---- the residual test and the final counts --------------------------------------------------------------------------------------------------
def first_unconverged(H, b, tol, divide):
    for j in range(H.shape[1]):
        s = F32(0)
        for i in range(H.shape[0] - b, H.shape[0]):
            s = F32(s + H[i, j] * H[i, j])
        nrm = np.sqrt(s)
        if divide:
            nrm = F32(nrm / H[j, j])
        if nrm >= F32(tol):
            return j
    return H.shape[1]


# 5 x 3 with blk = 2: the residual rows are the last two; column norms 0, 5, 10 over the diagonal 4, 2, 8
UNCONV_H = np.array([[4, 0, 0], [0, 2, 0], [0, 0, 8], [0, 3, 6], [0, 4, 8]], F32)


@pytest.mark.parametrize("tol,divide,want", [
    (2.5, 1, 1),      # 5 / 2 = 2.5 is exactly tol: unconverged (>=)
    (2.5000002, 1, 3),  # the next float32 above it: every column converged -> H.c (10 / 8 = 1.25)
    (1.25, 1, 1), (5.0, 0, 1), (5.0000005, 0, 2), (10.0, 0, 2), (10.000001, 0, 3), (0.0, 1, 0), (0.0, 0, 0),
])
def test_first_unconverged(exe, tol, divide, want):
    assert first_unconverged(UNCONV_H, 2, tol, divide) == want
    out = run(exe, [["blk", 2], ["tight", 5, 3] + [float(v) for v in UNCONV_H.flatten(order="F")], ["unconv", repr(float(F32(tol))), divide]])
    assert out[2]["j"] == want


@pytest.mark.parametrize("nconv,last_j,restarts,maxit,want", [
    # (nc, nc_ref, noconv); nev = 2, tol = 5: the non-dividing rule finds column 1 (norm 5 >= tol) whatever the restarts did
    (3, 3, 1, 4, (2, 2, False)),   # converged before maxit: both counts are nconv, clipped to nev
    (1, 1, 4, 4, (1, 1, True)),    # maxit exhausted with last_j < nev: NOCONV, nc = last_j
    (0, 0, 4, 4, (0, 1, True)),
    (0, 1, 4, 4, (1, 1, True)),    # nc is the LAST test's count, not the one the last expansion started from
    (2, 2, 4, 4, (2, 1, False)),   # maxit exhausted with last_j >= nev: no error
    (2, 3, 4, 4, (2, 1, False)),
])
def test_final_counts(exe, nconv, last_j, restarts, maxit, want):
    nev, tol = 2, 5.0
    nc = nc_ref = nconv
    noconv = False
    if restarts == maxit:
        nc_ref = first_unconverged(UNCONV_H, 2, tol, False)
        nc = min(last_j, nev)
        noconv = nc < nev
    assert (min(nc, nev), min(nc_ref, nev), noconv) == want
    out = run(exe, [["blk", 2], ["nev", nev], ["tight", 5, 3] + [float(v) for v in UNCONV_H.flatten(order="F")],
                    ["counts", tol, nconv, last_j, restarts, maxit]])
    assert (out[3]["nc"], out[3]["nc_ref"], out[3]["noconv"]) == want


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
def test_mailbox_layout(exe):
    k = run(exe, [["consts"]])[0]
    assert k["slots"] == [k["KS_AGREE"], k["KS_AGREE"] + 1, k["KS_AGREE"] + 2] and k["KS_AGREE"] >= 2  # beside the QR's rank and status
    assert k["KS_AGREE"] + 3 <= k["MB_R"] and k["MB_COEF"] - k["MB_R"] >= 32 * 32
    script = [["mail", cap_r, blk, npass, m] for blk in (1, 3, 32) for cap_r in (2 * blk, 12 + blk, 2010 + blk)
              for npass in (2, 3) for m in sorted({0, blk, cap_r - blk})]
    for line, o in zip(script, run(exe, script)):
        _, cap_r, blk, npass, m = line
        assert o["floats"] == k["MB_COEF"] + 3 * cap_r * blk and o["copied"] == k["MB_COEF"] + npass * m * blk
        assert o["copied"] <= o["floats"]


@pytest.mark.parametrize("text,want", [("-", 2), ("3", 3), ("2", 2), ("1", 2), ("4", 3), ("x", 2)])
def test_ortho_passes(exe, text, want):
    assert run(exe, [["passes", text]])[0]["npass"] == want


@pytest.mark.parametrize("dim,world", [(10, 8), (4096, 8), (4099, 3)])
def test_row_slices(exe, dim, world):
    s = run(exe, [["slice", dim, world]])[0]["slices"]
    assert len(s) == world and len({nloc for nloc, _, _ in s}) == 1 and s[0][0] % 4 == 0 and s[0][0] * world >= dim
    at = 0
    for nloc, r0, r1 in s:  # in rank order, disjoint, the union [0, dim); a rank with rows starts at a multiple of 4, one without is [dim, dim)
        assert r0 == at and r0 <= r1 <= dim and r1 - r0 <= nloc and (r0 % 4 == 0 if r1 > r0 else r0 == dim)
        at = r1
    assert at == dim
    if (dim, world) == (10, 8):
        assert [r1 - r0 for _, r0, r1 in s] == [4, 4, 2, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("n,keep,nconv", [(9, 4, 0), (8, 2, 2), (7, 1, 3), (1410, 400, 600)])
def test_staging_layout(exe, n, keep, nconv):
    s = run(exe, [["stage", n, keep, nconv]])[0]
    sizes = [n * n, n * keep, nconv * n, nconv * keep]  # subH, vH, the locked rows, top
    assert [s["subH"], s["vH"], s["blkH"], s["top"]] == [sum(sizes[:i]) for i in range(4)]
    assert s["bytes"] == 4 * sum(sizes)


# ---- the argument rule ---------------------------------------------------------------------------------------------------------------------
OK, COUNTS, NCV_SMALL, NCV_LARGE = 0, 1, 2, 3


@pytest.mark.parametrize("nev,ncv,blk,maxit,dim,counts,rng", [
    (0, 8, 2, 1, 100, COUNTS, None), (1, 8, 2, 1, 100, OK, OK),
    (4, 8, 0, 1, 100, COUNTS, None), (4, 8, 1, 1, 100, OK, OK),
    (40, 200, 33, 1, 1000, COUNTS, None), (40, 200, 32, 1, 1000, OK, OK),
    (4, 8, 2, 0, 100, COUNTS, None),
    (4, 7, 2, 1, 100, OK, NCV_SMALL), (4, 8, 2, 1, 100, OK, OK),      # nev + 2 blk <= ncv
    (4, 8, 2, 1, 9, OK, NCV_LARGE), (4, 8, 2, 1, 10, OK, OK),         # ncv + blk <= dim
    (4, 5, 9, 1, 6, OK, NCV_SMALL), (4, 6, 9, 1, 6, OK, NCV_LARGE), (4, 6, 9, 1, 7, OK, OK),  # with the effective width 1
])
def test_argument_rule(exe, nev, ncv, blk, maxit, dim, counts, rng):
    o = run(exe, [["args", nev, ncv, blk, maxit, dim]])[0]
    assert o["counts"] == counts
    if counts == OK:
        assert o["blk"] == (blk if blk < nev else 1) and o["range"] == rng
