"""The free k-means++ draw of isle_hip_kmeanspp_projected (no injected seeds) held to the fp64 replay of tests/kmpp_certificate.py.

Exact cases: B of small integers and U = the first k columns of the identity make every float32 operation in front of the draw exact, so
the ordered seeds, the rounds, the residual, min_dist (the last batch not folded in) and C_lowd = P[seeds] must EQUAL the replay's, in
every form the switch table names for these rounds: the default (dice thrown on the device, search_frac_k), ISLE_KMPP_HOST_DICE=1
(kmpp_draw_by_ranks: search_args_k up to 16 dice, search_k beyond), ISLE_KMPP_TRACK=0 / 1 at k > 224 and ISLE_KMPP_SPARSE=0 / 1.  The
thin-product rounds (SPARSE=1) need the LDS-banded operator, which the projection behind set_U builds when every word of B holds one
value: the row-constant cases have it; where it is not built SPARSE=1 is a request the library declines.  Which route the rounds took is
read from the library's own debug lines (ISLE_DEBUG_HAMERLY=1: one line per call of k_kmpp_update) and asserted where a switch forces it;
the report names it beside every form.  The nearest seeds are kept (TRACK) only by the thin-product rounds, so TRACK is swept alone and
together with SPARSE=1.  Every case runs every form, the long shapes (blocks-257, k-1540, exhausted-38) included.  The guard that every
switch of route_kmpp_plan and route_kmpp_sparse has a form needs no GPU: tests/test_kmpp_certificate_cpu.py.

Generic case: the small corpus of the k-means certificate under a random orthonormal U, free seeds, the weak certificate
(kmpp_certificate.admissible) inside its cap of 2 % ambiguous dice, and the residual against the fp64 sum within the summed allowance.

The draw on several ranks (the owner rule at shard edges, holds_last with an empty last shard): tests/test_gpu_kmpp_sharded.py.
"""
import json
import os
import re
import time

import numpy as np
import pytest

import kmpp_certificate as kc
from kmeans_certificate import certify_assignment
from kmpp_certificate import ALL_CASES, BIG_CASES, CASES, Exhausted, exact_P, expected, forms_of

pytestmark = pytest.mark.gpu

REPORT = dict(cases={}, generic={}, walls={})


def _fid(f):
    return ",".join("%s=%s" % (a[10:], b) for a, b in f.items()) or "default"


@pytest.fixture(scope="module", autouse=True)
def kmpp_report():
    """At the end of the module: cases, forms, duplicates, the ambiguous share and the wall time, printed (shown with -s);
    KMPP_CERT_REPORT=<path> writes the same as JSON."""
    t0 = time.time()
    yield REPORT
    REPORT["wall_s"] = round(time.time() - t0, 2)
    lines = ["k-means++ certificate: %d exact cases, %d runs, every one equal to the fp64 replay; %.1f s"
             % (len(REPORT["cases"]), sum(len(c["forms"]) for c in REPORT["cases"].values()), REPORT["wall_s"])]
    for n, c in sorted(REPORT["cases"].items()):
        lines.append("  %-18s D %7d k %4d rounds %4s duplicates %3s zero-add rounds %4s forms %s"
                     % (n, c["D"], c["k"], c["rounds"], c["duplicates"], c["zero_add_rounds"], " | ".join(c["forms"])))
    for k, g in sorted(REPORT["generic"].items()):
        lines.append("  generic k %d: %d of %d dice ambiguous (%.1f %%), %d with a chosen document in their set, widest set %d documents"
                     % (k, g["ambiguous"], g["dice"], 100 * g["share"], g["with_chosen"], g["widest"]))
    print("\n".join(lines))
    path = os.environ.get("KMPP_CERT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


THIN, ON_P = "through thin products of B", "on the projection"


def route_of(case, form, err, banded):
    """The route every round took, as ISLE_DEBUG_HAMERLY=1 names it per call of k_kmpp_update ("thin" / "projection" / "mixed"; "none": no
    round folded a seed).  banded: operator_form() == 1 behind the draw, i.e. the LDS-banded operator is built for this B (every
    row-constant case must have it; a tiny case whose words occur once each has it by accident).  Asserted: SPARSE=1 takes the thin
    products in every round where the operator is banded and the projection in every round where it is not; SPARSE=0 the projection."""
    took = set(re.findall(r"\[k-means\+\+\] \d+ new seeds (%s|%s)" % (THIN, ON_P), err))
    sparse = form.get("ISLE_KMPP_SPARSE")
    assert banded or not case["row_constant"]
    if sparse == "1" and banded:
        assert took <= {THIN}, took
    elif sparse is not None:
        assert took <= {ON_P}, took
    assert took or case["k"] == 1
    return "none" if not took else "mixed" if len(took) == 2 else "thin" if took == {THIN} else "projection"


def _run(hp, case, form, monkeypatch, capfd):
    """the case uploaded afresh (every form starts from its own projection), the switches of the form set, the free draw and min_dist;
    the route of the rounds is checked and noted whether the draw returns or refuses"""
    for a, b in form.items():
        monkeypatch.setenv(a, b)
    monkeypatch.setenv("ISLE_DEBUG_HAMERLY", "1")
    V, vals, rows, offs, U = kc.exact_inputs(case)
    hp.upload_csc(V, vals, rows, offs)
    hp.set_U(U)
    capfd.readouterr()
    try:
        g = hp.kmeans_init_on_projected_space(case["k"], rng_seed=case["rng_seed"])
    finally:
        _note(case, expected(case), form, route_of(case, form, capfd.readouterr().err, hp.operator_form() == 1))
    g["min_dist"] = hp.get_min_dist()
    return g


def _equal(case, g, e, what):
    P = exact_P(case)
    assert np.array_equal(g["seeds"], e["seeds"]), "%s: seeds differ first at %d: %s against the replay's %s" % (
        what, int(np.flatnonzero(g["seeds"] != e["seeds"])[0]), g["seeds"][:12], e["seeds"][:12])
    assert g["rounds"] == e["rounds"], (what, g["rounds"], e["rounds"])
    assert g["residual"] == e["residual"], (what, g["residual"], e["residual"])
    bad = np.flatnonzero(g["min_dist"].view(np.uint32) != e["min_dist"].view(np.uint32))
    assert bad.size == 0, "%s: min_dist of %d documents differs, first %d: %.9g against %.9g" % (
        what, bad.size, bad[0], g["min_dist"][bad[0]], e["min_dist"][bad[0]])
    assert np.array_equal(g["C_lowd"], P[e["seeds"].astype(np.int64)].astype(np.float32)), what


def _note(case, e, form, route):
    c = REPORT["cases"].setdefault(case["name"], dict(D=case["D"], k=case["k"], forms=[],
                                                      rounds=None if isinstance(e, Exhausted) else e["rounds"],
                                                      duplicates=None if isinstance(e, Exhausted) else e["duplicates"],
                                                      zero_add_rounds="100 k" if isinstance(e, Exhausted) else e["zero_add_rounds"]))
    c["forms"].append("%s (%s)" % (_fid(form), route))


def _params(cases):
    return [pytest.param(c, f, id="%s-%s" % (c["name"], _fid(f))) for c in cases for f in forms_of(c)]


@pytest.mark.parametrize("case,form", _params([c for c in CASES if not c.get("raises")]))
def test_free_draw_equals_the_replay(hp, case, form, monkeypatch, capfd):
    g = _run(hp, case, form, monkeypatch, capfd)
    _equal(case, g, expected(case), "%s [%s]" % (case["name"], _fid(form)))


@pytest.mark.parametrize("case,form", _params(BIG_CASES))
def test_free_draw_equals_the_replay_at_the_long_shapes(hp, case, form, monkeypatch, capfd):
    """blocks-257: D = 256 x 4096 + 1, scan_blk_k's carry loop makes its second trip, which no other k-means test reaches.  k-1540 of 1600
    documents: from 1527 seeds on a round throws 41 dice, more than search_frac_k holds, and the one-rank draw goes through
    kmpp_draw_by_ranks for those rounds only."""
    _equal(case, _run(hp, case, form, monkeypatch, capfd), expected(case), "%s [%s]" % (case["name"], _fid(form)))


@pytest.mark.parametrize("form", forms_of(ALL_CASES["exhausted-38"]), ids=_fid)
def test_exhausted_corpus_is_refused_and_the_context_stays_usable(hp, form, monkeypatch, capfd):
    """36 distinct rows and document D - 1 give 37 seeds; the 38th cannot be found: every further round has a zero total, throws the
    die 0, runs off the end of the prefix sums and is clamped to D - 1, a seed already (k_kmpp_update with nc = 0 each time), until the
    refusal after 100 k rounds.  A good case passes on the same context afterwards."""
    from isle_amd import IsleHipError
    case = ALL_CASES["exhausted-38"]
    assert isinstance(expected(case), Exhausted)
    with pytest.raises(IsleHipError, match="k-means\\+\\+ cannot find 38 distinct seeds"):
        _run(hp, case, form, monkeypatch, capfd)
    good = ALL_CASES["exhausted-37"]
    _equal(good, _run(hp, good, form, monkeypatch, capfd), expected(good), "exhausted-37 after the refusal")


def test_second_call_and_injected_copy(hp, monkeypatch, capfd):
    """The same seed twice: the same arrays.  The free run's seeds injected: the same C_lowd and min_dist bits — where the free run had no
    duplicate, so that its rounds added the seeds in the batches the injected schedule adds them in (a skipped duplicate shortens a batch,
    and min_dist leaves out the LAST batch)."""
    case = ALL_CASES["k-65"]
    e = expected(case)
    assert e["duplicates"] == 0
    a = _run(hp, case, {}, monkeypatch, capfd)
    b = hp.kmeans_init_on_projected_space(case["k"], rng_seed=case["rng_seed"])
    b["min_dist"] = hp.get_min_dist()
    c = hp.kmeans_init_on_projected_space(case["k"], inject_seeds=a["seeds"])
    c["min_dist"] = hp.get_min_dist()
    for other in (b, c):
        assert np.array_equal(other["seeds"], a["seeds"]) and other["rounds"] == a["rounds"]
        assert np.array_equal(other["C_lowd"].view(np.uint32), a["C_lowd"].view(np.uint32))
        assert np.array_equal(other["min_dist"].view(np.uint32), a["min_dist"].view(np.uint32))
    assert b["residual"] == a["residual"] == c["residual"]
    dup = ALL_CASES["clustered-36"]  # with duplicates: a second call still returns the same arrays
    a = _run(hp, dup, {}, monkeypatch, capfd)
    b = hp.kmeans_init_on_projected_space(dup["k"], rng_seed=dup["rng_seed"])
    assert np.array_equal(a["seeds"], b["seeds"]) and a["rounds"] == b["rounds"] and a["residual"] == b["residual"]
    assert np.array_equal(hp.get_min_dist().view(np.uint32), a["min_dist"].view(np.uint32))


@pytest.mark.parametrize("track", ["1", "0"])
def test_lloyd_after_a_draw_with_duplicates_at_k_260(hp, track, monkeypatch, capfd):
    """clustered-260: rounds in which a die is skipped as a duplicate, through the thin products, which keep every document's nearest
    seed (k > 224).  The first assignment of Lloyd in span(U) is taken from the rounds with tracking on and computed with it off; both are
    certified against fp64.  A round that adds NO seed cannot precede a hand-over: it happens only at a zero total, after which no run
    ends (kmpp_certificate's docstring; test_exhausted_corpus_is_refused_and_the_context_stays_usable holds that run)."""
    case = ALL_CASES["clustered-260"]
    e = expected(case)
    assert e["duplicates"] >= 3 and case["k"] > 224
    g = _run(hp, case, {"ISLE_KMPP_SPARSE": "1", "ISLE_KMPP_TRACK": track}, monkeypatch, capfd)
    _equal(case, g, e, "clustered-260 track=%s" % track)
    capfd.readouterr()
    lp = hp.run_lloyds_on_projected_space(case["k"], g["C_lowd"], max_reps=1)
    err = capfd.readouterr().err
    P = exact_P(case)
    certify_assignment(P, np.einsum("ij,ij->i", P, P), g["C_lowd"], lp["assign"], what="clustered-260 track=%s:" % track, near_ties=True)
    assert ("first assignment taken from the k-means++ rounds" in err) == (track == "1"), err[-2000:]
    assert ("first assignment computed" in err) == (track == "0"), err[-2000:]


@pytest.mark.parametrize("k", sorted(kc.GENERIC_SEEDS))
def test_generic_corpus_passes_the_weak_certificate(hp, k):
    g = kc.generic_inputs(k)
    hp.upload_csc(g["V"], g["vals"], g["rows"], g["offs"])
    hp.set_U(g["U"])
    r = hp.kmeans_init_on_projected_space(k, rng_seed=g["rng_seed"])
    a = kc.admissible(g["P64"], k, g["rng_seed"], r["seeds"], r["rounds"])
    print("generic k = %d: %d of %d dice ambiguous, widest set %d, residual %.9g against %.9g, allowance %.3g"
          % (k, a["ambiguous"], a["dice"], a["widest"], r["residual"], a["total"] - a["last"], a["allowance"]))
    REPORT["generic"][k] = {x: a[x] for x in ("ambiguous", "with_chosen", "dice", "share", "widest")}
    assert a["share"] <= kc.AMBIGUOUS_CAP and a["with_chosen"] / a["dice"] <= kc.AMBIGUOUS_CAP, a
    # the summed allowance of the distances, and the rounding of the result to float32
    assert abs(r["residual"] - (a["total"] - a["last"])) <= a["allowance"] + 2.0 ** -24 * a["total"]
    assert np.array_equal(r["C_lowd"].view(np.uint32), hp.get_projection(k)[r["seeds"].astype(np.int64)].view(np.uint32))
