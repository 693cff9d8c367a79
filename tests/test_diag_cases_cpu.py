"""The case table of tests/diag_cases.py without a GPU: every case reaches the edge it was built for (counted from its inputs alone), every
deliberately wrong rule fails at the case named for it, and where the repository holds a second statement of a rule the two agree bit for
bit on the table."""
import math
from fractions import Fraction

import numpy as np
import pytest

import diag_cases as dc
from diag_cases import COH, CS, F, WAVE, build
from isle_amd.hot_path import top_words
from test_corpus_stats_cpu import literal

COH_CASES = dc.coherence_cases()
HCAP = COH["HCAP"]


def test_constants_are_the_ones_the_cases_aim_at():
    assert dict(COH=dc.COH, CS=dc.CS, AM=dc.AM) == dc.EXPECTED_CONSTANTS
    assert dc.coh_tile(2000) == (163328 - (2 * 63 + 16 * 256) * 4) // 4 == 36610
    assert dc.coh_tile(131072) == 36736 - 8192 and dc.coh_tile(131073) == 36736
    assert dc.AW == 4


# ---- coherence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(COH_CASES) if n.startswith(("hits", "bitmap"))])
def test_coherence_hit_cases_reach_the_list_edges(name):
    case = build(COH_CASES[name])
    V = case["V"]
    hits = dc.coh_hits(case)
    assert [len(ids) for _, ids in hits] == case["want_hits"]
    counts = sorted(set(case["want_hits"]))
    assert counts == list(dc.COH_HITS) and {HCAP - 1, HCAP, HCAP + 1, WAVE - 1, WAVE, WAVE + 1} <= set(counts)
    assert (case["tw"] == V - 1).sum() == 1                                   # the last word of the vocabulary is a top word ...
    assert sum(1 for d in range(len(hits)) if case["rows"][case["offs"][d + 1] - 1] == V - 1 and len(hits[d][1])) >= 9   # ... and occurs
    for pos, ids in hits:                                                      # the list is sorted: the binary search's premise
        assert np.all(np.diff(ids) > 0)
    # compaction across batches: documents whose hits per 64-entry batch differ, with misses in between
    spread = [np.bincount(pos // WAVE) for pos, _ in hits if len(pos) > WAVE]
    assert spread and all(len(s) >= 2 and 0 < s.min() < WAVE for s in spread)
    if name == "hits-131072":
        assert not dc.coh_uses_table(V) and (V + 31) // 32 == 4096
    if name == "hits-131073":
        assert dc.coh_uses_table(V) and max(len(ids) for _, ids in hits) > HCAP   # the slow path in table form
    if name.startswith("bitmap-tail"):
        assert V % 32 in (1, 31) and (V - 1) // 32 == (V + 31) // 32 - 1


TILE_REACH = {"tile-exact": (1, "N == tile"), "tile-plus-1": (2, "N == tile + 1"), "cut-at-nU": (2, "nU == tile"), "words-only": (19, "nU > tile")}


@pytest.mark.parametrize("name", sorted(dc.COH_TILE_SPECS))
def test_coherence_tile_cases_reach_their_cuts(name):
    case = build(COH_CASES[name])
    plan = dc.coh_plan(case["tw"])
    tile = dc.coh_tile(case["V"])
    nU, N = plan["nU"], plan["N"]
    passes = -(-N // tile)
    assert passes == TILE_REACH[name][0]
    if name == "tile-exact":
        assert N == tile
    elif name == "tile-plus-1":
        assert N == tile + 1 and nU < tile                                     # the second pass holds one pair counter
    elif name == "cut-at-nU":
        assert nU == tile and plan["nP"] > 0                                   # c0 == nU: pass 0 words only, pass 1 pairs only
    else:
        assert nU > tile and nU % tile != 0                                    # pass 0: word counters only; pass 1: mixed
        _, df, co = dc.coh_reference(case)
        cuts = [j * tile for j in range(1, passes) if j * tile > nU]
        off = plan["part_off"]
        inside = 0
        for c in cuts:                                                         # a tile end strictly inside one word's partner range
            a = int(np.searchsorted(off, c - nU, "right")) - 1
            inside += off[a] < c - nU < off[a + 1]
        assert inside >= 10
        assert max(len(ids) for _, ids in dc.coh_hits(case)) > HCAP            # the slow path under the cb / ce clamps as well
        assert (co > 0).mean() > 0.05
    _, df, co = dc.coh_reference(case)
    assert (df > 0).mean() > 0.9 and (co > 0).any()


def test_coherence_wrong_rules_fail():
    case = build(COH_CASES["hits-2000"])
    coh, df, co = dc.coh_reference(case)
    for rule in ("within-batch", "drop-beyond-hcap"):
        _, df2, co2 = dc.coh_reference(case, rule)
        assert np.array_equal(df, df2) and not np.array_equal(co, co2), rule
    # drop-beyond-hcap is wrong only from the first slow-path document on: without the documents of more than HCAP hits it is right
    keep = [d for d, h in enumerate(case["want_hits"]) if h <= HCAP]
    docs = [case["rows"][case["offs"][d]:case["offs"][d + 1]] for d in keep]
    small = dc.csc_of_sets(case["V"], docs)
    small["tw"] = case["tw"]
    assert np.array_equal(dc.coh_reference(small)[2], dc.coh_reference(small, "drop-beyond-hcap")[2])
    assert not np.array_equal(dc.coh_reference(small)[2], dc.coh_reference(small, "within-batch")[2])


@pytest.mark.parametrize("name", ["hits-2000", "hits-131073", "tile-plus-1"])
def test_coherence_agrees_with_the_sparse_product_of_the_feature_test(name):
    from test_gpu_coherence import brute
    case = build(COH_CASES[name])
    a = dc.coh_reference(case)
    b = brute(case["V"], case["rows"], case["offs"], case["tw"])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    nan = np.isnan(a[0])
    assert np.array_equal(nan, np.isnan(b[0])) and a[0][~nan].tobytes() == b[0][~nan].tobytes()


# ---- log-combinatorial -----------------------------------------------------------------------------------------------------------
def test_log_combinatorial_cases_reach_the_table_edges():
    nlf = {name: int(dc.doc_words(dc.lc_case(name)).max()) + 1 for name in ("lds-last", "hbm-first")}
    assert nlf["lds-last"] == CS["LF_LDS_MAX"] and nlf["hbm-first"] == CS["LF_LDS_MAX"] + 1
    for name in nlf:
        case = dc.lc_case(name)
        N = dc.doc_words(case)
        assert np.diff(case["offs"])[N == N.max()].tolist().count(1) == 1      # one entry of that count ...
        assert (np.diff(case["offs"])[N == N.max()] > 1).any()                 # ... and documents of several entries that index T[N_d] at the end
    assert np.diff(dc.lc_case("wave-sum")["offs"]).tolist()[:5] == [0, 1, 63, 64, 65]
    assert dc.doc_words(dc.lc_case("refuse")).max() == 2 ** 31 > np.iinfo(np.int32).max


def test_log_combinatorial_wrong_rule_and_agreement():
    from test_gpu_corpus_stats import log_comb_checker as walker
    for name in dc.log_comb_cases():
        case = dc.lc_case(name)
        plain = dc.log_comb_reference(case)
        assert plain.view(np.uint32).tolist() == walker(case["cnt"], case["offs"]).view(np.uint32).tolist(), name
        clamped = dc.log_comb_reference(case, "clamp-index")
        assert (plain.tobytes() != clamped.tobytes()) == (name == "hbm-first"), name   # the clamp fails exactly at the first HBM table
    plain = dc.log_comb_reference(dc.lc_case("lds-last"))
    assert plain[0] == 0 and plain[1] > 0


# ---- top five --------------------------------------------------------------------------------------------------------------------
def test_top_five_lane_cases_reach_their_lanes():
    case = dc.t5_lanes_case()
    lens = np.diff(case["offs"])
    assert lens[:7].tolist() == list(dc.T5_LENGTHS) and (lens >= 5).sum() == len(lens) - 1
    nv = dc.normalised(case).view(np.uint32)
    for what, (d, pos) in case["plant"].items():
        v = nv[case["offs"][d]:case["offs"][d + 1]]
        top = np.argsort(-v.astype(np.int64), kind="stable")[:len(pos)]
        assert sorted(top.tolist()) == sorted(pos), what                       # the planted entries are the largest
        lanes = sorted(p % WAVE for p in pos)
        if what == "one-lane":
            assert lanes == [dc.T5_ONE_LANE] * 5 and len(set(v[pos].tolist())) == 5
        elif what == "five-equal":
            assert len(set(lanes)) == 5 and len(set(v[pos].tolist())) == 1
        else:
            assert lanes == [10] * 3 + [11] * 3 and len(set(v[pos].tolist())) == 1


def test_top_five_run_cases_reach_the_block_cut():
    ct = CS["CT"]
    for n, (at, length) in dc.T5_RUN_SPECS.items():
        ref = dc.top5_reference(dc.t5_runs_case(n))
        runs = ref["runs"]
        assert len(ref["tuples"]) == n == sum(runs) and runs[-1] == 3          # a run ends at the last sorted position
        starts = np.concatenate([[0], np.cumsum(runs)[:-1]])
        if at is not None:
            i = starts.tolist().index(at)
            assert runs[i] == length and at < ct < at + length - 1             # equal tuples on both sides of the 256-thread cut
    assert {n - ct for n in dc.T5_RUN_SPECS if n < 300} == {-1, 0, 1}


def _counts(ref):
    return {m: literal(ref["run_ids"], m) for m in dc.MS}


def test_top_five_wrong_rules_and_agreement():
    from test_gpu_corpus_stats import top5_checker as checker
    lanes = dc.t5_lanes_case()
    plain = dc.top5_reference(lanes)
    assert plain["tuples"].tobytes() == dc.top5_reference(lanes, "lanes")["tuples"].tobytes()      # the kernel's scheme is the plain rule
    assert plain["tuples"].tobytes() != dc.top5_reference(lanes, "lane-top-4")["tuples"].tobytes()
    assert plain["tuples"].tobytes() != dc.top5_reference(lanes, "pop-all-holders")["tuples"].tobytes()
    # which planted document each wrong rule gets wrong
    nv = dc.normalised(lanes).view(np.uint32)
    doc = lambda what: nv[lanes["offs"][lanes["plant"][what][0]]:lanes["offs"][lanes["plant"][what][0] + 1]]
    want = lambda v: np.sort(v)[::-1][:5].tolist()
    assert dc.lane_top5(doc("one-lane"), keep=4) != want(doc("one-lane")) == dc.lane_top5(doc("one-lane"))
    assert dc.lane_top5(doc("five-equal"), pop_all=True) != want(doc("five-equal")) == dc.lane_top5(doc("five-equal"))
    assert dc.lane_top5(doc("six-in-two"), pop_all=True) != want(doc("six-in-two")) == dc.lane_top5(doc("six-in-two"))
    for name, spec in dc.top_five_cases().items():
        case = build(spec)
        ref = dc.top5_reference(case)
        T, counts = checker(case["cnt"], case["offs"])
        assert T.view(np.uint32).tolist() == ref["tuples"].view(np.uint32).tolist(), name
        assert counts == _counts(ref), name
        if name != "lanes":
            assert dc.top5_reference(case, "last-run-1")["runs"] != ref["runs"], name


# ---- the average model -------------------------------------------------------------------------------------------------------------
def test_average_model_cases_reach_their_edges():
    hi = dc.avg_case("hi-half")
    ref = dc.avg_reference(hi)
    ratio = float(hi["nv"].max()) / float(hi["nv"].min())
    assert 2 ** 9 <= ratio <= 2 ** 12 and ref["exact"] and max(ref["N"]) < 2 ** 53
    assert ref["n_hi"] >= 100 and ref["n_hi"] == sum(1 for x in hi["nv"] if float(x) * 2.0 ** ref["e"] >= 2 ** 32)   # the hi half is in use
    assert ref["sizes"].tolist()[1] == 1 and ref["sizes"][3] == 0 and (hi["cl"] == -1).sum() == 2
    lens = np.diff(hi["offs"])
    assert {63, 64, 65} <= set(lens[hi["cl"] == 2].tolist())
    big = dc.avg_case("beyond-2^53")
    rb = dc.avg_reference(big)
    assert not rb["exact"] and rb["N"][0] >= 2 ** 53 and rb["N"][0] & 1 and rb["S"][0][0] >= 2 ** 53 and rb["S"][0][0] & 1
    assert float(rb["N"][0]) != rb["N"][0] and len(big["offs"]) - 1 <= 400
    assert dc.avg_case("one-topic")["topics"] == 1 and dc.avg_case("one-word")["V"] == 1
    assert dc.avg_reference(dc.avg_case("one-word"))["sizes"].tolist() == [6, 0]


@pytest.mark.parametrize("name", dc.AVG_CASES)
def test_average_model_statements_are_consistent(name):
    """The bit-exact expectation lies inside the derived bound, and certify_avg accepts it."""
    case = dc.avg_case(name)
    ref = dc.avg_reference(case)
    if ref["exact"]:
        assert dc.certify_avg(ref["model"], case, ref)["ratio"] <= 1.0
    else:
        near = np.full((case["V"], case["topics"]), np.nan, F)
        for t, n in enumerate(ref["N"]):
            if n:
                near[:, t] = [dc.round_f32(Fraction(ref["S"][w][t], n)) for w in range(case["V"])]
        assert dc.certify_avg(near, case, ref) == dict(mode="bound", ratio=pytest.approx(0.5, abs=0.5))


def test_average_model_wrong_rules_fail():
    hi = dc.avg_case("hi-half")
    ref = dc.avg_reference(hi)
    dropped = dc.avg_reference(hi, "drop-hi")
    with pytest.raises(AssertionError):
        dc.certify_avg(dropped["model"], hi, ref)
    with pytest.raises(AssertionError):
        dc.certify_avg(dc.avg_fp32_in_document_order(hi), hi, ref)
    big = dc.avg_case("beyond-2^53")
    with pytest.raises(AssertionError):
        dc.certify_avg(dc.avg_reference(big, "drop-hi")["model"], big, dc.avg_reference(big))
    one_ulp = ref["model"].copy()                                               # one ulp off in one entry: today's 2^-22 bound lets it pass
    w = int(np.argmax(one_ulp[:, 0]))
    one_ulp[w, 0] = np.nextafter(one_ulp[w, 0], F(2))
    assert abs(float(one_ulp[w, 0]) / float(ref["model"][w, 0]) - 1) < 2.0 ** -22
    with pytest.raises(AssertionError):
        dc.certify_avg(one_ulp, hi, ref)


def test_normalised_values_agree_with_the_feature_tests_formula():
    """setup_post of test_gpu_avg_model.py: avg * (cnt / doc_sum) with float32 operands."""
    case = dc.avg_case("hi-half")
    lens = np.diff(case["offs"])
    sums = np.add.reduceat(case["cnt"].astype(np.float64), case["offs"][:-1])
    nv = F(case["B"]["avg"]) * (case["cnt"] / np.repeat(sums.astype(F), lens))
    assert nv.dtype == np.float32 and nv.tobytes() == case["nv"].tobytes()


# ---- top words -------------------------------------------------------------------------------------------------------------------
def test_top_words_sizes_reach_the_empty_ranges():
    for V in dc.TW_SIZES:
        per = -(-V // dc.AW)
        empty = [wv for wv in range(dc.AW) if wv * per >= V]
        assert (len(empty) > 0) == (V in (1, 2, 3, 5)) or V == 4
        assert dc.tw_size_case(V)["ns"] == sorted({1, min(V, 32)})
    assert [wv for wv in range(4) if wv * 2 >= 5] == [3] and [wv for wv in range(4) if wv >= 1] == [1, 2, 3]


def test_top_words_tie_cases_reach_their_ranges():
    M = dc.tw_ties_case()["M"]
    K, r, ranges = dc.tie_ranges(M[:, 0], 8)
    assert (K, r, ranges) == (0.5, 3, [0, 0, 1, 1])                             # the three taken: two of wave 0's range, one of wave 1's
    K, r, ranges = dc.tie_ranges(M[:, 1], 5)
    assert (K, r) == (0.5, 3) and ranges == [0] * 40                           # more than 32 ties in one range, three needed
    K, r, ranges = dc.tie_ranges(M[:, 2], 32)
    assert r == 32 and len(ranges) == 1024
    K, r, ranges = dc.tie_ranges(M[:, 3], 3)
    assert (K, r, ranges) == (0.5, 2, [2, 3, 3])
    keys = dc.tw_keys_case()["M"]
    assert np.isfinite(keys[:, 0]).sum() == 4 < 32
    assert (np.signbit(keys[:, 1]) & (keys[:, 1] == 0)).sum() == 30 and (~np.signbit(keys[:, 1]) & (keys[:, 1] == 0)).sum() == 30
    assert ((keys[:, 2] != 0) & (np.abs(keys[:, 2]) < 2.0 ** -126)).sum() == 4
    assert (keys[:, 3].view(np.uint32) == 0xffc00000).sum() == 1 and np.isinf(keys[:, 3]).sum() == 4


def test_top_words_wrong_rule_fails_and_ties_follow_id_order():
    M = dc.tw_ties_case()["M"]
    assert top_words(M, 8)[0].tolist()[5:] == [254, 255, 256]
    assert top_words(M, 5)[1].tolist() == [500, 700, 0, 2, 4]
    assert top_words(M, 32)[2].tolist() == list(range(32))
    for n in (5, 8, 32):
        assert not np.array_equal(top_words(M, n), dc.top_words_highest_id(M, n))
    keys = dc.tw_keys_case()["M"]
    assert top_words(keys, 32)[0].tolist()[:4] == [69, 3, 40, 41] and top_words(keys, 32)[0].tolist()[4:8] == [0, 1, 2, 4]


@pytest.mark.parametrize("ratio", dc.EDGE_RATIOS)
def test_edge_case_ties_only_after_the_fma(ratio):
    M = dc.edge_model(ratio)
    lo, hi = dc.EDGE_TIE_WORDS
    assert M[lo, 1] != M[hi, 1] and (ratio == 1.0 or M[lo, 0] != M[hi, 0])
    E = dc.edge_columns(M, dc.EDGE_PAIRS, ratio)
    assert E[lo, 0].view(np.uint32) == E[hi, 0].view(np.uint32) and E[lo, 0] == E[:, 0].max() and (E[:, 0] == E[lo, 0]).sum() == 2
    assert top_words(E, 1)[0].tolist() == [lo] and top_words(E, 10)[0].tolist()[:2] == [lo, hi]
    assert dc.top_words_highest_id(E, 1)[0].tolist() == [hi]
    # the certificate of the edge topics holds for these columns: a second statement of the same entries
    dc.sc.certify_edge(E, M, np.array(dc.EDGE_PAIRS), ratio)


def test_round_f32_is_round_to_nearest_even():
    rng = np.random.default_rng(5)
    for x in rng.standard_normal(200) * 10.0 ** rng.integers(-44, 30, 200):
        assert dc.round_f32(Fraction(float(x))) == F(x) or (math.isinf(float(F(x))))
    assert dc.round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == F(1) and dc.round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == F(1) + F(2.0 ** -22)


# ---- diversity -------------------------------------------------------------------------------------------------------------------
def test_diversity_cases_and_bound():
    kps = {name: dc.diversity_reference(dc.div_case(name)["M"])["kp"] for name in dc.DIV_CASES}
    assert kps == {"no-finite-topic": 0, "one-finite-topic": 1, "one-inf": 3, "block-255": 5, "block-256": 5, "block-257": 5}
    assert [dc.div_case("block-%d" % V)["V"] - dc.AM["AT"] for V in (255, 256, 257)] == [-1, 0, 1]
    for name in dc.DIV_CASES:
        M = dc.div_case(name)["M"]
        ref = dc.diversity_reference(M)
        text = dc.dense_text(M)
        assert text.count(b"\n") == M.shape[1] and len(text.split()) == M.size
        # an fp64 evaluation in the kernels' order lies inside the bound; one that is 1e-12 off does not
        fin = ref["finite"]
        X = M.astype(np.float64)
        if ref["kp"]:
            abar = np.zeros(M.shape[0])
            for t in np.flatnonzero(fin):
                abar = abar + X[:, t]
            abar = abar / ref["kp"]
            dist = np.where(fin, ((X - abar[:, None]) ** 2).sum(axis=0), np.nan)
            avg = 0.0
            for t in np.flatnonzero(fin):
                avg += dist[t]
            got = dict(dist=dist, avg=avg / ref["kp"])
        else:
            got = dict(dist=np.full(M.shape[1], np.nan), avg=math.nan)
        assert dc.certify_diversity(got, ref) <= 1.0
        if ref["kp"] > 1:
            off = dict(dist=got["dist"] * (1 + 1e-12), avg=got["avg"])
            with pytest.raises(AssertionError):
                dc.certify_diversity(off, ref)
            assert (ref["bound"][fin] < 1e-12 * ref["dist"][fin]).all() and (ref["dist"][fin] > 0).all()
