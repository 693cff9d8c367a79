"""The plain reference of tests/stages_certificate.py against the project's C++ restatements (tools/synth_corpus.cpp through
tools.synth.Corpus, oracle/isle_post_oracle.cpp through oracle.post_*), on the inputs test_gpu_stages_certified.py runs.  No GPU.

Agreement: both sides were written from the reference for their own reasons and must agree bit for bit.  Reach: every case reaches the
edge it was built for, asserted with counts.  Discrimination: every case fails under the wrong rule it was built for.  The model
certificate accepts fp32 accumulation in any order and rejects a model that lacks one document."""
import numpy as np
import pytest

import stages_certificate as sc
from stages_certificate import F, build, post_reference, ref_threshold

TH_CASES = sc.threshold_cases()


def _thr(case, rule="device"):
    return ref_threshold(case["V"], case["cnt"], case["rows"], case["offs"], case["k"], doc_base=case.get("doc_offset", 0), rule=rule)


def _corpus(case):
    from tools.synth import Corpus
    return Corpus.from_csc(case["V"], len(case["offs"]) - 1, case["cnt"], case["rows"], case["offs"])


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- agreement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TH_CASES))
def test_threshold_agrees_with_cpu_port(name):
    case = build(TH_CASES[name])
    want = _thr(case)
    got = _corpus(case).threshold(case["k"])
    got["original_cols"] = got["original_cols"] + np.uint64(case.get("doc_offset", 0))  # the port numbers documents from 0
    sc.assert_same_B(got, want, name)


def _post_cases():
    out = [("catch-%d-rho%g" % (k, rho), (sc.p_catch_case, k), dict(rho=rho)) for k in sc.CATCH_K for rho in sc.CATCH_RHOS]
    out.append(("arms", (sc.p_arms_case,), {}))
    out += [("dts-%d" % k, (sc.p_dts_case, k), {}) for k in sc.DTS_K]
    out += [("select-r%d" % r, (sc.p_select_case,), dict(r=r, rank=r)) for r in sc.select_ranks()]
    return out


POST_CASES = _post_cases()


@pytest.mark.parametrize("name,spec,kw", POST_CASES, ids=[c[0] for c in POST_CASES])
def test_post_agrees_with_oracle(name, spec, kw):
    from oracle import oracle as O
    case = build(spec)
    R = post_reference(case, **kw)
    k, V = case["topics"], case["V"]
    r, rho = kw.get("r", case["r"]), kw.get("rho", 1.1)
    rank = kw.get("rank", case.get("rank", 1))
    nv = O.post_normalize(case["offs"], case["cnt"], case["B"]["avg"])
    assert _same_bits(nv, case["nv"])
    thr = O.post_catch_thresholds(V, case["offs"], case["rows"], nv, case["cl"], k, r)
    assert _same_bits(thr, R["thr"])
    ct = O.post_find_catchwords(thr, rho)
    assert np.array_equal(ct, R["catch_topic"])
    ref = O.post_topic_model(V, case["offs"], case["rows"], nv, case["cl"], ct, k, rank)
    dts = R["dts"]
    assert np.array_equal(ref["dts_doc"], np.repeat(np.arange(len(case["offs"]) - 1, dtype=np.uint64), np.diff(dts["dts_off"])))
    assert np.array_equal(ref["dts_topic"], dts["dts_topic"]) and _same_bits(ref["dts_val"], dts["dts_val"])
    assert _same_bits(ref["model_threshold"], R["mthr"])
    assert np.array_equal(ref["top1"], dts["top1"]) and np.array_equal(ref["top2"], dts["top2"])
    sc.certify_model(ref["model"], R["model64"], R["m"], V)  # the oracle accumulates in fp32 in document order


# ---- reach and discrimination: thresholding ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("avg", sc.ROUND_AVGS)
def test_round_case_reaches_and_discriminates(avg):
    case = sc.t_round_case(avg)
    B = {r: _thr(case, r) for r in sc.RULES}
    assert B["device"]["avg"] == avg and (B["device"]["count_gr"], B["device"]["count_eq"]) == (60, 6)
    ties = sum(p["tie"] for p in case["probes"])
    order = sum(p["q"]["device"] != p["q"]["assoc"] or p["q"]["device"] != p["q"]["fp64"] for p in case["probes"])
    assert ties >= 1
    assert order >= (2 if avg in (11, 19, 23) else 0)
    for p in case["probes"]:
        i = case["offs"][p["doc"]]  # the probe word has the smallest id of its document
        assert case["rows"][i] == p["word"]
        for r in sc.RULES:
            assert B[r]["zetas"][p["word"]] == p["Z"], "the probe word's zeta is not pinned"
            assert B[r]["q"][i] == p["q"][r] and bool(B[r]["keep"][i]) == (p["q"][r] >= p["Z"])
    for r in ("assoc", "fp64", "banker"):
        flips = sum(p["q"][r] != p["q"]["device"] for p in case["probes"])
        changed = not np.array_equal(B[r]["keep"], B["device"]["keep"])
        assert changed == (flips > 0)
        if r == "banker" and avg in (9, 11, 13, 19, 23):
            assert changed
        if r != "banker" and avg in (11, 19, 23):
            assert changed


def test_round_cases_together_fail_every_wrong_rule():
    for r in ("assoc", "fp64", "banker"):
        n = 0
        for avg in sc.ROUND_AVGS:
            case = sc.t_round_case(avg)
            n += not np.array_equal(_thr(case, r)["rows"], _thr(case)["rows"])
        assert n >= 3, r


def test_known_triples():
    """(11, 13, 22): the device order gives 6, (avg * cnt) / sum and fp64 give 7.  (9, 1, 2) is 4.5 exactly: 5, where rint gives 4."""
    q = {r: int(sc.quantise(11, np.array([13], F), np.array([22]), r)[0]) for r in sc.RULES}
    assert q == dict(device=6, assoc=7, fp64=7, banker=6)
    q = {r: int(sc.quantise(9, np.array([1], F), np.array([2]), r)[0]) for r in sc.RULES}
    assert q == dict(device=5, assoc=5, fp64=5, banker=4)


def test_zeta_case_takes_every_arm():
    case = sc.t_zeta_case()
    B = _thr(case)
    assert (B["avg"], B["nz_docs"], B["count_gr"], B["count_eq"]) == (12.0, 480, 30, 3)
    tr = B["trace"]
    for w, (arm, zeta) in sc.ZETA_EXPECT.items():
        assert tr[w]["arm"] == arm and B["zetas"][w] == zeta, (w, tr[w], B["zetas"][w])
    assert tr[1]["size"] == B["count_gr"] - 1 and tr[2]["size"] == B["count_gr"]
    assert tr[4]["eq"] == B["count_eq"] - 1 and not tr[4]["descents"]
    assert tr[5]["descents"] == [(5, 4, B["count_eq"])]                      # #eq == count_eq descends
    assert tr[6]["descents"][0][0] - tr[6]["descents"][0][1] - 1 >= 2        # over at least two empty bins
    assert tr[7]["descents"] and tr[7]["arm"] == "end" and tr[8]["arm"] == "one" and tr[8]["eq"] >= B["count_eq"]
    assert tr[9]["first"] == int(B["avg"])                                    # the largest bin in use: one-word documents
    lens = np.diff(case["offs"])
    one_word = np.flatnonzero(lens == 1)
    assert np.all(B["q"][case["offs"][one_word]] == int(B["avg"])) and (case["rows"][case["offs"][one_word]] == 9).sum() == 31


def test_lanes_case_places_survivors_on_lane_boundaries():
    case = sc.t_lanes_case()
    B = _thr(case)
    assert (B["avg"], B["nz_docs"], B["count_gr"], B["count_eq"]) == (2000.0, 900, 15, 2)
    seen = set()
    for l in case["lanes"]:
        s, e = case["offs"][l["doc"]], case["offs"][l["doc"] + 1]
        assert e - s == l["n"]
        if l["n"] >= 63:
            assert np.array_equal(B["keep"][s:e], l["mask"])
            seen.add((l["n"], l["pattern"]))
        elif l["n"] == 1:
            assert B["keep"][s]
    assert seen == {(n, p) for n in sc.LANE_SIZES if n >= 63 for p in sc.LANE_PATTERNS}
    lens = np.diff(case["offs"])
    assert (lens == 0).sum() >= 45 and ((lens > 0) & (B["kept"] == 0)).sum() >= 7   # empty and fully dropped documents in between


def test_sampled_lanes_keep_lane_documents():
    """T-sampled reaches lane documents: under the CPU port's key draw the chosen seed keeps documents of 128 and 129 entries."""
    case = sc.t_lanes_case()
    B = _corpus(case).threshold(case["k"], sample_rate=sc.SAMPLED_RATE, sample_seed=sc.SAMPLED_SEED)
    kept = set(int(d) for d in B["original_cols"])
    assert {(l["n"], l["pattern"]) for l in case["lanes"] if l["n"] >= 63 and l["doc"] in kept} == sc.SAMPLED_LANES_KEPT
    assert 0 < B["D"] < _thr(case)["D"]


@pytest.mark.parametrize("D", sc.SCAN_D)
def test_scan_case_shape(D):
    case = sc.t_scan_case(D)
    B = _thr(case)
    lens = np.diff(case["offs"])
    assert len(lens) == D and lens.max() <= 3 and B["avg"] == 40.0
    third = np.arange(D) % 3 == 2
    assert np.all(B["kept"][third] == 0) and (lens[third] == 0).sum() > D // 7 and (lens[third] == 2).sum() > D // 7
    assert 0 < B["D"] < D and B["original_cols"][0] >= case["doc_offset"]


def test_stride_case_needs_two_trips():
    case = sc.t_stride_case()
    D, nnz = len(case["offs"]) - 1, len(case["rows"])
    assert D > sc.MI355X_CUS * 32 * 4 and nnz > sc.MI355X_CUS * 8 * 256
    B = _thr(case)
    assert 0 < B["nnz"] < nnz and len(np.unique(B["zetas"])) > 5


# ---- reach and discrimination: downstream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.CATCH_K)
def test_catch_case_rows(k):
    case = sc.p_catch_case(k)
    assert case["B"]["D"] == k == len(case["offs"]) - 1 and case["B"]["avg"] == sc.CATCH_SUM
    names = case["names"]
    res = {rho: post_reference(case, rho=rho) for rho in sc.CATCH_RHOS}
    thr = res[1.1]["thr"]
    assert res[1.1]["arms"]["S == r, n == S"] > 0 and set(res[1.1]["arms"]) <= {"S == r, n == S", "n == r", "empty cluster"}
    for w, (name, spec) in enumerate(zip(names, case["spec"])):
        if not name.startswith("ulp"):
            want = np.zeros(k, F)
            for t, c in spec.items():
                want[t] = c
            assert np.array_equal(thr[w], want), name   # the threshold matrix is the designed one
    for rho in sc.CATCH_RHOS:
        ct = dict(zip(names, res[rho]["catch_topic"]))
        loose = dict(zip(names, sc.ref_find_catchwords(thr, rho, strict=False)))
        if k == 1:
            assert all(v == -1 for v in ct.values())
            continue
        for name in names:
            if name.startswith("max@"):
                assert ct[name] == int(name[4:])
            if name.startswith("tie") or name == "zero":
                assert ct[name] == -1
        assert ct["single@last"] == k - 1 and ct["single@0"] == 0
        assert ct["eq1.5"] == (k - 1 if rho < 1.5 else -1) and ct["eq2.0"] == (0 if rho < 2.0 else -1)
        if rho in (1.5, 2.0):   # m1 == rho * m2 exactly in double: the strict rule refuses, >= would accept
            w = names.index("eq%.1f" % rho)
            m = np.sort(thr[w].astype(np.float64))
            assert m[-1] == rho * m[-2] and loose["eq%.1f" % rho] >= 0 and ct["eq%.1f" % rho] == -1
            assert not np.array_equal(sc.ref_find_catchwords(thr, rho, strict=False), res[rho]["catch_topic"])
        if k >= 63:
            for rr, t in ((1.5, 4), (2.0, 7)):
                w = names.index("ulp%.1f" % rr)
                m = np.sort(thr[w])
                assert float(F(rr * float(m[-2]))) == rr * float(m[-2]) and m[-1] == np.nextafter(F(rr * float(m[-2])), F(np.inf))
                if rho <= rr:
                    assert ct["ulp%.1f" % rr] == t
    if k > 65:
        assert "tie(t,t+64)" in names and "max@64" in names and "max@63" in names


def test_arms_case_populates_every_arm():
    case = sc.p_arms_case()
    R = post_reference(case)
    for arm in ("n > r + 1", "n == r", "n == r + 1", "S == r, n == S", "S < r, n == S", "n < S <= r", "S > r >= n", "empty cluster"):
        assert R["arms"][arm] >= 1, arm
    assert (case["cl"] == -1).sum() == 3 and np.all(case["want_cluster"][case["cl"] == -1] == -1)
    assert np.isnan(R["model64"][:, 3]).all() and not np.isnan(np.delete(R["model64"], 3, axis=1)).any()
    # counting the dropped documents would change the thresholds
    cl2 = case["cl"].copy()
    cl2[cl2 == -1] = 0
    assert not np.array_equal(sc.ref_catch_thresholds(case["V"], case["rows"], case["offs"], case["nv"], cl2, 5, 3)[0], R["thr"])


def test_select_case_segments():
    case = sc.p_select_case()
    assert case["B"]["D"] == len(case["offs"]) - 1
    lens = {(s["n"], s["kind"]) for s in case["segs"]}
    assert lens == {(n, kd) for n in sc.SELECT_LENGTHS for kd in sc.SELECT_KINDS}
    for n in sc.SELECT_LENGTHS:
        assert {1, max(n // 2, 1), n - 1, n, n + 1} <= set(sc.select_ranks())
    nv, rows, cl = case["nv"], case["rows"].astype(np.int64), case["cl"]
    doc_of = np.repeat(np.arange(len(case["offs"]) - 1), np.diff(case["offs"]))
    for s in case["segs"]:
        v = np.sort(nv[(rows == s["word"]) & (cl[doc_of] == s["topic"])])[::-1]
        assert len(v) == s["n"]
        if s["kind"] == "equal":
            assert len(np.unique(v)) == 1
        elif s["kind"] == "run" and s["n"] >= 255:
            n = s["n"]
            assert v[0] == v[1] and v[n // 2 - 2] == v[n // 2 + 1] and v[n - 3] == v[n - 1] and len(np.unique(v)) > n // 2
        elif s["kind"] == "top16" and s["n"] >= 255:
            assert len(np.unique(v)) >= 100 and len(np.unique(v.view(np.uint32) >> 16)) == 1
    # the per-topic sums give segments of the same lengths: rank == tcnt and rank == tcnt + 1 are both reached
    R = post_reference(case, r=1, rank=1)
    tcnt = np.bincount(R["dts"]["dts_topic"].astype(np.int64), minlength=case["topics"])
    assert set(sc.SELECT_LENGTHS) <= set(tcnt)   # (the filler word is a catchword too: one longer segment)
    for n in sc.SELECT_LENGTHS:
        at, above = post_reference(case, r=1, rank=n)["mthr"], post_reference(case, r=1, rank=n + 1)["mthr"]
        assert np.all(at[tcnt == n] > 0) and np.all(above[tcnt == n] == 0)


@pytest.mark.parametrize("k", sc.DTS_K)
def test_dts_case_reach(k):
    case = sc.p_dts_case(k)
    R = post_reference(case)
    dts, notes = R["dts"], case["notes"]
    assert case["V"] <= 256 and case["B"]["avg"] == 70.0 and case["B"]["D"] == len(case["offs"]) - 1
    assert np.array_equal(R["catch_topic"], [sc.dts_catch_topic(w, k) for w in range(sc.DTS_V)])
    lens = np.diff(case["offs"])
    assert {64, 65, 129} <= set(lens)

    def sums(d):
        s = slice(dts["dts_off"][d], dts["dts_off"][d + 1])
        return dts["dts_topic"][s], dts["dts_val"][s]

    assert len(sums(notes["no catchword"])[0]) == 0
    d = notes["boundaries 0, 63, 64, 128"]
    ct_e = R["catch_topic"][case["rows"][case["offs"][d]:case["offs"][d + 1]]]
    assert lens[d] == 129 and np.all(ct_e[[0, 63, 64, 128]] >= 0)
    d = notes["one topic only"]
    assert len(sums(d)[0]) == 1 and dts["top1"][d] == -1 and dts["top2"][d] == -1
    d = notes["two equal sums"]
    t, v = sums(d)
    assert len(t) == 2 and v[0] == v[1] and (dts["top1"][d], dts["top2"][d]) == (t[0], t[1])
    d = notes["both routes"]
    assert R["contribs"].count((int(case["cl"][d]), d)) == 2
    eq = [(t, v) for t, v in zip(dts["dts_topic"], dts["dts_val"]) if R["mthr"][t] > 0 and v == R["mthr"][t]]
    assert eq, "no sum equals its topic's threshold"
    assert dts["dts_topic"].max() >= 64 and np.isnan(R["model64"][:, case["empty_topic"]]).all()
    # entry order matters: the reversed order gives other bits, in the document built for it
    rev = sc.ref_doc_topic_sums(case["rows"], case["offs"], case["nv"], R["catch_topic"], k, order="reversed")
    diff = np.flatnonzero(rev["dts_val"].view(np.uint32) != dts["dts_val"].view(np.uint32))
    d = notes["order-sensitive"]
    assert dts["dts_off"][d] in diff
    # >= in the membership rule changes the model beyond the certificate
    loose = sc.model_contributions(case["offs"], case["cl"], dts, R["mthr"], strict=False)
    assert len(loose) > len(R["contribs"])
    M, _ = sc.ref_model64(case["V"], case["rows"], case["offs"], case["nv"], loose, k)
    with pytest.raises(AssertionError):
        sc.certify_model(np.nan_to_num(M, nan=np.nan).astype(F), R["model64"], R["m"], case["V"])


# ---- the model certificate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(sc.p_arms_case,), (sc.p_dts_case, 65), (sc.p_dts_case, 130)], ids=["arms", "dts-65", "dts-130"])
def test_model_certificate_accepts_any_order_and_rejects_a_missing_document(spec):
    case = build(spec)
    R = post_reference(case)
    k, V = case["topics"], case["V"]
    worst = 0.0
    for seed in range(3):
        M = sc.emulate_model32(V, case["rows"], case["offs"], case["nv"], R["contribs"], k, np.random.default_rng(seed))
        worst = max(worst, sc.certify_model(M, R["model64"], R["m"], V)["max_ratio"])
    assert 0 < worst <= 1
    gone = R["contribs"][len(R["contribs"]) // 2][1]
    less = [c for c in R["contribs"] if c[1] != gone]
    M = sc.emulate_model32(V, case["rows"], case["offs"], case["nv"], less, k, np.random.default_rng(0))
    with pytest.raises(AssertionError):
        sc.certify_model(M, R["model64"], R["m"], V)


def test_edge_certificate():
    case = sc.p_arms_case()
    R = post_reference(case)
    M = sc.emulate_model32(case["V"], case["rows"], case["offs"], case["nv"], R["contribs"], 5, np.random.default_rng(0))
    pairs = sc.edge_pairs(5, 3)
    a, b = sc.edge_coefficients(0.7)
    E = np.stack([np.float32(a * M[:, p]) + np.float32(b * M[:, q]) for p, q in pairs], axis=1)  # three roundings: one more than the kernel
    E64 = np.stack([(float(a) * M[:, p].astype(np.float64) + float(b) * M[:, q].astype(np.float64)).astype(F) for p, q in pairs], axis=1)
    assert sc.certify_edge(E64, M, pairs)["max_ratio"] <= 0.5
    assert np.isnan(E64[:, -1]).all()
    with pytest.raises(AssertionError):
        sc.certify_edge((E64 * F(1 + 2.0 ** -21)).astype(F), M, pairs)
    with pytest.raises(AssertionError):
        sc.certify_edge(E64[:, ::-1].copy(), M, pairs)
    del E
