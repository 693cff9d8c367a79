"""tests/post_shard_cases.py without a device: the layouts put the cases where the sharded stage can go wrong (asserted from the reference
alone), and the certificate accepts per-rank arrays made from the references by the right rule (fp32 partial sums per shard, then summed;
the single-rank arrays cut at the bounds) and refuses arrays made by a wrong one: a threshold selected per shard instead of globally, a
minimum taken over one shard, sums rebased wrongly, a model with one shard left out."""
import numpy as np
import pytest

import post_shard_cases as ps
import rank_launch
import shard_cases as sc
import stages_certificate as stc

F = np.float32


def test_layout_bounds():
    for name in ps.CASE_NAMES:
        case = ps.case_of(name)
        D = ps.num_docs(case)
        for layout in ps.GENERAL_LAYOUTS + ("W1",):
            b = ps.bounds(layout, case)
            assert len(b) == ps.WORLD[layout] + 1 <= 5 and b[0] == 0 and b[-1] == D and np.all(np.diff(b) >= 0)
        assert list(ps.bounds("H", case)) == [0, -(-D // 2), D]
        assert list(ps.bounds("E3", case)) == [0, 1, D, D] and list(ps.bounds("E4", case)) == [0, 0, D // 3, D // 3, D]


def test_select_cuts_put_every_long_segment_on_two_ranks():
    """Every segment of 255, 256, 257 and 1000 values lies on two ranks with both parts non-empty in its S layout; for some r of
    select_ranks() the r-th largest value of a cut segment lies on the first part only, for another on the second part only; the values
    that share their top 16 bits are cut, a hundred and more on either side, and selecting within a part alone gives another value."""
    case = ps.case_of("select")
    assert sorted({s["n"] for s in case["segs"]} - {2}) == list(ps.SELECT_CUT_LENGTHS)
    cut = set()
    for layout in ps.SELECT_LAYOUTS:
        b = ps.bounds(layout, case)
        assert len(b) == 5 and np.all(np.diff(b) > 0)
        facts = ps.select_layout_facts(case, b)
        assert [(f["seg"]["n"], f["seg"]["kind"]) for f in facts] == [(int(layout[1:]), kind) for kind in stc.SELECT_KINDS]
        for f in facts:
            n, kind = f["seg"]["n"], f["seg"]["kind"]
            assert len(f["parts"]) == 2 and min(f["parts"]) >= 1 and sum(f["parts"]) == n
            cut.add((n, kind))
            assert f["per_part_differs"], (n, kind)  # no part alone answers every rank
            if kind == "run":
                assert f["first"] and f["second"] and set(f["first"]) != set(f["second"])
                assert {n - 1, n} <= set(f["second"]) and 1 in f["first"]
            if kind == "top16":
                assert min(f["shared16"]) >= 100 and sum(f["shared16"]) == n  # all of them share sign, exponent and seven mantissa bits
                v, _ = ps.segment_values(case, f["seg"])
                assert len(np.unique(v.view(np.uint32) >> 16)) == 1 and len(np.unique(v.view(np.uint32) & 0xffff)) >= 100
    assert cut == {(n, kind) for n in ps.SELECT_CUT_LENGTHS for kind in stc.SELECT_KINDS}
    # the runs with r == n - 1, n, n + 1 at every length are among those of the case
    assert {m for n in stc.SELECT_LENGTHS for m in (n - 1, n, n + 1) if m >= 1} <= {r for r, _ in ps.runs_of("select")}


def test_the_general_layouts_cut_clusters_too():
    """the plain layouts cut at least one segment of p_select_case, and the empty topic of p_arms_case / p_dts_case stays empty"""
    case = ps.case_of("select")
    for layout in ps.GENERAL_LAYOUTS:
        assert ps.select_layout_facts(case, ps.bounds(layout, case))
    for name in ("arms",) + tuple("dts%d" % k for k in stc.DTS_K):
        c = ps.case_of(name)
        r, rank = ps.runs_of(name)[0]
        assert np.isnan(stc.post_reference(c, r=r, rho=ps.RHO, rank=rank)["model64"]).all(axis=0).any()


RIGHT = [(name, layout) for name in ("arms", "dts65") for layout in ps.GENERAL_LAYOUTS] + [("select", "S257"), ("select", "H")]


@pytest.mark.parametrize("name,layout", RIGHT)
def test_right_arrays_are_accepted(name, layout):
    """fp32 partial sums per shard, then summed; everything else the single-rank arrays, replicated or cut at the bounds"""
    case = ps.case_of(name)
    bnd = ps.bounds(layout, case)
    for r, rank in ps.runs_of(name)[:3] + ps.runs_of(name)[-2:]:
        res = ps.certify_post(case, name, r, rank, bnd, ps.reference_ranks(case, name, r, rank, bnd))
        assert res["model_ratio"] <= 1.0


def _per_shard_thresholds(case, bnd, q, r):
    """The thresholds rank q finds when it selects among its own documents only (a wrong rule)."""
    d0, d1 = int(bnd[q]), int(bnd[q + 1])
    o0, o1 = int(case["offs"][d0]), int(case["offs"][d1])
    thr, _ = stc.ref_catch_thresholds(case["V"], case["rows"][o0:o1], case["offs"][d0:d1 + 1] - o0, case["nv"][o0:o1], case["cl"][d0:d1], case["topics"], r)
    return thr


def test_a_threshold_selected_per_shard_is_refused():
    case, r = ps.case_of("select"), 128
    bnd = ps.bounds("S257", case)
    wrong = _per_shard_thresholds(case, bnd, 1, r)
    assert wrong.tobytes() != stc.post_reference(case, r=r, rho=ps.RHO, rank=r)["thr"].tobytes()
    with pytest.raises(AssertionError, match="thresholds differ"):
        ps.certify_post(case, "select", r, r, bnd, ps.reference_ranks(case, "select", r, r, bnd, thr=wrong))


def test_a_minimum_over_one_shard_is_refused():
    """p_arms_case: word 3 in cluster 1 has n == S == r, its threshold is the minimum of the documents 6, 7, 8; the shard [7, D) alone
    finds another"""
    case = ps.case_of("arms")
    r, rank = ps.runs_of("arms")[0]
    R = stc.post_reference(case, r=r, rho=ps.RHO, rank=rank)
    bnd = np.array([0, 7, ps.num_docs(case)], np.int64)
    v = [float(case["nv"][i]) for d in (6, 7, 8) for i in range(case["offs"][d], case["offs"][d + 1]) if case["rows"][i] == 3]
    assert len(v) == 3 and R["thr"][3, 1] == F(min(v)) == F(v[0]) < F(min(v[1:]))
    wrong = R["thr"].copy(order="F")
    wrong[3, 1] = F(min(v[1:]))
    with pytest.raises(AssertionError, match="thresholds differ"):
        ps.certify_post(case, "arms", r, rank, bnd, ps.reference_ranks(case, "arms", r, rank, bnd, thr=wrong))
    ps.certify_post(case, "arms", r, rank, bnd, ps.reference_ranks(case, "arms", r, rank, bnd))


def test_sums_rebased_wrongly_are_refused():
    case = ps.case_of("dts65")
    r, rank = ps.runs_of("dts65")[0]
    bnd = ps.bounds("H", case)
    with pytest.raises(AssertionError, match="offsets beginning at"):
        ps.certify_post(case, "dts65", r, rank, bnd, ps.reference_ranks(case, "dts65", r, rank, bnd, rebase=False))


@pytest.mark.parametrize("name,layout,leave_out", [("dts65", "H", 1), ("arms", "H", 0), ("select", "S1000", 2)])
def test_a_model_with_one_shard_left_out_is_refused(name, layout, leave_out):
    case = ps.case_of(name)
    r, rank = ps.runs_of(name)[0]
    bnd = ps.bounds(layout, case)
    with pytest.raises(AssertionError, match="model entries outside the bound|NaN pattern"):
        ps.certify_post(case, name, r, rank, bnd, ps.reference_ranks(case, name, r, rank, bnd, leave_out=leave_out))


def test_ranks_that_differ_are_refused():
    """a replicated result must be bit-identical on every rank"""
    case = ps.case_of("arms")
    r, rank = ps.runs_of("arms")[0]
    bnd = ps.bounds("H", case)
    for what in ("thr", "model", "mthr", "pairs", "tw"):
        ranks = [dict(q) for q in ps.reference_ranks(case, "arms", r, rank, bnd)]
        a = np.array(ranks[1][ps.key("arms", r, what)], copy=True)
        a.flat[0] = a.flat[0] + 1
        ranks[1][ps.key("arms", r, what)] = a
        with pytest.raises(AssertionError):
            ps.certify_post(case, "arms", r, rank, bnd, ranks)


def test_the_chunk_case_needs_a_second_chunk_of_bins():
    """more qualifying pairs than one all-reduce of bins takes, each with one value on either rank, the larger one on rank 0 for some and on
    rank 1 for others; the certificate accepts the reference and refuses the thresholds a rank finds among its own documents"""
    case = ps.chunk_case()
    D = ps.num_docs(case)
    assert D % 2 == 0 and ps.CHUNK_SLOTS < case["nslots"] == 65700 < 2 * ps.CHUNK_SLOTS
    assert case["arms"]["S > r >= n"] == 300 and case["nslots"] + 300 == case["V"] * case["topics"]
    doc_of = np.repeat(np.arange(D), np.diff(case["offs"]))
    rk = (doc_of >= D // 2).astype(np.int64)
    pair = case["rows"].astype(np.int64) * 2 + case["cl"][doc_of]
    per = np.zeros((case["V"] * 2, 2), np.int64)
    np.add.at(per, (pair, rk), 1)
    q = per.sum(1) == 2
    assert q.sum() == case["nslots"] and np.all(per[q] == 1)  # every segment: one value on each rank
    best = np.full((case["V"] * 2, 2), -1.0)
    np.maximum.at(best, (pair, rk), case["nv"].astype(np.float64))
    assert (best[q, 0] > best[q, 1]).sum() > 10000 and (best[q, 1] > best[q, 0]).sum() > 10000
    last = np.flatnonzero(q)[ps.CHUNK_SLOTS:]  # the pairs of the second chunk, in pair order
    assert len(last) == case["nslots"] - ps.CHUNK_SLOTS and len(np.unique(case["thr"].reshape(-1, order="C")[last])) > 50
    right = [{ps.key("chunk", 1, "thr"): case["thr"], ps.key("chunk", 1, "ct"): case["catch_topic"],
              ps.key("chunk", 1, "nc"): np.array([int((case["catch_topic"] >= 0).sum())])}] * 2
    ps.certify_chunk(case, right)
    o1 = int(case["offs"][D // 2])
    own, _ = stc.ref_catch_thresholds(case["V"], case["rows"][:o1], case["offs"][:D // 2 + 1], case["nv"][:o1], case["cl"][:D // 2], 2, 1)
    wrong = [dict(right[0], **{ps.key("chunk", 1, "thr"): own})] * 2
    with pytest.raises(AssertionError, match="thresholds differ"):
        ps.certify_chunk(case, wrong)


def test_the_worker_covers_what_the_certificate_reads():
    assert set(ps.WORLD) == set(ps.GENERAL_LAYOUTS) | set(ps.SELECT_LAYOUTS) | {"W1", "C2"} and max(ps.WORLD.values()) <= 4
    # one limit for every launch, rank_launch's: no case module has one of its own
    import doc_shard_cases
    import tdf_shard_cases
    assert rank_launch.LAUNCH_TIMEOUT_S == 60
    assert not any(hasattr(m, "LAUNCH_TIMEOUT_S") for m in (sc, ps, tdf_shard_cases, doc_shard_cases))
