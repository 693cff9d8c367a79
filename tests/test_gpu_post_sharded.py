"""Catchwords, the topic model and the edge pairs on column-sharded documents (N ranks on one GPU over the host-staged transport) against
the plain reference of the single-rank stage (tests/post_shard_cases.py): thresholds, catch topics, rank thresholds and edge pairs bit
for bit and bit-identical on every rank, the per-document results of the shards side by side, the model bit-identical on every rank and
within the single-rank certificate's bound of fp64.  Each layout's worker runs once per module; the tests certify the arrays it stored,
on the host.  A launch that fails fails that layout's tests and ends the launches: nothing more is started on the GPU behind a fault, an
abort or a time limit."""
from functools import partial

import numpy as np
import pytest

import post_shard_cases as ps
from rank_launch import launch_each, ranks_of, write_report

pytestmark = pytest.mark.gpu

LAYOUTS = ps.GENERAL_LAYOUTS + ps.SELECT_LAYOUTS + ("W1", "C2")
REPORT = []  # (case, layout, largest model error / bound)
_FAILED = []  # the first launch of this module that failed: nothing is started behind it


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """layout -> its launch (every case of the layout, every run of the case), one launch after another"""
    tmp = str(tmp_path_factory.mktemp("post_shards"))
    return launch_each([(layout, layout, partial(ps.launch, layout, tmp)) for layout in LAYOUTS], _FAILED)


@pytest.fixture(scope="module", autouse=True)
def report(launches):
    """At the end of the module: the launch times and the largest error / bound of the model per case, printed (shown with -s or on a
    failure) and written to the file ISLE_POST_SHARD_REPORT names."""
    yield
    lines = ["post shard certificate, launch %s (%d ranks): %.1f s" % (name, ps.WORLD[name], l["wall"]) for name, l in launches.items() if isinstance(l, dict)]
    lines += ["post shard certificate, %s on %s: model max error / bound %.3g" % r for r in REPORT]
    write_report(lines, "ISLE_POST_SHARD_REPORT")


def _certify(launches, name, layout):
    case, ranks = ps.case_of(name), ranks_of(launches, layout)
    bnd = ps.bounds(layout, case)
    worst = 0.0
    for r, rank in ps.runs_of(name):
        worst = max(worst, ps.certify_post(case, name, r, rank, bnd, ranks)["model_ratio"])
    REPORT.append((name, layout, worst))
    return ranks


@pytest.mark.parametrize("layout", ps.GENERAL_LAYOUTS)
@pytest.mark.parametrize("name", ps.CASE_NAMES)
def test_sharded_stage(launches, name, layout):
    """Every downstream case on two ranks, on a one-document shard beside an empty one, and on empty first and middle shards; p_select_case
    with r = rank over select_ranks()."""
    ranks = _certify(launches, name, layout)
    if name != "select":
        case = ps.case_of(name)
        r = ps.runs_of(name)[0][0]
        t = 3 if name == "arms" else case["empty_topic"]
        assert all(np.isnan(q[ps.key(name, r, "model")][:, t]).all() for q in ranks)  # the empty topic: a NaN column on every rank


@pytest.mark.parametrize("layout", ps.SELECT_LAYOUTS)
def test_select_on_cut_segments(launches, layout):
    """p_select_case with the three segments of one length cut in the middle (post_shard_cases.select_layout_facts): the r-th largest
    value on the first part, on the second, in a run that spans the cut, and among values that share their top 16 bits, for r == n - 1,
    n and n + 1 of every length."""
    _certify(launches, "select", layout)


@pytest.mark.parametrize("name", ps.CASE_NAMES)
def test_a_communicator_of_one_rank_gives_the_single_rank_results(launches, name):
    _certify(launches, name, "W1")


def test_more_slots_than_one_chunk_of_bins(launches):
    """post_shard_cases.chunk_case: 65 700 segments, each with one value on either rank, walked in two chunks of bins; B from the host, so the
    corpus totals behind avg_doc_sz are summed over the ranks in the catchword call"""
    ps.certify_chunk(ps.chunk_case(), ranks_of(launches, "C2"))


def test_the_average_model_is_still_refused_with_two_ranks(launches):
    for q in ranks_of(launches, "H"):
        assert str(q["avg_refused"]).endswith(": avg_topic_model: single-rank only"), str(q["avg_refused"])
