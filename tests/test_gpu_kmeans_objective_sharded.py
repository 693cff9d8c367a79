"""isle_hip_kmeans_objective and the Lloyd trace on document shards (N ranks on one GPU over the host-staged transport,
tests/objective_shard_cases.py): an odd split, a one-document shard, empty first, middle and last shards, and the entry-balanced plan.
Sums, sizes and total of every rank are the one-rank launch's bit for bit, the ranks' doc_dist side by side are its array, in both
spaces; the one-rank launch itself lies within tests/objective_certificate.py.  One launch per layout, one after another; a launch
that fails fails its tests and ends the launches: nothing more is started on the GPU behind a fault, an abort or a time limit."""
from functools import partial

import pytest

import objective_shard_cases as osc
from rank_launch import launch_each, ranks_of, write_report

pytestmark = pytest.mark.gpu

MULTI = tuple(l for l in osc.LAYOUTS if osc.WORLD[l] > 1)
REPORT = []
_FAILED = []  # the first launch of this module that failed: nothing is started behind it


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("objective_shards"))
    return launch_each([(layout, layout, partial(osc.launch, layout, tmp)) for layout in osc.LAYOUTS], _FAILED)


@pytest.fixture(scope="module", autouse=True)
def report(launches):
    """the launch times and the ratios of error to bound, printed (shown with -s or on a failure) and written to the file
    ISLE_OBJECTIVE_SHARD_REPORT names"""
    yield
    lines = ["objective shard certificate, launch %s (%d ranks): %.1f s" % (n, osc.WORLD[n], l["wall"]) for n, l in launches.items() if isinstance(l, dict)]
    write_report(lines + REPORT, "ISLE_OBJECTIVE_SHARD_REPORT")


@pytest.mark.parametrize("k", osc.KS)
def test_the_one_rank_launch_lies_within_the_certificate(launches, k):
    single = ranks_of(launches, "W1")[0]
    for tag, worst in osc.certify_single(single, k).items():
        REPORT.append("objective shard certificate, W1 %s: worst error / bound %r" % (tag, worst))
    assert single["w%d_sums" % k][k - 1] == 0.0 and single["w%d_sizes" % k][k - 1] == 0


@pytest.mark.parametrize("layout", MULTI)
def test_every_rank_holds_the_one_rank_sums_and_the_distances_lie_side_by_side(launches, layout):
    """a rank without documents returns the replicated values too"""
    ranks, single = ranks_of(launches, layout), ranks_of(launches, "W1")[0]
    bnd = osc.bounds(layout)
    for k in osc.KS:
        for tag in ("w%d" % k, "p%d" % k):
            osc.certify_replicated(ranks, single, tag)
            osc.certify_side_by_side(ranks, single, tag, bnd)


@pytest.mark.parametrize("layout", osc.LAYOUTS)
def test_the_trace_of_a_sharded_loop_is_replicated_and_within_the_certificate_of_its_final_state(launches, layout):
    tr, ratio = osc.certify_trace(ranks_of(launches, layout))
    REPORT.append("objective shard certificate, %s trace %r: last entry error / bound %.3g" % (layout, [float(x) for x in tr], ratio))
