"""Inference and the per-document reports on document shards (N ranks on one GPU over the host-staged transport) against the
single-rank run on the whole corpus (tests/doc_shard_cases.py): the four report kinds and the two inference texts of the ranks side by
side byte-equal to the host statements applied to the plain single-rank arrays, nbytes / nlines per rank, the inference arrays bit-equal
to the one-rank launch's, avg_doc_sz the corpus value.  Each layout's worker runs once per module; the tests certify what it stored, on
the host.  A launch that fails fails that layout's tests and ends the launches: nothing more is started on the GPU behind a fault, an
abort or a time limit."""
from functools import partial

import numpy as np
import pytest

import doc_shard_cases as dc
from rank_launch import launch_each, ranks_of, write_report

pytestmark = pytest.mark.gpu

MULTI = tuple(l for l in dc.LAYOUTS if dc.WORLD[l] > 1)
REPORT = []  # (layout, what, verdict)
_FAILED = []  # the first launch of this module that failed: nothing is started behind it


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """layout -> its launch, one launch after another"""
    tmp = str(tmp_path_factory.mktemp("doc_shards"))
    return launch_each([(layout, layout, partial(dc.launch, layout, tmp)) for layout in dc.LAYOUTS], _FAILED)


@pytest.fixture(scope="module", autouse=True)
def report(launches):
    """At the end of the module: the launch times and per case and layout "bytes equal" or the first differing line, printed (shown
    with -s or on a failure) and written to the file ISLE_DOC_SHARD_REPORT names."""
    yield
    lines = ["doc shard certificate, launch %s (%d ranks): %.1f s" % (name, dc.WORLD[name], l["wall"]) for name, l in launches.items() if isinstance(l, dict)]
    lines += ["doc shard certificate, %s on %s: %s" % (what, layout, verdict) for layout, what, verdict in REPORT]
    write_report(lines, "ISLE_DOC_SHARD_REPORT")


def single_of(launches, prefix):
    """the single-rank inference result: what the one-rank launch computed on the whole corpus"""
    res = ranks_of(launches, "W1")[0]
    return {f: res["%s_%s" % (prefix, f)] for f in ("tt", "tw", "llh", "off", "topic", "weight")}


def noted(layout, what, fn):
    try:
        verdict = fn()
    except AssertionError as e:
        REPORT.append((layout, what, str(e).splitlines()[0]))
        raise
    if isinstance(verdict, dict):
        REPORT.extend((layout, k, v) for k, v in verdict.items())
    else:
        REPORT.append((layout, what, verdict))


@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_reports_side_by_side_are_the_single_rank_files(launches, layout):
    """catchwords, topic_sums, topic_sums_by_doc and top_two of every rank, and topic_sums over ranges with fewer sums than ranks and with
    none: bytes, nbytes, nlines (the call's and the size query's) and whether the sink was called"""
    ranks = ranks_of(launches, layout)
    noted(layout, "reports", lambda: dc.certify_reports(layout, ranks))


@pytest.mark.parametrize("layout", MULTI)
def test_a_refusing_sink_on_rank_1_leaves_the_others_to_complete(launches, layout):
    dc.certify_sink_refusal(layout, ranks_of(launches, layout))


@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_avg_doc_sz_is_the_corpus_value(launches, layout):
    """floor(tokens / non-empty documents) in numpy: once behind threshold (a_avg valid), once with B from the host (the inference call
    makes the all-reduce), and as every inference call reports it"""
    ranks = ranks_of(launches, layout)
    for name in ("avg_th", "hb_avg", "inf_avg", "ld_avg", "in_avg"):
        dc.certify_avg(layout, ranks, name)


@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_inference_is_the_single_rank_inference_bit_for_bit(launches, layout):
    """under the host model with both texts, with B from the host, under the loaded model, and on an inner range in chunks with texts
    numbered from base + a_doc_offset + b"""
    ranks = ranks_of(launches, layout)
    noted(layout, "infer_resident, its texts", lambda: dc.certify_infer(layout, ranks, single_of(launches, "inf"), "inf"))
    noted(layout, "infer_resident with B from the host", lambda: dc.certify_infer(layout, ranks, single_of(launches, "inf"), "hb"))
    noted(layout, "infer_resident under the loaded model", lambda: dc.certify_infer(layout, ranks, single_of(launches, "ld"), "ld"))
    noted(layout, "inner ranges in chunks, their texts", lambda: dc.certify_infer(layout, ranks, single_of(launches, "ld"), "in", inner=True))


def test_the_one_rank_launch_gives_something_to_compare(launches):
    """the single-rank reference itself: documents converged and entries exist under both models, and none for the empty documents"""
    res = ranks_of(launches, "W1")[0]
    lens = np.diff(dc.corpus()["offs"])
    assert int(res["inf_nc"]) > 1000 and int(res["inf_ne"]) > 1000 and int(res["ld_nc"]) > 1000 and int(res["ld_ne"]) > 1000
    assert (np.diff(res["inf_off"])[lens == 0] == 0).all() and (res["inf_tt"][lens == 0] == -1).all()


@pytest.mark.parametrize("layout", MULTI)
def test_what_is_not_built_is_still_refused(launches, layout):
    """avg_topic_model, topic_coherence, log_combinatorial, distinct_top_five and model="avg" in the readers, with their messages"""
    dc.certify_refusals(layout, ranks_of(launches, layout))


def test_the_writers_domain_applies_to_the_number_in_the_corpus(launches):
    """doc_shard_cases.domain_case: a shard uploaded at document 0x7ffffffd prints 0x7ffffffe and refuses 0x7fffffff, naming the local
    and the corpus's document (upload_counts and the catchword stage accept the offset: no collective checks that the shards tile the
    corpus)"""
    dc.certify_domain(ranks_of(launches, dc.DOMAIN_LAYOUT))
