"""isle_hip_similar_docs on document shards (N ranks on one GPU over the host-staged transport; tests/rank_launch.py): the rows of the tie,
no-candidate, exclude and empty cases of tests/simdocs_rule.py cut at row bounds (simdocs_rule.cuts: the tied documents span a shard
boundary, one rank has no rows, one rank has rows and no entries, an excluded document lies on another rank), every rank passing its own
doc_base and the same queries.  One launch per world (1: a communicator of one rank; 2; 3); every rank's four arrays equal the single-rank
rule on the uncut rows bit for bit, and are identical across the ranks.  A bad weight on the last rank alone is ISLE_E_ARG on every rank and
the next call works; differing queries are ISLE_E_COMM; query_rows is refused.  A launch that fails fails its tests and ends the launches:
nothing more is started on the GPU behind a fault, an abort or a time limit."""
from functools import partial

import numpy as np
import pytest

import rank_launch
import simdocs_rule as sr
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu
WORLDS = (1, 2, 3)
FIELDS = ("docs", "scores", "counts", "candidates")
_FAILED = []


def _call(hp, c, world, rank, measure, **kw):
    base, rows = sr.share(c, sr.cuts(c, world), rank)
    args = dict(source=rows, measure=measure, num_topics=c.num_topics, doc_base=base, exclude=c.given_exclude)
    args.update(kw)
    return hp.similar_docs((c.q_off, c.q_topic, c.q_weight), c.n, **args)


def _text(fn):
    from isle_amd import IsleHipError
    try:
        fn()
        return np.array("accepted")
    except IsleHipError as e:
        return np.array(str(e))


def _worker(hp, rank, world, res):
    for name in sr.SHARDED:
        c = sr.BY_NAME[name]
        for measure in sr.MEASURES:
            hp.simdocs_table_form(("lds", "global")[(rank + len(name)) % 2])  # the ranks need not agree on the table's home
            got = _call(hp, c, world, rank, measure)
            for f in FIELDS:
                res["%s.%s.%s" % (name, measure, f)] = got[f].view(np.uint32) if f == "scores" else got[f]
    hp.simdocs_table_form("auto")
    # a bad weight on the last rank alone: every rank returns ISLE_E_ARG, the last names its entry, and the context stays usable
    off, topic, weight = sr.GOOD_ROWS
    weight = weight.copy()
    weight[2201] = np.float32("nan")
    case = sr.Case("refusal", 3, 5, 0, (off, topic, weight), sr.GOOD_QUERIES)
    cut = [0] + [1100] * (world - 1) + [case.rows] if world > 1 else [0, case.rows]
    base, rows = sr.share(case, cut, rank)
    res["refusal"] = _text(lambda: hp.similar_docs(sr.GOOD_QUERIES, 5, rows, "dot", num_topics=3, doc_base=base))
    c = sr.BY_NAME[sr.SHARDED[0]]
    res["after.docs"] = _call(hp, c, world, rank, "cosine")["docs"]
    # queries that differ on the last rank, an exclude that differs on the last rank
    q_off, q_topic, q_weight = sr.GOOD_QUERIES
    mine = q_weight.copy()
    if rank == world - 1:
        mine[0] = np.float32(1.5)
    good = sr.Case("good", 3, 5, 0, sr.GOOD_ROWS, sr.GOOD_QUERIES)
    base, rows = sr.share(good, sr.cuts(good, world), rank)
    res["differ.queries"] = _text(lambda: hp.similar_docs((q_off, q_topic, mine), 5, rows, "dot", num_topics=3, doc_base=base))
    res["differ.exclude"] = _text(lambda: hp.similar_docs(sr.GOOD_QUERIES, 5, rows, "dot", num_topics=3, doc_base=base,
                                                          exclude=[7, 9 if rank == world - 1 else 8]))
    res["query_rows"] = _text(lambda: hp.similar_docs(np.array([0], np.uint64), 5, sr.GOOD_ROWS, "dot", num_topics=3))
    res["after.all"] = _call(hp, c, world, rank, "cosine")["docs"]


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


def _launch(world, tmp):
    return rank_launch.launch("similar docs W%d" % world, "simdocs_W%d" % world, world, tmp, rank_launch.module_command("test_gpu_similar_docs_sharded", world))


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("similar_docs_shards"))
    return launch_each([(w, "W%d" % w, partial(_launch, w, tmp)) for w in WORLDS], _FAILED)


@pytest.fixture(scope="module")
def rules():
    return {(n, m): sr.rule(sr.BY_NAME[n], sr.MEASURES[m]) for n in sr.SHARDED for m in sr.MEASURES}


@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_returns_the_single_rank_lists(launches, rules, world):
    ranks = ranks_of(launches, world)
    assert len(ranks) == world
    for (name, measure), want in rules.items():
        for q, res in enumerate(ranks):
            what = (name, measure, world, q)
            for f in FIELDS:
                key = "%s.%s.%s" % (name, measure, f)
                assert np.array_equal(res[key], want[f]), what + (f,)
                assert res[key].tobytes() == ranks[0][key].tobytes(), what + (f,)  # identical across the ranks, byte for byte


@pytest.mark.parametrize("world", WORLDS)
def test_a_bad_weight_on_the_last_rank_is_refused_on_every_rank(launches, rules, world):
    ranks = ranks_of(launches, world)
    texts = [str(res["refusal"]) for res in ranks]
    assert all("isle_hip error -1" in t for t in texts), texts
    if world == 1:
        assert "entry 2201 (row 1100) has weight" in texts[0]
    else:
        assert "entry 1 (row 0) has weight" in texts[-1]  # the last rank's share begins at row 1100: entry 2201 is its entry 1
        assert all("another rank refused its rows" in t for t in texts[:-1])
    for res in ranks:
        assert np.array_equal(res["after.docs"], rules[sr.SHARDED[0], "cosine"]["docs"])


@pytest.mark.parametrize("world", WORLDS)
def test_differing_queries_are_a_comm_error_and_query_rows_are_refused(launches, rules, world):
    ranks = ranks_of(launches, world)
    for res in ranks:
        if world == 1:
            assert str(res["differ.queries"]) == "accepted" and str(res["differ.exclude"]) == "accepted" and str(res["query_rows"]) == "accepted"
        else:
            for key in ("differ.queries", "differ.exclude"):
                assert "isle_hip error -5" in str(res[key]) and "ranks disagree on the queries" in str(res[key]), str(res[key])
            assert "isle_hip error -1" in str(res["query_rows"]) and "query_rows with %d ranks" % world in str(res["query_rows"])
        assert np.array_equal(res["after.all"], rules[sr.SHARDED[0], "cosine"]["docs"])


def test_the_cuts_are_what_the_test_is_about():
    ties = [sr.BY_NAME[n] for n in sr.SHARDED if sr.BY_NAME[n].aim == "tie"]
    assert ties and all(0 < c.off[sr.cuts(c, 2)[1]] < c.topic.size for c in ties)        # the tied documents span the boundary of two ranks
    b = sr.cuts(ties[0], 3)
    assert b[1] == b[2] > 0 and ties[0].off[b[1]] == 0                                  # rank 0: rows and no entries; rank 1: no rows
    e = sr.BY_NAME["exclude_hits_and_misses"]
    cut = sr.cuts(e, 2)[1]
    hit = [int(x) - e.doc_base for x in e.given_exclude if e.doc_base <= int(x) < e.doc_base + e.rows]
    assert any(r < cut for r in hit) and any(r >= cut for r in hit)                     # each rank excludes a document of the other
    assert {sr.BY_NAME[n].aim for n in sr.SHARDED} >= {"tie", "no_match", "exclude", "no_entries"}
