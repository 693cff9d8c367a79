"""isle_hip_topic_top_docs on document shards (N ranks on one GPU over the host-staged transport; tests/rank_launch.py): the triples of the
tie, value-byte, empty and bins'-home cases of tests/topdocs_rule.py cut at row bounds (topdocs_rule.cuts: the tied documents span a shard
boundary, one rank has no rows, one rank has rows and no entries), every rank passing its own doc_base.  One launch per world (1: a
communicator of one rank; 2; 3); every rank's four arrays equal the single-rank rule on the uncut triples bit for bit, and are identical
across the ranks.  A launch that fails fails its tests and ends the launches: nothing more is started on the GPU behind a fault, an abort
or a time limit."""
from functools import partial

import numpy as np
import pytest

import rank_launch
import topdocs_rule as tr
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu
WORLDS = (1, 2, 3)
_FAILED = []


def _worker(hp, rank, world, res):
    from isle_amd import IsleHipError
    for name in tr.SHARDED:
        c = tr.BY_NAME[name]
        base, off, topic, bits = tr.share(c, tr.cuts(c, world), rank)
        got = hp.topic_top_docs(c.n, (off, topic, bits.view(np.float32)), num_topics=c.num_topics, doc_base=base)
        res[name + ".docs"], res[name + ".values"] = got["docs"], got["values"].view(np.uint32)
        res[name + ".counts"], res[name + ".entries"] = got["counts"], got["topic_entries"]
    # a bad entry on the first and on the last rank, none between: every rank returns ISLE_E_ARG, a rank that holds one names its own, and
    # the context stays usable
    r = tr.REFUSALS[0]
    case = tr.Case("refusal", r.num_topics, r.n, 0, r.off, r.topic, r.bits, "refusal")
    cut = [0] + [1100] * (world - 1) + [case.rows] if world > 1 else [0, case.rows]   # entry 1401 lies on rank 0, entry 2201 on the last
    base, off, topic, bits = tr.share(case, cut, rank)
    try:
        hp.topic_top_docs(r.n, (off, topic, bits.view(np.float32)), num_topics=r.num_topics, doc_base=base)
        res["refusal"] = np.array("accepted")
    except IsleHipError as e:
        res["refusal"] = np.array(str(e))
    c = tr.BY_NAME[tr.SHARDED[0]]
    base, off, topic, bits = tr.share(c, tr.cuts(c, world), rank)
    res["after.docs"] = hp.topic_top_docs(c.n, (off, topic, bits.view(np.float32)), num_topics=c.num_topics, doc_base=base)["docs"]


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


def _launch(world, tmp):
    return rank_launch.launch("top docs W%d" % world, "topdocs_W%d" % world, world, tmp, rank_launch.module_command("test_gpu_top_docs_sharded", world))


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("top_docs_shards"))
    return launch_each([(w, "W%d" % w, partial(_launch, w, tmp)) for w in WORLDS], _FAILED)


@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_returns_the_single_rank_lists(launches, world):
    ranks = ranks_of(launches, world)
    assert len(ranks) == world
    for name in tr.SHARDED:
        c = tr.BY_NAME[name]
        want = tr.rule(c)
        for q, res in enumerate(ranks):
            what = (name, world, q)
            assert np.array_equal(res[name + ".counts"], want["counts"]) and np.array_equal(res[name + ".entries"], want["topic_entries"]), what
            assert np.array_equal(res[name + ".docs"], want["docs"]), what
            assert np.array_equal(res[name + ".values"], want["values"]), what
            for f in ("docs", "values", "counts", "entries"):  # identical across the ranks, byte for byte
                assert res["%s.%s" % (name, f)].tobytes() == ranks[0]["%s.%s" % (name, f)].tobytes(), what


@pytest.mark.parametrize("world", WORLDS)
def test_a_bad_entry_on_one_rank_is_refused_on_every_rank(launches, world):
    ranks = ranks_of(launches, world)
    texts = [str(res["refusal"]) for res in ranks]
    assert all("isle_hip error -1" in t for t in texts), texts
    assert "entry 1401 (row 700) has topic 3 >= num_topics 3" in texts[0]
    if world > 1:
        assert "entry 1 (row 0) has topic 3 >= num_topics 3" in texts[-1]  # the last rank's share begins at row 1100: its entry 2201 is its entry 1
        assert all("another rank refused its entries" in t for t in texts[1:-1])
    c = tr.BY_NAME[tr.SHARDED[0]]
    for res in ranks:
        assert np.array_equal(res["after.docs"], tr.rule(c)["docs"])


def test_the_cuts_are_what_the_test_is_about():
    for name in tr.SHARDED:
        c = tr.BY_NAME[name]
        assert c.device and c.n <= tr.MAX_N
    ties = [tr.BY_NAME[n] for n in tr.SHARDED if tr.BY_NAME[n].aim == "tie"]
    assert ties and all(0 < c.off[tr.cuts(c, 2)[1]] < c.topic.size for c in ties)        # the tied documents span the boundary of two ranks
    b = tr.cuts(ties[0], 3)
    assert b[1] == b[2] > 0 and ties[0].off[b[1]] == 0                                  # rank 0: rows and no entries; rank 1: no rows
    assert {tr.BY_NAME[n].num_topics for n in tr.SHARDED if tr.BY_NAME[n].aim == "bins"} == {3, 64, 65, 257}
