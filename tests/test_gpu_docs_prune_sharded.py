"""isle_hip_prune_docs on document shards (N ranks on one GPU over the host-staged transport; tests/rank_launch.py): the sharded cases of
tests/docs_rule.py cut at document bounds (docs_rule.cuts: one rank has no documents, one has documents that are all dropped, another
case leaves a rank with nothing, so that doc_offset of the ranks above it moves), every rank uploading its own documents with its
doc_offset and the corpus's document count.  One launch per world (1: a communicator of one rank; 2; 3); every rank's A, kept_docs and
doc_offset equal its slice of the single-rank rule's result bit for bit, and docs_global and dropped are byte-identical across the ranks.
The nothing-kept refusal arrives on every rank with one text and leaves the context usable.  drop_duplicates and doc_duplicates are
refused on every rank of a world of 2 or 3 before any collective: no rank waits for another.  A launch that fails fails its tests and
ends the launches: nothing more is started on the GPU behind a fault, an abort or a time limit."""
from functools import partial

import numpy as np
import pytest

import docs_rule as dr
import rank_launch
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu
WORLDS = (1, 2, 3)
_FAILED = []


def _upload(hp, case, world, rank):
    offs, rows, counts, base = dr.share(case, dr.cuts(case, world), rank)
    hp.upload_counts(case.V, counts, rows, offs, doc_offset=base, docs_global=case.offs.size - 1)


def _prune(hp, c, **kw):
    return hp.prune_docs(min_words=c.min_words, max_words=c.max_words or None, min_tokens=c.min_tokens, max_tokens=c.max_tokens or None, **kw)


def _text(call):
    from isle_amd import IsleHipError
    try:
        call()
        return np.array("accepted")
    except IsleHipError as e:
        return np.array(str(e))


def _worker(hp, rank, world, res):
    for c in dr.SHARDED:
        _upload(hp, c, world, rank)
        words, tokens = hp.doc_lengths()      # per rank, never collective
        res[c.name + ".words"], res[c.name + ".tokens"] = words, tokens
        if world > 1:   # refused on every rank before any collective: a rank that went on alone would wait for the others until the time limit
            res[c.name + ".dups"] = _text(lambda: _prune(hp, c, drop_duplicates=True))
            res[c.name + ".find"] = _text(hp.doc_duplicates)
        got = _prune(hp, c)
        cnt, rows, offs = hp.get_A()
        res[c.name + ".kept"], res[c.name + ".first"] = got["kept_docs"], got["first_of"]
        res[c.name + ".global"] = np.array([got["docs_global"], got["dropped_short"], got["dropped_long"], got["dropped_duplicate"]], np.uint64)
        res[c.name + ".own"] = np.array([got["docs"], got["nnz"], hp.a_doc_offset, hp._counts_shape()[4]], np.uint64)
        res[c.name + ".offs"], res[c.name + ".rows"], res[c.name + ".counts"] = offs, rows, cnt.view(np.uint32)
    # nothing kept: every rank returns ISLE_E_ARG with the same text, its A stays, and the context goes on
    r = dr.SHARD_REFUSAL
    _upload(hp, r, world, rank)
    res["refusal"] = _text(lambda: _prune(hp, r))
    cnt, rows, offs = hp.get_A()
    res["refusal.offs"], res["refusal.rows"] = offs, rows
    res["refusal.at"] = np.array([hp.a_doc_offset, hp._counts_shape()[4]], np.uint64)
    res["after.kept"] = hp.prune_docs(min_words=2)["kept_docs"]


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


def _launch(world, tmp):
    return rank_launch.launch("docs prune W%d" % world, "docs_W%d" % world, world, tmp, rank_launch.module_command("test_gpu_docs_prune_sharded", world))


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("docs_prune_shards"))
    return launch_each([(w, "W%d" % w, partial(_launch, w, tmp)) for w in WORLDS], _FAILED)


@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_holds_its_slice_of_the_single_rank_result(launches, world):
    ranks = ranks_of(launches, world)
    assert len(ranks) == world
    for c in dr.SHARDED:
        want, cut = dr.rule(c), dr.cuts(c, world)
        for q, res in enumerate(ranks):
            what = (c.name, world, q)
            b, e = cut[q], cut[q + 1]
            assert np.array_equal(res[c.name + ".words"], want["words"][b:e]) and np.array_equal(res[c.name + ".tokens"], want["tokens"][b:e]), what
            offs, rows, bits, kept, base = dr.rule_share(c, cut, q)
            assert np.array_equal(res[c.name + ".offs"], offs) and np.array_equal(res[c.name + ".rows"], rows) and np.array_equal(res[c.name + ".counts"], bits), what
            assert np.array_equal(res[c.name + ".kept"], kept), what
            first = want["first_of"][b:e].astype(np.int64)
            assert np.array_equal(res[c.name + ".first"], np.where(first == dr.DROPPED, dr.DROPPED, first - b).astype(np.uint32)), what   # local numbers
            assert res[c.name + ".own"].tolist() == [kept.size, rows.size, base, want["docs"]], what
            assert res[c.name + ".global"].tolist() == [want["docs"]] + want["dropped"], what
            assert res[c.name + ".global"].tobytes() == ranks[0][c.name + ".global"].tobytes(), what      # identical across the ranks, byte for byte


@pytest.mark.parametrize("world", WORLDS)
def test_nothing_kept_is_refused_on_every_rank_and_the_context_goes_on(launches, world):
    ranks = ranks_of(launches, world)
    r = dr.SHARD_REFUSAL
    for q, res in enumerate(ranks):
        assert str(res["refusal"]) == "isle_hip error -1: " + dr.rule(r)["text"], (world, q)
        offs, rows, _, base = dr.share(r, dr.cuts(r, world), q)
        assert np.array_equal(res["refusal.offs"], offs) and np.array_equal(res["refusal.rows"], rows)
        assert res["refusal.at"].tolist() == [base, r.offs.size - 1]
        assert np.array_equal(res["after.kept"], dr.rule_share(r._replace(min_words=2), dr.cuts(r, world), q)[3])


@pytest.mark.parametrize("world", (2, 3))
def test_duplicates_are_refused_on_every_rank_before_any_collective(launches, world):
    for q, res in enumerate(ranks_of(launches, world)):
        for c in dr.SHARDED:
            assert str(res[c.name + ".dups"]) == "isle_hip error -1: " + dr.check_args(c.min_words, c.max_words, c.min_tokens, c.max_tokens, 1, world=world), (world, q)
            assert str(res[c.name + ".find"]) == "isle_hip error -1: " + dr.check_args(0, 0, 0, 0, 1, world=world, who="doc_duplicates"), (world, q)
