"""isle_hip_word_doc_freq / isle_hip_prune_vocab on document shards (N ranks on one GPU over the host-staged transport;
tests/rank_launch.py): the sharded cases of tests/vocab_rule.py cut at document bounds (vocab_rule.cuts: a word reaches min_df = 2 only summed
over two ranks, one rank has no documents, one has documents and no entries, keep_n cuts through a tie), every rank uploading its own
documents with its doc_offset and the corpus's document count.  One launch per world (1: a communicator of one rank; 2; 3); every rank's A
equals its slice of the single-rank rule's result bit for bit, and df, kept_words, vocab and docs_emptied are byte-identical across the
ranks.  The nothing-kept refusal arrives on every rank and leaves the context usable.  A launch that fails fails its tests and ends the
launches: nothing more is started on the GPU behind a fault, an abort or a time limit."""
from functools import partial

import numpy as np
import pytest

import rank_launch
import vocab_rule as vr
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu
WORLDS = (1, 2, 3)
_FAILED = []


def _upload(hp, case, world, rank):
    offs, rows, counts, base = vr.share(case, vr.cuts(case, world), rank)
    hp.upload_counts(case.V, counts, rows, offs, doc_offset=base, docs_global=case.offs.size - 1)


def _worker(hp, rank, world, res):
    from isle_amd import IsleHipError
    for i, c in enumerate(vr.SHARDED):
        hp.vocab_hist_form(("lds", "global")[i % 2])
        _upload(hp, c, world, rank)
        res[c.name + ".df0"] = hp.word_doc_freq()
        got = hp.prune_vocab(min_df=c.min_df, max_df=c.max_df or None, keep_n=c.keep_n or None)
        cnt, rows, offs = hp.get_A()
        res[c.name + ".df"], res[c.name + ".kept"] = got["df"], got["kept_words"]
        res[c.name + ".scalars"] = np.array([got["vocab"], got["docs_emptied"]], np.uint64)
        res[c.name + ".nnz"] = np.array([got["nnz"]], np.uint64)
        res[c.name + ".offs"], res[c.name + ".rows"], res[c.name + ".counts"] = offs, rows, cnt.view(np.uint32)
    # nothing kept: every rank returns ISLE_E_ARG with the same text, its A stays, and the context goes on
    r = vr.SHARD_REFUSAL
    _upload(hp, r, world, rank)
    try:
        hp.prune_vocab(min_df=r.min_df)
        res["refusal"] = np.array("accepted")
    except IsleHipError as e:
        res["refusal"] = np.array(str(e))
    cnt, rows, offs = hp.get_A()
    res["refusal.offs"], res["refusal.rows"] = offs, rows
    res["after.kept"] = hp.prune_vocab(min_df=2)["kept_words"]


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


def _launch(world, tmp):
    return rank_launch.launch("vocab prune W%d" % world, "vocab_W%d" % world, world, tmp, rank_launch.module_command("test_gpu_vocab_prune_sharded", world))


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("vocab_prune_shards"))
    return launch_each([(w, "W%d" % w, partial(_launch, w, tmp)) for w in WORLDS], _FAILED)


@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_holds_its_slice_of_the_single_rank_result(launches, world):
    ranks = ranks_of(launches, world)
    assert len(ranks) == world
    for c in vr.SHARDED:
        want, cut = vr.rule(c), vr.cuts(c, world)
        for q, res in enumerate(ranks):
            what = (c.name, world, q)
            assert np.array_equal(res[c.name + ".df0"], want["df"]) and np.array_equal(res[c.name + ".df"], want["df"]), what
            assert np.array_equal(res[c.name + ".kept"], want["kept_words"]), what
            assert res[c.name + ".scalars"].tolist() == [want["vocab"], want["docs_emptied"]], what
            offs, rows, bits = vr.rule_share(c, cut, q)
            assert np.array_equal(res[c.name + ".offs"], offs) and np.array_equal(res[c.name + ".rows"], rows), what
            assert np.array_equal(res[c.name + ".counts"], bits) and int(res[c.name + ".nnz"][0]) == rows.size, what
            for f in ("df0", "df", "kept", "scalars"):  # identical across the ranks, byte for byte
                assert res["%s.%s" % (c.name, f)].tobytes() == ranks[0]["%s.%s" % (c.name, f)].tobytes(), what


@pytest.mark.parametrize("world", WORLDS)
def test_nothing_kept_is_refused_on_every_rank_and_the_context_goes_on(launches, world):
    ranks = ranks_of(launches, world)
    r = vr.SHARD_REFUSAL
    for q, res in enumerate(ranks):
        assert str(res["refusal"]) == "isle_hip error -1: " + vr.rule(r)["text"], (world, q)
        offs, rows, _, _ = vr.share(r, vr.cuts(r, world), q)
        assert np.array_equal(res["refusal.offs"], offs) and np.array_equal(res["refusal.rows"], rows)
        assert np.array_equal(res["after.kept"], vr.rule(r._replace(min_df=2))["kept_words"])
