"""The near-duplicate calls under a communicator of two ranks (one GPU, the host-staged transport; tests/rank_launch.py): similarity across
ranks needs the contents exchanged, which is out of scope, so isle_hip_doc_near_duplicates, isle_hip_prune_near_docs and
isle_hip_doc_jaccard (and isle_hip_doc_signatures with them) are refused on every rank with the rule's text before any collective: no rank
waits for another, and each rank's A stays as it uploaded it.  One launch."""
from functools import partial

import numpy as np
import pytest

import docs_rule as dr
import neardup_rule as nr
import rank_launch
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu
WORLD = 2
CASE = nr.BY_NAME["lengths_16x4"]
CALLS = (("doc_near_duplicates", lambda hp: hp.near_duplicates((4, 5), 16, 4)), ("prune_near_docs", lambda hp: hp.prune_near_docs((4, 5), 16, 4)),
         ("doc_jaccard", lambda hp: hp.doc_jaccard([0], [0])), ("doc_signatures", lambda hp: hp.doc_signatures(16, 4)))
_FAILED = []


def _cut():
    D = CASE.offs.size - 1
    return [0, D // 2, D]


def _worker(hp, rank, world, res):
    from isle_amd import IsleHipError
    offs, rows, counts, base = dr.share(CASE, _cut(), rank)
    hp.upload_counts(CASE.V, counts, rows, offs, doc_offset=base, docs_global=CASE.offs.size - 1)
    for who, call in CALLS:
        try:
            call(hp)
            res[who] = np.array("accepted")
        except IsleHipError as e:
            res[who] = np.array(str(e))
    cnt, r, o = hp.get_A()
    res["offs"], res["rows"], res["counts"] = o, r, cnt.view(np.uint32)
    res["at"] = np.array([hp.a_doc_offset, hp._counts_shape()[4]], np.uint64)


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


def _launch(tmp):
    return rank_launch.launch("near dups W%d" % WORLD, "near_dups_W%d" % WORLD, WORLD, tmp, rank_launch.module_command("test_gpu_near_dups_sharded", WORLD))


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("near_dups_shards"))
    return launch_each([(WORLD, "W%d" % WORLD, partial(_launch, tmp))], _FAILED)


def test_the_calls_are_refused_on_every_rank_before_any_collective(launches):
    ranks = ranks_of(launches, WORLD)
    assert len(ranks) == WORLD
    for q, res in enumerate(ranks):
        for who, _ in CALLS:
            want = nr.check_args(who, True, 4, 5, 16, 4, world=WORLD)
            assert want.endswith("needs the contents exchanged: out of scope") and str(res[who]) == "isle_hip error -1: " + want, (q, who)
        offs, rows, counts, base = dr.share(CASE, _cut(), q)
        assert np.array_equal(res["offs"], offs) and np.array_equal(res["rows"], rows) and np.array_equal(res["counts"], counts.view(np.uint32))
        assert res["at"].tolist() == [base, CASE.offs.size - 1]
