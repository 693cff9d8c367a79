"""One tdf file onto document shards on 2, 3 and 4 ranks (one GPU, host-staged transport; tests/tdf_shard_cases.py): the bounds are
identical on all ranks and the rule's, the shards side by side are the single-rank ingest of the file and the plain rule's matrix bit for
bit, entries_read is the whole file's on every rank, ranks that pass different agree_tags all get ISLE_E_COMM, and one text goes on to
the collective threshold and is held to shard_cases.certify_threshold against the single-rank run.  Each world's worker runs once per
module; a launch that fails fails its tests and ends the launches: nothing more is started on the GPU behind a fault, an abort or a time
limit."""
from functools import partial

import numpy as np
import pytest

import shard_cases as sc
import tdf_shard_cases as tc
import tdf_shard_rule as tr
from rank_launch import launch_each, ranks_of, write_report

pytestmark = pytest.mark.gpu

_FAILED = []  # the first launch of this module that failed: nothing is started behind it


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """world -> its launch, one launch after another"""
    tmp = str(tmp_path_factory.mktemp("tdf_shards"))
    return launch_each([(world, "of %d ranks" % world, partial(tc.launch, world, tmp)) for world in tc.WORLDS], _FAILED)


@pytest.fixture(scope="module", autouse=True)
def report(launches):
    """At the end of the module: the launch times, printed and written to the file ISLE_TDF_SHARD_REPORT names."""
    yield
    lines = ["tdf shard certificate, launch of %d rank%s (%s): %.1f s" % (w, "" if w == 1 else "s", ", ".join(tc.cases_of(w)), l["wall"])
             for w, l in launches.items() if isinstance(l, dict)]
    write_report(lines, "ISLE_TDF_SHARD_REPORT")


@pytest.mark.parametrize("case", list(tr.SHARDED))
def test_shards_side_by_side_are_the_single_rank_ingest(launches, case):
    world, V, D, text = tr.SHARDED[case]
    one = ranks_of(launches, 1)[0]
    single = (one[tc.key(case, "cnt")], one[tc.key(case, "rows")], one[tc.key(case, "offs")])
    ranks = tc.rank_arrays(ranks_of(launches, world), case)
    b = tr.certify_sharded(ranks, text, V, D, single=single)
    assert int(one[tc.key(case, "entries_read")]) == int(ranks[0]["entries_read"])
    if case == "one-document-4":
        assert sum(int(b[r + 1] == b[r]) for r in range(world)) >= 2          # empty windows: matrices of zero columns
    if case == "one-line-no-newline-4":
        assert [int(q["lines_local"]) for q in ranks] == [1, 0, 0, 0]


def test_different_agree_tags_are_a_comm_error_on_every_rank(launches):
    for q in ranks_of(launches, tr.AGREE_WORLD):
        msg = str(q["agree"])
        assert msg.startswith("isle_hip error -5:") and "agree_tag" in msg and "min 1000, max 1003" in msg, msg


def test_a_sharded_ingest_feeds_the_collective_threshold(launches):
    """doc_offset / docs_global of the windowed A reach the collective threshold: the shards' B side by side is the single-rank B"""
    case = tr.THRESHOLD_CASE
    world, V, D, text = tr.SHARDED[case]
    one = ranks_of(launches, 1)[0]
    meta = one[tc.key(case, "th_meta")]
    want = {f: one[tc.key(case, "th_%s" % f)] for f in ("rows", "vals", "offs", "original_cols", "zetas")}
    want.update(D=int(meta[2]), entries_above=int(meta[3]))
    assert want["D"] > 0 and len(want["rows"]) > 0
    ranks = [{"th_%s" % f: q[tc.key(case, "th_%s" % f)] for f in ("rows", "vals", "offs", "original_cols", "zetas", "meta")} for q in ranks_of(launches, world)]
    bnd = ranks_of(launches, world)[0][tc.key(case, "bounds")]
    kept = sc.certify_threshold(want, bnd, ranks, "th")
    assert sum(kept) == want["D"]
