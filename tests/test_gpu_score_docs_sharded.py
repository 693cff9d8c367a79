"""isle_hip_score_docs on document shards: 2 and 3 ranks on one GPU over the host-staged transport (tests/rank_launch.py), uneven shards and,
with 3 ranks, an empty one.  There is no collective in the call: every rank uploads its documents, infers their weights under the caller's
model and scores its own rows, the resident entries and a held-out part split with the shard's doc_offset.  The ranks' arrays side by side
equal the arrays of the same steps on one rank without a communicator (the session's context) bit for bit, in every mode of
tests/score_rule.py, and isle_hip_score_total of the concatenation is the single-rank total.  model="avg" is refused on every rank."""
import numpy as np
import pytest

import rank_launch
import score_rule as sr
from isle_amd import IsleHipError, hot_path

pytestmark = pytest.mark.gpu
_FAILED = []
V, D, K, SEED = 500, 700, 5, 3
CUTS = {2: (0, 250, 700), 3: (0, 250, 250, 700)}
KEYS = ("score", "tokens", "unscored_tokens", "unscored_entries", "floored")
MEASURE = {sr.LOG: "log", sr.PROB: "prob"}
HELD = (9, 1, 3)  # seed, num, den


def steps(hp, m, cnt, word, off, doc_offset, docs_global, res):
    """what every rank does with its documents, and the session's context with all of them"""
    hp.upload_counts(V, cnt, word, off, doc_offset, docs_global)
    inf = hp.infer_resident(m, min_weight=0.0)
    res["nentries"] = np.array(inf["nentries"])
    _, held = hot_path.split_held_out(cnt, word, off, *HELD, doc_offset=doc_offset)
    res["held.word"], res["held.len"] = held[1], np.diff(held[2])
    for i, mode in enumerate(sr.MODES):
        kw = dict(measure=MEASURE[mode[0]], normalise=bool(mode[1]), floor=mode[2])
        for name, got in (("resident", hp.score_docs(m, "infer", "resident", **kw)), ("held", hp.score_docs(m, "infer", held, **kw))):
            for key in KEYS:
                res["%s.%d.%s" % (name, i, key)] = got[key]
            res["%s.%d.total" % (name, i)] = np.array([got["total_score"], got["total_tokens"]])


def _worker(hp, rank, world, res):
    m, cnt, word, off = sr.planted(V, D, K, SEED)
    b, e = CUTS[world][rank], CUTS[world][rank + 1]
    sl = slice(int(off[b]), int(off[e]))
    steps(hp, m, cnt[sl], word[sl], off[b:e + 1] - off[b], b, D, res)
    try:
        hp.score_docs("avg", "infer", "resident")
        res["avg"] = np.array("accepted")
    except (IsleHipError, KeyError, ValueError) as err:
        res["avg"] = np.array(str(err))


def worker_main(rank, port, out, world):
    rank_launch.run_rank(int(world), int(rank), int(port), out, _worker)


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("score_docs_ranks"))
    jobs = [(w, "W%d" % w, (lambda w=w: rank_launch.launch("score docs W%d" % w, "score_W%d" % w, w, tmp,
                                                          rank_launch.module_command("test_gpu_score_docs_sharded", w)))) for w in sorted(CUTS)]
    return rank_launch.launch_each(jobs, _FAILED)


@pytest.fixture(scope="module")
def single(hp):
    m, cnt, word, off = sr.planted(V, D, K, SEED)
    res = {}
    steps(hp, m, cnt, word, off, 0, 0, res)
    assert int(res["nentries"]) > 1000 and res["held.word"].size > 1000
    return res


@pytest.mark.parametrize("world", sorted(CUTS))
def test_the_ranks_arrays_side_by_side_are_the_single_rank_arrays(launches, single, world):
    ranks = rank_launch.ranks_of(launches, world)
    assert len(ranks) == world and [r["resident.0.score"].size for r in ranks] == np.diff(CUTS[world]).tolist()
    assert sum(int(r["nentries"]) for r in ranks) == int(single["nentries"])
    for key in ("held.word", "held.len"):  # the split does not depend on the shards
        assert np.concatenate([r[key] for r in ranks]).tobytes() == single[key].tobytes(), key
    for name in ("resident", "held"):
        for i, mode in enumerate(sr.MODES):
            side = {key: np.concatenate([r["%s.%d.%s" % (name, i, key)] for r in ranks]) for key in KEYS}
            for key in KEYS:
                assert side[key].dtype == single["%s.%d.%s" % (name, i, key)].dtype and side[key].tobytes() == single["%s.%d.%s" % (name, i, key)].tobytes(), \
                    (name, mode, key)
            total = np.array([hot_path.score_total(side["score"]), hot_path.score_total(side["tokens"])])
            assert total.tobytes() == single["%s.%d.total" % (name, i)].tobytes(), (name, mode, "total")
            for r, res in enumerate(ranks):  # a rank's own totals are those of its rows
                own = np.array([hot_path.score_total(res["%s.%d.score" % (name, i)]), hot_path.score_total(res["%s.%d.tokens" % (name, i)])])
                assert own.tobytes() == res["%s.%d.total" % (name, i)].tobytes(), (name, mode, r)


@pytest.mark.parametrize("world", sorted(CUTS))
def test_the_average_model_is_refused_on_every_rank(launches, world):
    for res in rank_launch.ranks_of(launches, world):
        assert "accepted" not in str(res["avg"]) and ("single-rank only" in str(res["avg"]) or "no average model" in str(res["avg"])), str(res["avg"])
