"""The free k-means++ draw on document shards (N ranks on one GPU over the host-staged transport, tests/kmpp_shard_cases.py): a plain
split with a seed on either side of the cut, a one-document shard and an empty last shard, and an exhausted corpus whose last seed is
the clamp's document D - 1 at a zero total.  Every rank's seeds, rounds, residual and
C_lowd equal the one-rank fp64 replay of tests/kmpp_certificate.py with `==`, and the ranks' min_dist side by side is the replay's.
One launch per layout, one after another; a launch that fails fails its tests and ends the launches: nothing more is started on the GPU
behind a fault, an abort or a time limit."""
from functools import partial

import pytest

import kmpp_shard_cases as ksc
from rank_launch import launch_each, ranks_of

pytestmark = pytest.mark.gpu

_FAILED = []


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("kmpp_shards"))
    out = launch_each([(layout, layout, partial(ksc.launch, layout, tmp)) for layout in ksc.LAYOUTS], _FAILED)
    print("\n".join("k-means++ shard certificate, launch %s (%d ranks): %.1f s" % (n, ksc.WORLD[n], l["wall"]) for n, l in out.items() if isinstance(l, dict)))
    return out


@pytest.mark.parametrize("name", ksc.NAMES)
@pytest.mark.parametrize("layout", ksc.LAYOUTS)
def test_every_rank_draws_the_one_rank_replay(launches, layout, name):
    ksc.certify(ranks_of(launches, layout), layout, name)
