"""route_host.h route_objective_acc / route_objective_lds_bytes, the one rule of the k-means objective that chooses a kernel form (the
exact accumulation privatised in LDS, or global atomics), without the library and without a GPU: isle_amd/host/route_host_main.cpp built
with the address and undefined-behaviour sanitizers answers a script.  The answers are stated here: 3 k 64-bit words in LDS while they fit
in 24 KB, none beyond.  The sizes the GPU tests use lie on the LDS side; 1024 | 1025 is the edge."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("objective_route") / "route_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "route_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def test_lds_up_to_1024_centres_global_atomics_beyond(exe):
    ks = [1, 5, 65, 300, 1000, 1023, 1024, 1025, 2048, 8192]
    r = subprocess.run([exe], input="".join("objective %d\n" % k for k in ks), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert [(o["cmd"], o["lds"], o["lds_bytes"]) for o in out] == [("objective", int(k <= 1024), 24 * k if k <= 1024 else 0) for k in ks]
    assert max(o["lds_bytes"] for o in out) == 24 * 1024  # under the 64 KB a workgroup gets without asking
