"""tests/rank_launch.py without a GPU: every child is python -c with a few lines of stub text."""
import os
import sys
import time

import pytest

import rank_launch as rl

HEAD = "import os, sys, time; rank, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]\n"
PID = "with open(out[:-4] + '.pid', 'w') as f: f.write(str(os.getpid()))\n"  # <stem>_r<rank>.pid


def stub(text):
    return lambda rank, port, out: [sys.executable, "-c", HEAD + text, str(rank), str(port), out]


def assert_no_child_is_left(tmp, stem, world):
    for r in range(world):
        with open(os.path.join(tmp, "%s_r%d.pid" % (stem, r))) as f:
            pid = int(f.read())
        with pytest.raises(ProcessLookupError):  # ended and waited for: the pid names no process of ours any more
            os.kill(pid, 0)


def test_a_clean_launch_returns_the_ranks_in_order(tmp_path):
    l = rl.launch("clean", "c", 3, str(tmp_path), stub("import numpy as np; print('rank %d here' % rank); np.savez(out, rank=rank, port=port)"))
    assert [int(q["rank"]) for q in l["ranks"]] == [0, 1, 2]
    assert len({int(q["port"]) for q in l["ranks"]}) == 1
    assert all("rank %d here" % r in l["outputs"][r] for r in range(3)) and len(l["outputs"]) == 3
    assert l["wall"] > 0
    assert sorted(os.listdir(str(tmp_path))) == sorted("c_r%d.%s" % (r, e) for r in range(3) for e in ("log", "npz"))


def test_a_rank_that_fails_ends_the_others_at_once(tmp_path):
    text = PID + ("if rank == 1:\n"  # it fails once the others are known to run
                  "    while not all(os.path.exists(out[:-5] + '%d.pid' % r) for r in (0, 2)): time.sleep(0.01)\n"
                  "    print('rank one gives up'); sys.exit(3)\n"
                  "time.sleep(30)")
    t0 = time.monotonic()
    with pytest.raises(rl.LaunchFailed) as e:
        rl.launch("the label", "f", 3, str(tmp_path), stub(text), timeout=20)
    assert time.monotonic() - t0 < 20
    msg = str(e.value)
    assert msg.startswith("the label: rank 1 ended with status 3\n") and "--- rank 1\nrank one gives up" in msg and "time limit" not in msg
    assert_no_child_is_left(str(tmp_path), "f", 3)


def test_the_time_limit_is_the_launch_s_and_ends_every_rank(tmp_path):
    t0 = time.monotonic()
    with pytest.raises(rl.LaunchFailed, match="slow: time limit of 1 s"):
        rl.launch("slow", "t", 2, str(tmp_path), stub(PID + "time.sleep(30)"), timeout=1)
    assert 1 <= time.monotonic() - t0 < 20
    assert_no_child_is_left(str(tmp_path), "t", 2)


def test_the_environment_reaches_the_ranks_and_the_world_is_at_most_four(tmp_path):
    l = rl.launch("env", "e", 1, str(tmp_path), stub("import numpy as np; np.savez(out, v=os.environ['RANK_LAUNCH_TEST'])"), env={"RANK_LAUNCH_TEST": "set"})
    assert str(l["ranks"][0]["v"]) == "set" and "RANK_LAUNCH_TEST" not in os.environ
    for world in (0, 5):
        with pytest.raises(AssertionError):
            rl.launch("wide", "w", world, str(tmp_path), stub(""))
    assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("w_")]  # refused before anything was started


def test_launch_each_starts_nothing_behind_a_failure():
    calls, failed = [], []

    def thunk(name, fails):
        def run():
            calls.append(name)
            if fails:
                raise rl.LaunchFailed("%s: rank 0 ended with status 1" % name)
            return dict(ranks=[{"name": name}])
        return run

    out = rl.launch_each([("a", "first", thunk("first", False)), ("b", "second", thunk("second", True)), ("c", "third", thunk("third", False))], failed)
    assert calls == ["first", "second"] and failed == ["second"]
    assert list(out) == ["a", "b", "c"] and out["a"] == dict(ranks=[{"name": "first"}])
    assert isinstance(out["b"], rl.LaunchFailed) and str(out["b"]).startswith("second: rank 0")
    assert isinstance(out["c"], rl.LaunchFailed) and str(out["c"]) == "not started: the launch second failed"
    # the list is the module's: a second fixture that shares it starts nothing either
    again = rl.launch_each([("d", "fourth", thunk("fourth", False))], failed)
    assert calls == ["first", "second"] and str(again["d"]) == "not started: the launch second failed"


def test_ranks_of_turns_a_stored_failure_into_a_test_failure():
    launches = {"good": dict(ranks=[1, 2]), "bad": rl.LaunchFailed("docs H2: rank 1 ended with status -6\n--- rank 1\nabort")}
    assert rl.ranks_of(launches, "good") == [1, 2]
    with pytest.raises(pytest.fail.Exception) as e:
        rl.ranks_of(launches, "bad")
    assert "docs H2: rank 1 ended with status -6" in str(e.value) and "abort" in str(e.value)


def test_write_report(tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("RANK_LAUNCH_REPORT", raising=False)
    rl.write_report(["one", "two"], "RANK_LAUNCH_REPORT")
    assert capsys.readouterr().out == "one\ntwo\n"
    monkeypatch.setenv("RANK_LAUNCH_REPORT", str(tmp_path / "report.txt"))
    rl.write_report(["one", "two"], "RANK_LAUNCH_REPORT")
    assert (tmp_path / "report.txt").read_text() == "one\ntwo\n" and capsys.readouterr().out == "one\ntwo\n"


def test_module_command_calls_the_module_s_worker_main_with_strings(tmp_path):
    mods = tmp_path / "mods"
    mods.mkdir()
    (mods / "stub_rank_module.py").write_text(
        "import sys, numpy as np\n"
        "def worker_main(*a):\n"
        "    assert all(isinstance(x, str) for x in a)\n"
        "    np.savez(a[2], args=np.array(a), paths=np.array(sys.path[:2]))\n")
    path = os.pathsep.join([str(mods)] + [p for p in [os.environ.get("PYTHONPATH")] if p])
    l = rl.launch("module", "m", 2, str(tmp_path), rl.module_command("stub_rank_module", "H2", 7), env={"PYTHONPATH": path})
    for r, q in enumerate(l["ranks"]):
        rank, port, out, layout, seven = [str(x) for x in q["args"]]
        assert (rank, out, layout, seven) == (str(r), str(tmp_path / ("m_r%d.npz" % r)), "H2", "7") and int(port) > 0
        assert [str(p) for p in q["paths"]] == [os.path.join(rl.ROOT, "tests"), rl.ROOT]  # the repository's tests/ and root come first
