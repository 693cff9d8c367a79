"""isle_amd/host/tdf_file_main run as a real process on the GPU: FPSparseMatrixHip::from_tdf_file (the file streamed in pieces) against
FPSparseMatrixHip::from_tdf of the same file read whole.  The driver exits 0 only if the count matrix, entries_in_A, entries_above_threshold,
avg_doc_sz, original_cols and the shape of B agree in every bit, or if both throw and say the same of the file."""
import os
import re
import subprocess

import pytest

from ingest_cases import CASES
from ingest_rule import KINDS, ingest_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "isle_amd", "host", "tdf_file_main")
TOPICS = 5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    case = next(c for c in CASES if c.id == "passes-2")                  # 5000 lines over 200 x 200, repeated pairs among them
    text = case.build()[0]
    d = tmp_path_factory.mktemp("tdf_file")
    paths = {}
    for name, body in (("good", text), ("no-last-newline", text[:-1]), ("bad", text[:20000] + b"7 x 7\n" + text[20000:]), ("empty", b"")):
        paths[name] = str(d / (name + ".tdf"))
        with open(paths[name], "wb") as f:
            f.write(body)
    return case, paths, ingest_rule(text, case.V, case.D), ingest_rule(text[:20000] + b"7 x 7\n" + text[20000:], case.V, case.D)


def run(path, case, max_entries, piece):
    assert os.path.exists(EXE), "build with make -C isle_amd/csrc"
    return subprocess.run([EXE, path, str(case.V), str(case.D), str(max_entries), str(TOPICS), str(piece)], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name,piece", [("good", 0), ("good", 1000), ("no-last-newline", 4097)])
def test_from_tdf_file_equals_from_tdf(files, name, piece):
    case, paths, want, _ = files
    for max_entries in (0, want[4]):
        r = run(paths[name], case, max_entries, piece)
        assert r.returncode == 0, r.stdout + r.stderr
        assert re.fullmatch(r"identical: entries_in_A %d, above threshold \d+, B \d+ documents, \d+ entries" % len(want[1]), r.stdout.strip())


def test_a_bad_line_is_refused_alike(files):
    case, paths, _, bad = files
    assert bad[0] == "error"
    r = run(paths["bad"], case, 0, 1000)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "both refuse: %s on line %d" % (KINDS[bad[1]], bad[2])


def test_a_max_entries_mismatch_is_refused_alike(files):
    case, paths, want, _ = files
    r = run(paths["good"], case, want[4] + 1, 1000)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "both refuse: file has %d entries, <max_entries> says %d" % (want[4], want[4] + 1)
