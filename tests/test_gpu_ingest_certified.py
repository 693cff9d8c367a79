"""ingest.hip, its radix sort and the scans under it against the plain rule of tests/ingest_rule.py, on the case table of
tests/ingest_cases.py: newline geometry at the 16-byte chunk and the 4096-byte tile, line counts around the 256-line blocks and past the
scan's 1,048,576-input carry, every number of sort passes from 1 to 8, sort sizes around the wave, the flag block and the 2048-key tile,
repeated pairs whose counts tell the file order, offsets with empty runs, the edges of the id and count ranges, every kind of error with
its line.  Every comparison is exact: counts, rows, offsets, entries_read, nnz; an error by its kind's wording and its 1-based line.
test_ingest_rule_cpu.py holds the host parser to the same table without a GPU.  profiles/ingest_certificate.md holds a measured run."""
import re

import numpy as np
import pytest

from ingest_cases import CASES
from ingest_rule import KINDS, ingest_rule
from isle_amd import IsleHipError

pytestmark = pytest.mark.gpu


def assert_exact(hp, info, want):
    _, counts, rows, offs, entries_read = want
    assert info["entries_read"] == entries_read and info["nnz"] == len(counts)
    gc, gr, go = hp.get_A()
    np.testing.assert_array_equal(go, offs)
    np.testing.assert_array_equal(gr, rows)
    np.testing.assert_array_equal(gc, counts)


def assert_rejected(hp, text, V, D, kind, line):
    with pytest.raises(IsleHipError, match=re.escape("%s on line %d" % (KINDS[kind], line)) + r"\b"):
        hp.ingest_tdf(text, V, D)
    with pytest.raises(IsleHipError, match="no count matrix"):
        hp.get_A()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_ingest_equals_the_rule(hp, case):
    text, arrays = case.build()
    want = case.expected(text, arrays)
    if want[0] == "error":
        hp.ingest_tdf(b"1 1 1\n", 1, 1)                # get_A needs a shape to ask with: the failure below must void this matrix
        assert_rejected(hp, text, case.V, case.D, want[1], want[2])
        return
    info = hp.ingest_tdf(text, case.V, case.D, max_entries=want[4])
    assert_exact(hp, info, want)
    if not len(text.strip()):
        assert info["nnz"] == 0 and not hp.get_A()[2].any() and len(hp.get_A()[2]) == case.D + 1


def test_a_failed_ingest_leaves_no_matrix_and_the_next_one_is_exact(hp):
    good = b"2 3 4\n1 1 9\n2 3 5\n\n4 4 1"
    hp.ingest_tdf(good, 5, 5)
    assert_rejected(hp, b"1 1 1\n2 2 0\n", 5, 5, 5, 2)
    assert_exact(hp, hp.ingest_tdf(good, 5, 5, max_entries=4), ingest_rule(good, 5, 5))


def test_a_small_matrix_after_a_large_one_has_no_stale_tail(hp):
    big = next(c for c in CASES if c.id == "passes-2")
    text, arrays = big.build()
    assert_exact(hp, hp.ingest_tdf(text, big.V, big.D), big.expected(text, arrays))
    small = b"200 200 7\n3 1 2\n3 1 9\n1 2 3\n"
    info = hp.ingest_tdf(small, big.V, big.D)
    assert info == dict(entries_read=4, nnz=3)
    assert_exact(hp, info, ingest_rule(small, big.V, big.D))
