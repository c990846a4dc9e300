"""The rule that orders the searches of a query whose parts lie in different places (`spaln -pr`): spdp_dispersed_rests, the
library's statement of quick4 (src/spaln.cc:1114-1134), against a table written from those lines.  After the first search left
the query's range org at cov, [org.left, cov.left) is searched again if cov.left - org.left > MinSegLen and [cov.right, org.right)
if org.right - cov.right > MinSegLen -- both strictly, the left rest first.  Host code: no device."""
import ctypes as C
import os

import pytest

from spaln_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M = 21          # a MinSegLen (2 Ktuple + Nshift of a nucleotide index with Ktuple 8, Nshift 5; the rule takes any positive value)

# (org, cov, min_seg_len) -> the rests, left first
TABLE = [
    # the covered range equals the query's: nothing is left over
    (((0, 1000), (0, 1000), M), []),
    # both ends short of the bound
    (((0, 1000), (10, 990), M), []),
    # the strict inequality on the left: a rest of exactly MinSegLen is not searched, one of MinSegLen + 1 is
    (((0, 1000), (M, 1000), M), []),
    (((0, 1000), (M + 1, 1000), M), [(0, M + 1)]),
    # ... and on the right
    (((0, 1000), (0, 1000 - M), M), []),
    (((0, 1000), (0, 1000 - M - 1), M), [(1000 - M - 1, 1000)]),
    # left only, right only, both (left first)
    (((0, 2665), (505, 2665), M), [(0, 505)]),
    (((0, 2665), (0, 2001), M), [(2001, 2665)]),
    (((0, 3000), (700, 2100), M), [(0, 700), (2100, 3000)]),
    # both at their bounds: one passes, one does not
    (((0, 1000), (M + 1, 1000 - M), M), [(0, M + 1)]),
    (((0, 1000), (M, 1000 - M - 1), M), [(1000 - M - 1, 1000)]),
    # a query whose own range does not begin at 0 (a trimmed tail, a clipped head): the rests are taken from org, not from the ends
    (((30, 970), (30 + M + 1, 970 - M - 1), M), [(30, 30 + M + 1), (970 - M - 1, 970)]),
    (((30, 970), (30 + M, 970 - M), M), []),
    # another bound
    (((0, 500), (100, 400), 100), []),
    (((0, 500), (101, 399), 100), [(0, 101), (399, 500)]),
]


@pytest.fixture(scope="module")
def lib():
    return engine.load_library()


@pytest.mark.parametrize("case,want", TABLE, ids=[f"{c[0]}-{c[1]}-{c[2]}".replace(" ", "") for c, _ in TABLE])
def test_rests_follow_quick4(lib, case, want):
    org, cov, msl = case
    assert engine.dispersed_rests(lib, org, cov, msl) == want


def test_unwritten_slots_stay_and_null_is_refused(lib):
    org, cov = (C.c_int32 * 2)(0, 1000), (C.c_int32 * 2)(0, 900)
    rests = (C.c_int32 * 4)(-7, -7, -7, -7)
    assert lib.spdp_dispersed_rests(org, cov, M, rests) == 1
    assert list(rests) == [900, 1000, -7, -7]
    assert lib.spdp_dispersed_rests(None, cov, M, rests) == -1
    assert lib.spdp_dispersed_rests(org, cov, M, None) == -1


def test_the_entries_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "spdp.h")).read()
    for name in ("spdp_dispersed_rests", "spdp_map_align_s_dispersed", "spdp_map_align_h_dispersed"):
        assert hasattr(lib, name), name
        assert name in engine.EXPORTS
        assert name + "(" in header
