"""CPU checks of the query preparation (include/spdp.h "query preparation"; PolyA::rmpolyA of the reference): the new entries are
exported and declared, their two records have the sizes the header gives them, and spdp_polya_scan_host -- the sequential rule
the device entries are held to -- agrees with the restatement in tests/polya_cases.py on its whole set of queries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spaln_amd import blocks, engine
from tests import polya_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("spdp_polya_scan_host", "spdp_polya_scan", "spdp_polya_scan_resident", "spdp_map_align_s_prep", "spdp_map_align_s_multi_prep")


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "spdp.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", txt)
    assert m, name
    return [a.strip() for a in " ".join(m.group(1).split()).split(",")]


def test_new_entries_are_exported_and_declared():
    lib = C.CDLL(engine.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        _declaration(name)
    for f in ("polya_scan", "polya_scan_host", "map_align_prep", "map_align_multi_prep"):
        assert callable(getattr(blocks, f))


def test_prep_argument_lists():
    """the arguments of spdp_map_align_s / _multi with `const SpdpQueryPrep* prep` in the place of ori, and the records last"""
    for name, base in (("spdp_map_align_s_prep", "spdp_map_align_s"), ("spdp_map_align_s_multi_prep", "spdp_map_align_s_multi")):
        new, old = _declaration(name), _declaration(base)
        assert new[:-1] == [("const SpdpQueryPrep* prep" if a == "int32_t ori" else a) for a in old], name
        assert new[-1] == "SpdpQueryTail* tails", name


def test_records_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spdp.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(SpdpQueryPrep), sizeof(SpdpQueryTail), offsetof(SpdpQueryPrep, polya_thr),'
                   'offsetof(SpdpQueryTail, ori), offsetof(SpdpQueryTail, reserved));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [8, 32, 4, 16, 20]
    assert got == [C.sizeof(blocks.QueryPrep), C.sizeof(blocks.QueryTail), blocks.QueryPrep.polya_thr.offset, blocks.QueryTail.ori.offset,
                   blocks.QueryTail.reserved.offset]


def test_the_set_holds_what_it_is_meant_to():
    """about 5 000 queries, every length of the list, and under the default parameters every outcome"""
    qs = polya_cases.queries()
    assert 4500 <= len(qs) <= 6000
    assert set(polya_cases.LENGTHS) <= {len(q) for q in qs}
    pols = [polya_cases.rule(q, 3, 12)[0][0] for q in qs]
    assert min(pols.count(p) for p in (0, 1, 2)) >= 200
    all_a = polya_cases.rule(np.full(200, polya_cases.A, np.uint8), 3, 12)[0]
    assert all_a == (1, 0, 0, 0, 3)                                 # (all A: nothing of the transcript is left)


@pytest.mark.parametrize("q_mns,thr", polya_cases.PARAMS)
@pytest.mark.parametrize("lead", [0, 3])
def test_host_scan_equals_the_rule(q_mns, thr, lead):
    lib = C.CDLL(engine.LIB_PATH)
    qs = polya_cases.queries()
    rec, norm = blocks.polya_scan_host(lib, qs, q_mns, thr, lead=lead)
    assert rec.shape == (len(qs), 5)
    n_turned = 0
    for i, q in enumerate(qs):
        want, wq = polya_cases.rule(q, q_mns, thr)
        assert tuple(int(x) for x in rec[i]) == want, (i, len(q), q[:40], q[-40:])
        # the codes: the reverse complement exactly where pol == 2, as they came otherwise
        assert np.array_equal(norm[i], wq), i
        assert want[0] == 2 or np.array_equal(norm[i], q)
        n_turned += want[0] == 2
    assert (n_turned > 0) == (q_mns == 3 and thr > 0)


def test_host_scan_in_place_and_without_codes_out():
    lib = C.CDLL(engine.LIB_PATH)
    qs = polya_cases.queries()[:600]
    codes, offs = blocks._packed(qs)
    prep = blocks.QueryPrep(3, 12)
    lib.spdp_polya_scan_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    t0, t1 = (blocks.QueryTail * len(qs))(), (blocks.QueryTail * len(qs))()
    assert lib.spdp_polya_scan_host(codes.ctypes.data, offs.ctypes.data, len(qs), C.byref(prep), t0, None) == 0
    work = codes.copy()
    assert lib.spdp_polya_scan_host(work.ctypes.data, offs.ctypes.data, len(qs), C.byref(prep), t1, work.ctypes.data) == 0
    assert bytes(t0) == bytes(t1)
    for i, q in enumerate(qs):
        assert np.array_equal(work[offs[i]:offs[i + 1]], polya_cases.rule(q, 3, 12)[1]), i


def test_refusals():
    """q_mns = 2 (and anything but 1 and 3) and a missing preparation are refused: by the host entry with -1, by the entries that
    have a context with a message.  The context-bound entries refuse before they touch the device."""
    lib = C.CDLL(engine.LIB_PATH)
    q = np.full(40, polya_cases.A, np.uint8)
    offs = np.array([0, 40], dtype=np.int64)
    t = (blocks.QueryTail * 1)()
    lib.spdp_polya_scan_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    for bad in (2, 0, 4, -1):
        assert lib.spdp_polya_scan_host(q.ctypes.data, offs.ctypes.data, 1, C.byref(blocks.QueryPrep(bad, 12)), t, None) == -1, bad
    assert lib.spdp_polya_scan_host(q.ctypes.data, offs.ctypes.data, 1, None, t, None) == -1
    assert lib.spdp_polya_scan_host(q.ctypes.data, offs.ctypes.data, 1, C.byref(blocks.QueryPrep(1, 12)), t, None) == 0
    # a null context: nothing to leave a message in
    lib.spdp_map_align_s_prep.argtypes = [C.c_void_p] * 11 + [C.c_int32] + [C.c_void_p] * 5
    assert lib.spdp_map_align_s_prep(*([None] * 11), 0, *([None] * 5)) == -1
