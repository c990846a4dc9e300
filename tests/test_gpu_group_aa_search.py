"""The protein-database search on a device group (spdp_group_blk_finds, spdp_group_map_align_b): three contexts on ONE card against
one context and against the program's recorded hit lists (tests/golden/aa_search_<set>.json.gz).  Records int for int, hit lists in
the caller's query order with the refused and the hitless queries keeping their empty slots, refusals with the member's message."""
import ctypes as C
import os

import numpy as np
import pytest

from spaln_amd import abi, blocks, engine
from tests import aa_fixture as af
from tests.test_gpu_aa_search import RUNS, Setup, printed_form

pytestmark = pytest.mark.gpu
GROUP_RUNS = ("default", "M4", "M4_pw", "LS_M2_pw")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def grp():
    g = engine.Group([0, 0, 0])
    yield g
    g.close()


class GroupSetup(Setup):
    """a run's set-up on one context, and the same index once per member of the group"""

    def __init__(self, eng, grp, tmp, name, max_out, local, qck):
        Setup.__init__(self, eng, tmp, name, max_out, local, qck)
        arrays, _ = blocks.read_protein_db_index(eng.lib, af.bka_path(name, tmp), max_out=max_out, local=local)
        self.gix = blocks.GroupIndex(grp, arrays)

    def free(self):
        self.gix.free()
        Setup.free(self)


def plain(lists):
    return [[{k: (v.tolist() if k == "corners" else v) for k, v in h.items()} for h in lst] for lst in lists]


@pytest.mark.parametrize("name,run", [(n, r) for n in af.SETS for r in GROUP_RUNS])
def test_records_and_hit_lists_equal_one_context_and_the_program(eng, grp, tmp_path, name, run):
    max_out, local, qck, all_out = RUNS[run]
    s = GroupSetup(eng, grp, str(tmp_path), name, max_out, local, qck)
    try:
        cap = 6 + 2 * (max_out + 10) + 1 + max_out
        want_rec, _ = blocks.finds(s.dix, s.fprm, s.queries, out_cap=cap)
        got_rec, ms = blocks.group_finds(s.gix, s.fprm, s.queries, out_cap=cap)
        served_finds = set(grp.shards(len(s.queries)).tolist())
        want, _ = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries, all_out=bool(all_out))
        got, sec = blocks.group_map_align_b(s.gix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries, all_out=bool(all_out))
        member = grp.shards(len(s.queries))
        stats = [blocks.finds_stats(grp.context(r)) for r in range(3)]
    finally:
        s.free()
    assert got_rec.shape == want_rec.shape and np.array_equal(got_rec, want_rec) and ms > 0
    assert served_finds == {0, 1, 2} and set(member.tolist()) == {0, 1, 2}
    assert plain(got) == plain(want)
    # the program's lists, and the slots that must stay empty
    rec = s.doc["runs"][run]["o4"]
    for q, hits in zip(s.doc["queries"], got):
        assert printed_form(s, hits) == [dict(b=r["b"], val=r["val"], corners=r["corners"]) for r in rec.get(q["name"], [])], (name, run, q["name"])
    refused = [i for i, q in enumerate(s.doc["queries"]) if q["name"] in s.doc["refused"]]
    hitless = [i for i, q in enumerate(s.doc["queries"]) if not rec.get(q["name"]) and q["name"] not in s.doc["refused"]]
    assert refused and all(got[i] == [] for i in refused)
    if run == "default":
        assert hitless, name                            # a searched query without a printed hit, between queries with hits
    assert all(got[i] == [] for i in hitless)
    assert got[0] and got[-1] and sum(1 for lst in got if lst) > len(refused + hitless)     # the empty slots lie between queries with hits
    # the counters stay per context: the members' add up to the call's
    assert sum(st["refused_short"] for st in stats) == len(refused) and sum(st["searched"] for st in stats) == len(s.queries) - len(refused)
    assert sec[3] >= max(sec[:3]) > 0                   # the call is the group's wall time, a phase its slowest member's


def test_refusals_go_through_the_group(eng, grp, tmp_path):
    s = GroupSetup(eng, grp, str(tmp_path), "b", 1, 0, 3)
    nix = None
    try:
        # a nucleotide index: every member refuses, the group says which device and what
        nix = blocks.GroupIndex(grp, blocks.read_index_file(eng.lib, os.path.join(af.GOLDEN, "blk_k3.bkn")))
        with pytest.raises(RuntimeError) as e:
            blocks.group_finds(nix, s.fprm, s.queries[:4])
        assert "device 0: spdp_blk_finds: a nucleotide index" in str(e.value)
        # a query of 65 536 residues: its member refuses, the others have answered; nothing is handed out
        queries = s.queries[:5] + [np.full(65536, 3, dtype=np.uint8)]
        with pytest.raises(RuntimeError) as e:
            blocks.group_map_align_b(s.gix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, queries)
        assert "longer than 65535" in str(e.value) and "device 0: " in str(e.value)
        codes, offs = blocks._packed(queries)
        g = blocks.Genome(s.db_codes.ctypes.data, s.db_off.ctypes.data, len(s.db_off) - 1)
        hit_off = np.full(len(queries) + 1, -1, dtype=np.int64)
        hits, corners = C.POINTER(abi.MapHitB)(), C.POINTER(C.c_int32)()
        lib = grp.lib
        lib.spdp_group_map_align_b.argtypes = [C.c_void_p] * 10 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4
        rc = lib.spdp_group_map_align_b(grp.h, s.gix.h, C.byref(s.gix.desc), C.byref(g), C.byref(s.sc), C.byref(s.up), C.byref(s.sp), C.byref(s.fprm),
                                        codes.ctypes.data, offs.ctypes.data, len(queries), 0, hit_off.ctypes.data, C.byref(hits), C.byref(corners), None)
        assert rc == -1 and not hits and not corners
        assert b"longer than 65535" in lib.spdp_group_last_error(grp.h)
        # the same call without the long query is served
        got, _ = blocks.group_map_align_b(s.gix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, queries[:5])
        want, _ = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, queries[:5])
        assert plain(got) == plain(want)
        # no query at all: the first member answers as a context does
        assert blocks.group_map_align_b(s.gix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, [])[0] == []
    finally:
        if nix is not None:
            nix.free()
        s.free()
