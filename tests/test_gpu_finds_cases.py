"""The vote of SrchBlk::finds on the device (spdp_blk_finds, spaln_amd/csrc/spdp_blk_finds.hip) against the restatement
(tests/finds_restate.py, itself held to the program by tests/test_finds_restate.py): every recipe of tests/finds_cases.py and
every query of the program's fixtures, every int of every record -- flags, nmmc, testword, sigm, the heap in order, the
candidates.  No record may come back with SPDP_BLK_TABLE or SPDP_BLK_CUT but in the recipe that plants an out_cap too small."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from spaln_amd import abi, blocks, engine
from tests import aa_fixture as af
from tests import finds_cases as fc
from tests import finds_restate as fr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def library_arrays(fx: dict) -> dict:
    """a recipe's index in the layout blocks.BlockIndex takes (a reference-side dump's)"""
    out = dict(fx)
    prm = np.zeros(42, dtype=np.int32)
    for name, pos in blocks._PRM.items():
        prm[pos] = int(fx[name])
    prm[36] = struct.unpack("<i", struct.pack("<f", fx["rbscoef"]))[0]
    prm[37] = struct.unpack("<i", struct.pack("<f", fx["rbscons"]))[0]
    out["blk_prm"] = prm
    out["blk_pb2c"] = np.frombuffer(np.array([fx["bclw"], fx["bcup"], fx["bcce"]], dtype=np.float64).tobytes(), dtype=np.uint8).copy()
    out["blk_cfact"] = np.frombuffer(np.array([fx["cfact"]], dtype=np.float64).tobytes(), dtype=np.uint8).copy()
    return out


def params_of(fx: dict) -> abi.BlkFindsParams:
    p = abi.BlkFindsParams()
    p.max_out, p.local, p.rln_coef, p.ptpl, p.avrscr = int(fx["max_out"]), int(fx["local"]), float(fx["rlncoef"]), int(fx["ptpl"]), int(fx["avrscr"])
    return p


def same_records(got: np.ndarray, want: list, what):
    assert got.shape[0] == len(want)
    for k, w in enumerate(want):
        g = got[k]
        assert int(g[0]) == len(w) and g[:len(w)].tolist() == w, (what, k, g[:max(int(g[0]), 6)].tolist(), w)


@pytest.mark.parametrize("name", fc.names())
def test_every_recipe_equals_the_restatement(eng, name):
    rcp = fc.recipes()[name]
    dix = blocks.BlockIndex(eng, library_arrays(rcp["fx"]))
    try:
        got, ms = blocks.finds(dix, params_of(rcp["fx"]), [q for q, _, _ in rcp["queries"]], ranges=[(l, r) for _, l, r in rcp["queries"]],
                               out_cap=rcp["out_cap"])
    finally:
        dix.free()
    same_records(got, [fc.wanted_record(x, rcp["out_cap"]) for x in fc.wanted(name)], name)
    assert ms > 0
    flagged = [k for k in range(got.shape[0]) if got[k, 2] & (fr.TABLE | fr.CUT)]
    assert flagged == (list(range(got.shape[0])) if name == "cut" else []), (name, flagged)


@pytest.mark.parametrize("name", ["phase_ns3", "family_m4", "ties_m2", "geometry_bp5", "zeros_bp5"])
def test_the_run_hash_in_the_slab_gives_the_same_records(eng, name, monkeypatch):
    """SPDP_FINDS_HH_LDS=0: the small tables of the recipes, which live in LDS otherwise, in the wave's slab of HBM"""
    monkeypatch.setenv("SPDP_FINDS_HH_LDS", "0")
    rcp = fc.recipes()[name]
    assert rcp["fx"]["hh_size"] * 8 <= 24 << 10
    dix = blocks.BlockIndex(eng, library_arrays(rcp["fx"]))
    try:
        got, _ = blocks.finds(dix, params_of(rcp["fx"]), [q for q, _, _ in rcp["queries"]], ranges=[(l, r) for _, l, r in rcp["queries"]],
                              out_cap=rcp["out_cap"])
    finally:
        dix.free()
    same_records(got, [fc.wanted_record(x, rcp["out_cap"]) for x in fc.wanted(name)], name)


@pytest.fixture(scope="module")
def mixed(eng):
    """queries of two recipes on one index, refused ones among them, and what the restatement says of each"""
    rcp, edge = fc.recipes()["phase_ns3"], fc.recipes()["edge_ns3"]
    qs = rcp["queries"] + edge["queries"]
    want = [fc.wanted_record(x, 64) for x in fc.wanted("phase_ns3") + fc.wanted("edge_ns3")]
    assert any(w[2] & fr.SHORT for w in want)
    dix = blocks.BlockIndex(eng, library_arrays(rcp["fx"]))
    yield dix, params_of(rcp["fx"]), qs, want
    dix.free()


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_batches_and_their_reversal(mixed, n):
    dix, prm, qs, want = mixed
    pick = [(7 * k + 3) % len(qs) for k in range(n)]
    for order in (pick, pick[::-1]):
        got, _ = blocks.finds(dix, prm, [qs[i][0] for i in order], ranges=[qs[i][1:] for i in order])
        same_records(got, [want[i] for i in order], (n, order is pick))
    if n > 1:
        assert any(want[i][2] & fr.SHORT for i in pick)


def test_resident_equals_the_copying_entry(mixed):
    dix, prm, qs, want = mixed
    a, _ = blocks.finds(dix, prm, [q for q, _, _ in qs], ranges=[(l, r) for _, l, r in qs])
    b, ms = blocks.finds(dix, prm, [q for q, _, _ in qs], ranges=[(l, r) for _, l, r in qs], resident=True)
    assert np.array_equal(a, b) and ms > 0
    same_records(b, want, "resident")


def test_refusals_by_name(eng, mixed, tmp_path):
    dix, prm, qs, _ = mixed
    q = [qs[0][0]]

    def refused(index, p, **kw):
        with pytest.raises(RuntimeError) as e:
            blocks.finds(index, p, q, **kw)
        return str(e.value)
    other = params_of(fc.recipes()["phase_ns3"]["fx"])
    other.max_out = 3
    assert "Ncand != MaxOut + 10" in refused(dix, other)
    assert "out_cap < 6" in refused(dix, prm, out_cap=5)
    gdb = dict(fc.recipes()["phase_ns3"]["fx"], gdb=1)
    gix = blocks.BlockIndex(eng, library_arrays(gdb))
    try:
        assert "genomic database" in refused(gix, prm)
    finally:
        gix.free()
    nix = blocks.BlockIndex(eng, blocks.read_index_file(eng.lib, os.path.join(HERE, "golden", "blk_k3.bkn")))
    try:
        assert "nucleotide index" in refused(nix, prm)
    finally:
        nix.free()
    lib = eng.lib
    lib.spdp_blk_finds.restype = C.c_int
    lib.spdp_blk_finds.argtypes = [C.c_void_p] * 8 + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    out = np.zeros(64, dtype=np.int32)
    assert lib.spdp_blk_finds(eng.ctx, dix.h, C.byref(dix.desc), C.byref(prm), None, None, None, None, 1, out.ctypes.data, 64, None) == -1
    assert b"null argument" in lib.spdp_last_error(eng.ctx)
    assert lib.spdp_blk_finds(eng.ctx, dix.h, C.byref(dix.desc), None, None, None, None, None, 1, out.ctypes.data, 64, None) == -1
    assert b"null argument" in lib.spdp_last_error(eng.ctx)
    left, right, offs = np.array([0], np.int32), np.array([len(q[0]) + 1], np.int32), np.array([0, len(q[0])], np.int64)
    assert lib.spdp_blk_finds(eng.ctx, dix.h, C.byref(dix.desc), C.byref(prm), q[0].ctypes.data, offs.ctypes.data, left.ctypes.data,
                              right.ctypes.data, 1, out.ctypes.data, 64, None) == -1
    assert b"bad query range" in lib.spdp_last_error(eng.ctx)


@pytest.mark.parametrize("name", af.SETS)
@pytest.mark.parametrize("max_out,local", [(1, 0), (4, 0), (2, 1)])
def test_the_programs_indexes(eng, tmp_path, name, max_out, local):
    """the index files `spaln -W -KA` wrote, read by the library, every query of the fixture (the refused ones too)"""
    arrays, prm = blocks.read_protein_db_index(eng.lib, af.bka_path(name, str(tmp_path)), max_out=max_out, local=local)
    ix = af.index(name, max_out, local)
    assert (prm.ptpl, prm.avrscr) == (ix.ptpl, ix.avrscr) and prm.rln_coef == np.float32(ix.rlncoef)
    queries = [af.encode(q["seq"]) for q in af.search(name)["queries"]]
    want = [fr.record(fr.finds(ix, q)) for q in queries]
    dix = blocks.BlockIndex(eng, arrays)
    try:
        got, _ = blocks.finds(dix, prm, queries, out_cap=64)
    finally:
        dix.free()
    same_records(got, want, (name, max_out, local))
    assert not any(got[k, 2] & (fr.TABLE | fr.CUT) for k in range(got.shape[0]))
