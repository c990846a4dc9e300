"""The locus search on a device group (spdp_group_blk_find): three contexts on ONE card against spdp_blk_find on one context -- the
paralog genome (two loci per query, antisense reads among the queries) and protein queries on the translated index.  Every field of
every locus, status, every int of every HSP; SpdpLocus.query in the caller's numbering."""
import ctypes as C

import numpy as np
import pytest

from oracle import blk
from spaln_amd import abi, blocks, defaults, engine
from tests import spdg
from tests.conftest import golden_files
from tests.test_blk_find import CASES, PROTEIN_CASES, genome_of

pytestmark = pytest.mark.gpu
LOCUS = ("query", "chr", "rvs", "base", "len", "left", "right", "jscr", "n_hsp")


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


def raw_find(index, gen, off, model, sc, prm, queries, ranges):
    """the entry's own arrays: ([locus fields + its HSPs' ints] in the order of *loci, status)"""
    call = blocks._Call(index, gen, off, queries, C.c_void_p(C.addressof(model)), C.byref(sc), C.byref(prm))
    n = call.n
    left = np.array([r[0] for r in ranges], dtype=np.int32)
    right = np.array([r[1] for r in ranges], dtype=np.int32)
    loci, hsps, nl = C.POINTER(blocks.Locus)(), C.POINTER(C.c_int32)(), C.c_int32()
    status = np.full(n, -99, dtype=np.int32)
    assert call.run("spdp_blk_find", left, right, n, C.byref(loci), C.byref(nl), C.byref(hsps), status) == 0
    out, at = [], 0
    for k in range(nl.value):
        L = loci[k]
        assert L.hsp_off == at                          # the pooled HSPs lie in the order of the loci, nothing between them
        out.append([getattr(L, f) for f in LOCUS] + [hsps[5 * L.hsp_off + j] for j in range(5 * (L.n_hsp + 1))])
        at += L.n_hsp + 1
    blocks._free(loci, hsps)
    return out, status


@pytest.mark.parametrize("name", ["blk_par", "blk_p1"])
def test_loci_equal_one_context(eng, grp, name):
    n_genes, seed, par = [c[1:] for c in CASES + PROTEIN_CASES if c[0] == name][0]
    fx = spdg.load([f for f in golden_files("blk_") if f.endswith(name + ".spdg")][0])
    gen, off = genome_of(name, n_genes, seed, par)
    model = abi.wilip_model_from_fixture(fx)
    prm = blocks.find_params_from_fixture(fx)
    v = [int(x) for x in fx["find_prm"]]
    sc = defaults.scoring(intpen=np.ascontiguousarray(fx["find_intpen"], dtype=np.int16))
    sc.gop, sc.gep, sc.lgop, sc.lgep, sc.codonk1 = v[13], v[14], v[15], v[16], v[17]
    qs = blk.parse_log(fx)
    queries = [q["codes"] for q in qs]
    ranges = [(q["left"], q["right"]) for q in qs]
    if name == "blk_par":                               # antisense reads among them (tests/test_gpu_multi.py)
        comp = np.arange(256, dtype=np.uint8)
        for a, b in ((2, 9), (9, 2), (3, 5), (5, 3)):
            comp[a] = b
        queries = [np.ascontiguousarray(comp[q[::-1]]) if i % 2 else q for i, q in enumerate(queries)]
        ranges = [(len(q) - r[1], len(q) - r[0]) if i % 2 else r for i, (q, r) in enumerate(zip(queries, ranges))]
    # queries nobody finds anything for, at the start, in the middle and at the end: their slots stay empty
    rng = np.random.default_rng(5)
    letters = np.array(list(range(3, 23)) if name == "blk_p1" else [2, 3, 5, 9], dtype=np.uint8)
    for at in (0, len(queries) // 2, len(queries)):
        queries.insert(at, rng.choice(letters, size=300))
        ranges.insert(at, (0, 300))
    dix = blocks.BlockIndex(eng, fx)
    gix = blocks.GroupIndex(grp, fx)
    try:
        want, want_status = raw_find(dix, gen, off, model, sc, prm, queries, ranges)
        got, got_status = raw_find(gix, gen, off, model, sc, prm, queries, ranges)
        member = grp.shards(len(queries))
        lists, status = blocks.group_find(gix, gen, off, model, sc, prm, queries, ranges)
        tasks = [blocks.find_stats(grp.context(r))["tasks"] for r in range(3)]
    finally:
        gix.free()
        dix.free()
    assert got == want
    assert got_status.tolist() == want_status.tolist() and status.tolist() == want_status.tolist()
    assert set(member.tolist()) == {0, 1, 2} and all(t > 0 for t in tasks)
    per_query = np.bincount([r[0] for r in want], minlength=len(queries))
    assert [r[0] for r in want] == sorted(r[0] for r in want)           # query by query, in the caller's numbers
    assert [len(x) for x in lists] == per_query.tolist()
    assert len(want) >= 15 and (per_query == 0).any()
    if name == "blk_par":
        assert (per_query >= 2).sum() >= 8              # two loci per query
        assert any(r[2] for r in want) and any(not r[2] for r in want)
