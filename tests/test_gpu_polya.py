"""The query preparation on the device (spdp_polya.hip; include/spdp.h "query preparation"): spdp_polya_scan and
spdp_polya_scan_resident against spdp_polya_scan_host on the whole set of tests/polya_cases.py, and spdp_map_align_s_prep with a
preparation that scans nothing against spdp_map_align_s."""
import ctypes as C
import os

import numpy as np
import pytest

from spaln_amd import abi, blocks
from tests import polya_cases, spdg
from tests.conftest import golden_files
from oracle import blk
from tests.test_blk_find import CASES, genome_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from spaln_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


def _odd_starts(qs):
    """the same queries with one-residue queries put between them wherever the next one would begin at an even offset;
    -> (the list, the positions of the real ones in it)"""
    out, real, at = [], [], 0
    for q in qs:
        if at % 2 == 0:
            out.append(np.array([polya_cases.C], dtype=np.uint8))
            at += 1
        real.append(len(out))
        out.append(q)
        at += len(q)
    return out, real


@pytest.mark.parametrize("q_mns,thr", polya_cases.PARAMS)
@pytest.mark.parametrize("packing", ["batch", "odd"])
def test_device_scan_equals_the_host_scan(eng, q_mns, thr, packing):
    qs = list(polya_cases.queries())
    if packing == "odd":
        qs, real = _odd_starts(qs)
        starts = np.concatenate([[0], np.cumsum([len(q) for q in qs])])[real]
        assert (starts % 2 == 1).all()
    want_rec, want_codes = blocks.polya_scan_host(eng.lib, qs, q_mns, thr)
    for resident in (False, True):
        rec, codes, ms = blocks.polya_scan(eng, qs, q_mns, thr, resident=resident)
        bad = np.nonzero((rec != want_rec).any(axis=1))[0]
        assert bad.size == 0, (resident, bad[:5], rec[bad[:5]], want_rec[bad[:5]], [len(qs[i]) for i in bad[:5]])
        for i, (g, w) in enumerate(zip(codes, want_codes)):
            assert np.array_equal(g, w), (resident, i, len(w))
        assert ms >= 0


def test_device_scan_refuses_what_the_host_scan_refuses(eng):
    q = [np.full(40, polya_cases.A, np.uint8)]
    for bad in (2, 0):
        with pytest.raises(RuntimeError, match="q_mns"):
            blocks.polya_scan(eng, q, bad, 12)
    rec, _, _ = blocks.polya_scan(eng, [], 3, 12)
    assert rec.shape == (0, 5)


def _setup(eng, name, n_genes, seed, par):
    """the set-up of tests/test_gpu_e2e.py::test_one_call_equals_its_steps"""
    fx = spdg.load([f for f in golden_files("blk_") if f.endswith(name + ".spdg")][0])
    fq = spdg.load(os.path.join(ROOT, "tests", "golden", "q_c2_seed0.spdg"))
    gen, off = genome_of(name, n_genes, seed, par)
    dix = blocks.BlockIndex(eng, fx)
    model = abi.wilip_model_from_fixture(fx)
    sigmodel = abi.signal_model_from_fixture(fq)
    prm = blocks.find_params_from_fixture(fx)
    sc = spdg.scoring(fq, intpen=np.ascontiguousarray(fx["find_intpen"], dtype=np.int16), scalar_engines=1, llmt=model.llmt, minl=model.minl)
    sp = abi.seed_params_from_fixture(fq)
    sp.minl, sp.ip_maxl = model.minl, model.maxl
    fs = fq["rng_fstat_A0"] if "rng_fstat_A0" in fq else [0, 0, 0, 0, 0, 0, 3, 1]
    rescore = (fq["prm"]["codonk1"], model.minl, int(fs[6]), int(fs[7]))
    queries = [q["codes"][q["left"]:q["right"]] for q in blk.parse_log(fx)]
    sp.wilip = C.addressof(model)
    return dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, model


@pytest.mark.parametrize("name,n_genes,seed,par", [c for c in CASES if c[0] in ("blk_par", "blk_k1")],
                         ids=[c[0] for c in CASES if c[0] in ("blk_par", "blk_k1")])
def test_a_preparation_that_scans_nothing_changes_nothing(eng, name, n_genes, seed, par):
    """polya_thr = 0 and q_mns = 1 / 3: spdp_map_align_s with ori = 1 / 3, gene for gene; the records say "no tail" """
    dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, model = _setup(eng, name, n_genes, seed, par)
    try:
        for ori in (1, 3):
            old, _, rc0 = blocks.map_align(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, ori=ori)
            new, _, rc1, rec = blocks.map_align_prep(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, q_mns=ori, polya_thr=0)
            assert rc0 == rc1 == 0
            assert sum(g is not None for g in old) >= 10
            assert new == old, ori
            assert rec.tolist() == [[0, len(q), 0, len(q), ori] for q in queries]
        # a missing preparation and -S2 are refused with a message, before anything runs
        for kw, what in ((dict(q_mns=2), "q_mns = 2"),):
            with pytest.raises(RuntimeError, match=what):
                blocks.map_align_prep(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, **kw)
        lib = eng.lib
        genes = (blocks.MapGene * len(queries))()
        exons = C.POINTER(blocks.MapExon)()
        codes, offs = blocks._packed(queries)
        g = blocks.Genome()
        gc, go = np.ascontiguousarray(gen, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
        g.codes, g.chr_off, g.n_chr = gc.ctypes.data, go.ctypes.data, len(go) - 1
        rp = abi.RescoreParams(*(int(x) for x in rescore))
        rc = lib.spdp_map_align_s_prep(eng.ctx, dix.h, C.byref(dix.desc), C.byref(g), C.byref(sc), C.byref(sp), C.addressof(sigmodel),
                                       C.byref(prm), C.byref(rp), codes.ctypes.data, offs.ctypes.data, len(queries), None, genes,
                                       C.byref(exons), None, None)
        assert rc == -1 and b"SpdpQueryPrep" in lib.spdp_last_error(eng.ctx)
    finally:
        dix.free()
