"""Parity at BASELINE's headline size against the REFERENCE itself (fixtures c2_seed*, c5_6kb: ref_dump -A 0).
Beyond 1472 nt the reference's int16 engines (-A1..3) are erratic and its scalar int32 engines (-A0) are the truth
(SURVEY.md App. B), so a 2 kb / 6 kb fixture can only hold -A0 records.  Two things are pinned here on the CPU:
  (a) the oracle's -A0 ladder (hexagonal volume, hirschbergS_ng rounds, forwardS_ng slabs) equals the reference's
      -A0 output exactly: HomScoreS_ng, gsi->scr, the SKL, skl_rngS_ng's score and exon records;
  (b) the `_wip` model the GPU runs at that size (int32, no int16 re-basing) finds the same gene: its exon
      boundaries against the reference's -A0 alignment, counted and thresholded, and the rescored total where the two
      corner lists coincide."""
import pytest

from tests import spdg
from tests.conftest import golden_files
from oracle import host_logic

BIG = golden_files("c2_") + golden_files("c5_")
IDS = [f.split("/")[-1][:-5] for f in BIG]
# what the `_wip` model (int32, as the GPU runs it) reproduces of the reference's -A0 alignment, fixture by fixture:
# exon ends of the reference found / exon ends of the reference, and whether the two corner lists are the same list
WIP_VS_A0 = {"c2_seed0": (16, 16, True), "c2_seed1": (16, 16, True), "c2_seed2": (16, 16, False),
             "c2_seed3": (16, 16, True), "c5_6kb": (48, 48, False),
             "c2_iupac": (8, 10, False)}     # IUPAC letters at the junctions: the 16-nt third exon (2921 .. 2937) is -A0's alone


@pytest.mark.parametrize("path", BIG, ids=IDS)
def test_scalar_ladder_equals_reference_A0(path):
    fx = spdg.load(path)
    sc = spdg.scoring(fx)
    _, p = spdg.problem(fx)
    assert host_logic.homscore_s(sc, p, simd=0) == int(fx["hom_scr_A0"][0])
    scr, skl = host_logic.align_s(sc, p, simd=0)
    assert scr == int(fx["aln_scr_A0"][0])
    assert (skl or []) == fx["aln_skl_A0"].tolist()
    fs = fx["rng_fstat_A0"]
    h, fst, recs = host_logic.skl_rng_s(sc, p, skl, codonk1=fx["prm"]["codonk1"], minl=fx["prm"]["minl"],
                                        jneibr=int(fs[6]), lsg=int(fs[7]))
    assert h == int(fx["rng_scr_A0"][0])
    assert recs == fx["rng_eij_A0"].reshape(-1, 21).tolist()


def exon_bounds(skl, minl):
    """genomic (start, end) of every exon of a corner list [flags, n, m1, n1, ...]: a gap in the query of more than
    minl columns is an intron (skl2exrng, src/spaln.cc:651-668)"""
    c = [(skl[i], skl[i + 1]) for i in range(2, len(skl), 2)]
    out, start = [], c[0][1]
    for (m0, n0), (m1, n1) in zip(c, c[1:]):
        if m1 == m0 and n1 - n0 > minl:
            out.append((start, n0))
            start = n1
    out.append((start, c[-1][1]))
    return out


@pytest.mark.parametrize("path", BIG, ids=IDS)
def test_wip_model_finds_the_reference_A0_gene(path):
    fx = spdg.load(path)
    sc = spdg.scoring(fx)
    _, p = spdg.problem(fx)
    scr, skl = host_logic.align_s(sc, p, simd=2)            # what the GPU runs: the `_wip` ladder in int32
    assert skl, "no alignment"
    ref = fx["aln_skl_A0"].tolist()
    minl = fx["prm"]["minl"]
    ex_w, ex_r = exon_bounds(skl, minl), exon_bounds(ref, minl)
    ends_w = {x for e in ex_w for x in e}
    ends_r = [x for e in ex_r for x in e]
    hit = sum(x in ends_w for x in ends_r)
    name = path.split("/")[-1][:-5]
    assert (hit, len(ends_r), skl == ref) == WIP_VS_A0[name]      # exact: a regression to "most of them" must not pass
    assert abs(len(ex_w) - len(ex_r)) <= 2
    if skl == ref:                                           # same traceback: the rescored total is engine-independent
        fs = fx["rng_fstat_A0"]
        h, _, _ = host_logic.skl_rng_s(sc, p, skl, codonk1=fx["prm"]["codonk1"], minl=minl, jneibr=int(fs[6]), lsg=int(fs[7]))
        assert h == int(fx["rng_scr_A0"][0])


def test_fullsize_fixtures_are_full_size():
    qs = [spdg.load(f)["prm"]["a_right"] for f in BIG]
    assert sum(1 for q in qs if 1900 <= q <= 2100) >= 4 and max(qs) >= 5900
