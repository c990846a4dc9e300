"""The DP step of spdp_sweep_fp where its values meet the floor, and where the penalty-table address is carried.

The gap opened from a cell is carried unfloored (`h + gop + gep`) and the floor is the third operand of the two maxima it
feeds, so the "extended or opened" compares of E and F see the unfloored value: they differ from the int32 sweep's only in
E / F states that sit at the floor, whose links no cell ever takes.  The cases put floor cells beside, and on, the paths
that are reported: global ends (first row and column run into the floor), bands narrower than the rectangle, rows that
reach the floor over 3000 quiet columns with a donor fired from there, intermediate rows that cross floor regions, and
problems whose only alignments are floor-derived.

The address of the penalty entry is carried less the step's share inside a half block of 8 steps (the read's immediate
offset advances it; a donor at step J sets the constant for which that read lands on entry 1; the half block adds its 64
bytes once): donors on every step of a block, so on the last step of a half block and the first of the next, in runs of
1, 2 and 17, and a second donor behind pen_cap, under the three tables of test_gpu_sweep_step._cap_scorings.

Every case runs with SPDP_FP=1 and SPDP_FP=0 and both are judged by the CPU oracle; spdp_sweep_stats says which kernel
ran (tests/test_gpu_fp_sweep_oracle.py: _check).  Linear-space results are compared where the reference's own are well
defined (test_gpu_fuzz._well_defined), at most a third of a case's may be left out; score-only and traceback results are
compared on every problem."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from spaln_amd import defaults, synth
from tests.test_gpu_fp_sweep_oracle import _check, _oracle, _serves, _share, _spec
from tests.test_gpu_sweep_step import FREE, GLOBAL, _cap_scorings, _fits_fp, _two_exons

pytestmark = pytest.mark.gpu

NEV16 = -32768 + 1024                               # SPDP_NEV16: what a cell that no alignment reaches starts from
ROWS = (40, 47, 48, 49, 64, 65, 81, 96, 97, 113, 129, 130)      # one to three passes, most with a partial last stripe (make_gene may add a few rows)


@pytest.fixture(scope="module")
def eng():
    from spaln_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(max(1, min(16, os.cpu_count() or 1))) as p:
        yield p


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _gene(rng, rows, n_exons, flank, intron_lo, intron_hi, exg):
    g = synth.make_gene(rng, n_exons=n_exons, mrna_len=rows, flank=flank, intron_lo=intron_lo, intron_hi=intron_hi,
                        sub=0.03, indel=0.0, exon_min=12)
    s5, s3 = synth.splice_signals(g.window)
    return _spec(defaults.encode(g.query), defaults.encode(g.window), s5, s3, exg=exg)


def _global_specs(rng):
    """global ends on both sequences: the first row and the first column ramp down to `nevsel` and on to the floor right
    beside the path's first cells, and every cell far from the diagonal of an exon sits at the floor (windows of 300 ..
    3000 columns against 40 .. 130 rows)"""
    specs = []
    for i, rows in enumerate(ROWS):
        n_ex = 2 + i % 2
        lo = (270, 600, 1100)[i % 3]
        specs.append(_gene(rng, rows, n_ex, int(rng.integers(0, 9)), lo, lo + 250, GLOBAL))
    for s in specs:
        assert 300 <= s["w"].size <= 3000, s["w"].size
    return specs


def _band_specs(rng):
    """the same shapes under a band shoulder of 10: cells outside the band are never computed, the cells at its two
    edges take floor values from them on both sides of the path; global and free ends in turn"""
    return [_gene(rng, rows, 2 + i % 2, 4 + i, 270, 500, GLOBAL if i & 1 else FREE) for i, rows in enumerate(ROWS)]


def _floor_donor_specs(rng, sc):
    """3000 columns whose sig5 + ipen is -32768, no donor can fire there and under global ends every row of the 40 runs
    into the floor; then a donor of +300 and more 60 .. 75 columns in front of the gene, fired from cells at the floor, its
    acceptor three columns in front of the gene's first exon, and the planted two-exon gene itself.  Free ends (the real
    path is reported, the floor-derived intron ends beside it) and global ends (the reported path itself comes out of the
    floor; every fourth: the linear-space links of most such paths are not well defined)"""
    specs = []
    for ph in range(12):
        L = 60 + 3 * ph
        don = {0: 150, -20 - 60 - ph: 300 + 40 * ph}
        acc = {L: 150, -20 - 3: 300}
        s, _ = _two_exons(rng, 40, 20, L, 3000 + 90 + ph, 6, don, acc, exg=GLOBAL if ph % 4 == 3 else FREE, quiet=-32768 - sc.ipen)
        specs.append(s)
    return specs


def _imd_specs(rng):
    """queries of 70 .. 130 rows against 1600 .. 3000 columns, global ends: an intermediate row runs from the band's
    left edge to its right one, nearly all of it through cells at the floor"""
    specs = [_gene(rng, rows, 3, int(rng.integers(0, 9)), 800, 1300, GLOBAL) for rows in (70, 79, 80, 81, 96, 97, 112, 113, 128, 130)]
    for s in specs:
        assert 1600 <= s["w"].size <= 3000, s["w"].size
    return specs


def _unrelated_specs(rng, sc):
    """no admissible alignment: an unrelated query (and one of Ns) against 3000 columns without a splice site, global
    ends: whatever crosses the window has been at the floor"""
    specs = []
    for k, rows in enumerate((40, 65, 97, 130)):
        w = synth.random_dna(rng, 3000 - 100 * k)
        q = np.full(rows, ord("N"), np.uint8) if k == 1 else synth.random_dna(rng, rows)
        s5 = np.full(w.size + 1, -32768 - sc.ipen, np.int16)         # (sig5 + ipen = -32768: no donor, so no intron either)
        s3 = np.full(w.size + 1, -900, np.int16)
        specs.append(_spec(defaults.encode(q), defaults.encode(w), s5, s3, exg=GLOBAL))
    return specs


def _donor_run_specs(rng, sc):
    """runs of 1, 2 and 17 adjacent donors (each stronger than the one before by more than the gap that leads to it) and
    an acceptor llmt or llmt + 1 columns behind the last (only the second is an intron: a donor that lands one entry too
    far prices the first too, and the signals are strong enough that it would be taken), the window start moved through
    the 16 phases of a block: in every row a donor falls on each step of a block, the last of a half block and the first
    of the next among them"""
    specs = []
    for run in (1, 2, 17):
        for gap in (sc.llmt, sc.llmt + 1):
            for ph in range(16):
                rows = 40 + (ph * 23) % 91               # 40 .. 130
                L = run - 1 + gap
                don = {i: 300 + 110 * i for i in range(run)}
                s, _ = _two_exons(rng, rows, rows // 2, L, 2 + ph, 260, don, {L: 300}, exg=FREE if ph & 1 else GLOBAL)
                specs.append(s)
    return specs


def _second_donor_specs(rng, sc, pen_cap):
    """a second donor 1 .. 16 columns after hil has passed pen_cap, its acceptor llmt + 5 columns on (as
    test_gpu_sweep_step.test_second_donor_behind_the_cap, with 40 and more rows)"""
    specs = []
    for j in range(1, 17):
        k = pen_cap + j
        L = k + sc.llmt + 5
        s, _ = _two_exons(rng, 40 + 5 * j, 20, L, 2 + (5 * j) % 16, 230, {0: 80, k: 500 + k}, {L: 80}, exg=GLOBAL)
        specs.append(s)
    return specs


ALL = ("score", "fwd", ("udh", 3))


# ---- 1. floor cells beside and on the path ----------------------------------------------------------------------------
def test_global_ends(eng, pool):
    rng = np.random.default_rng(synth.SEED + 13100)
    sc = defaults.scoring()
    specs = _global_specs(rng)
    want = _oracle(pool, sc, specs, ALL)
    assert all(wt["score"] > -1000 for wt in want), [wt["score"] for wt in want]  # (the planted gene is what is found)
    _check(eng, sc, specs, want, served=True, tag="floor_global", n_im=3)
    _share(want, "global ends")


def test_band_narrower_than_the_rectangle(eng, pool):
    rng = np.random.default_rng(synth.SEED + 13200)
    sc = defaults.scoring(sh=10)
    specs = _band_specs(rng)
    want = _oracle(pool, sc, specs, ALL)
    _check(eng, sc, specs, want, served=True, tag="floor_band", n_im=3)
    _share(want, "band narrower than the rectangle")


def test_donor_fired_from_the_floor(eng, pool):
    rng = np.random.default_rng(synth.SEED + 13300)
    sc = defaults.scoring(nquant=1, llmt=20)
    assert _serves(sc)
    specs = _floor_donor_specs(rng, sc)
    _fits_fp(sc, specs)
    want = _oracle(pool, sc, specs, ALL)
    # free ends: the real path; global ends: a score that came out of the floor
    assert all((wt["score"] > 0) == (s["exg"] == FREE) for wt, s in zip(want, specs)), [wt["score"] for wt in want]
    assert all(wt["score"] < NEV16 + 40 * 20 + 600 for wt, s in zip(want, specs) if s["exg"] == GLOBAL)
    _check(eng, sc, specs, want, served=True, tag="floor_donor", n_im=3)
    _share(want, "donor fired from the floor")


@pytest.mark.parametrize("n_im", [8, 16])
def test_intermediate_rows_across_the_floor(eng, pool, n_im):
    rng = np.random.default_rng(synth.SEED + 13400 + n_im)
    sc = defaults.scoring()
    specs = _imd_specs(rng)
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", n_im)))
    _check(eng, sc, specs, want, served=True, tag=("floor_imd", n_im), n_im=n_im, engines=("udh",))
    _share(want, "intermediate rows across the floor, n_im %d" % n_im)


def test_no_admissible_alignment(eng, pool):
    """score only: the host ignores the links of such a problem"""
    rng = np.random.default_rng(synth.SEED + 13500)
    sc = defaults.scoring()
    specs = _unrelated_specs(rng, sc)
    want = _oracle(pool, sc, specs, ("score",))
    assert all(wt["score"] <= NEV16 + 130 * 20 for wt in want), [wt["score"] for wt in want]
    _check(eng, sc, specs, want, served=True, tag="floor_unrelated", engines=("score",))


# ---- 2. the penalty-table address -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_donors_on_every_step_of_a_block(eng, pool, which):
    name, sc, pen_cap = _cap_scorings()[which]
    assert _serves(sc)
    rng = np.random.default_rng(synth.SEED + 13600 + which)
    specs = _donor_run_specs(rng, sc)
    _fits_fp(sc, specs)
    want = _oracle(pool, sc, specs, ALL)
    _check(eng, sc, specs, want, served=True, tag=("addr_runs", name), n_im=3)
    _share(want, "donors on every step of a block, %s" % name)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_second_donor_behind_the_cap(eng, pool, which):
    name, sc0, pen_cap = _cap_scorings()[which]
    sc = defaults.scoring(nquant=sc0.nquant, llmt=20, gep=-1, qm_len=[sc0.qm_len[j] for j in range(5)],
                          qm_pen=[sc0.qm_pen[j] for j in range(5)])
    assert _serves(sc)
    rng = np.random.default_rng(synth.SEED + 13700 + which)
    specs = _second_donor_specs(rng, sc, pen_cap)
    _fits_fp(sc, specs)
    want = _oracle(pool, sc, specs, ALL)
    _check(eng, sc, specs, want, served=True, tag=("addr_second", name), n_im=3)
    _share(want, "second donor behind the cap, %s" % name)


# ---- 3. the other geometries ------------------------------------------------------------------------------------------
def test_floor_in_every_geometry(eng, pool):
    """global ends and long introns (floor cells all around the path, donors from every step of a block) in the multi-wave
    geometry (>= 16 stripes), the same problems one wave each (SPDP_MULTI=0), and a query of 2100 rows as cross-CU groups
    of 4-wave blocks (SPDP_CROSS_WPB=4); then the traceback flavour alone on queries of 500 rows"""
    rng = np.random.default_rng(synth.SEED + 13800)
    sc = defaults.scoring()
    specs = [_gene(rng, rows, 3, 5, 500, 900, GLOBAL) for rows in (257, 300, 333)]
    want = _oracle(pool, sc, specs, ALL)
    _check(eng, sc, specs, want, served=True, tag="floor_multi", n_im=3, blocks16=None)
    _check(eng, sc, specs, want, served=True, tag="floor_one_wave", n_im=3, env=dict(SPDP_MULTI=0), blocks16=False)
    tall = [_gene(rng, 2100, 4, 5, 300, 600, GLOBAL)]
    want_t = _oracle(pool, sc, tall, ("score", "fwd", ("udh", 16)))
    cross = {}
    _check(eng, sc, tall, want_t, served=True, tag="floor_cross4", n_im=16, engines=("udh",), env=dict(SPDP_CROSS_WPB=4),
           blocks16=False, cross=cross)
    assert cross[("udh", 1)][0], cross
    _share(want + want_t, "floor in every geometry")
    fwd = [_gene(rng, 500, 3, 5 + 7 * i, 200, 700, GLOBAL if i & 1 else FREE) for i in range(4)]
    want_f = _oracle(pool, sc, fwd, ("fwd",))
    _check(eng, sc, fwd, want_f, served=True, tag="floor_fwd500", engines=("fwd",))
