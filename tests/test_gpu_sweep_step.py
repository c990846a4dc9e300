"""The DP step of spdp_sweep_fp where its penalty-table index and its donor state are handled: hil advances without a
clamp and is clamped once per block of 16 steps (the table is padded by 16 entries that price like pen_cap), and the
entry a step prices with is read after the donor decision of the step before (a donor lands on entry 1, which yields
`nevsel`).  Planted signals put the donors and acceptors exactly where these paths turn: introns a little longer than
pen_cap at every phase of a block, a second donor right after the cap was passed, rows that never see a donor, donors
on adjacent columns with an acceptor 1, 2, llmt, llmt + 1 columns behind them, and intermediate rows at the edges of
narrow bands.

Every case runs all its flavours with SPDP_FP=1 and SPDP_FP=0 (the int32 sweeps of spdp_kernels.hip on the same
problems) and both are judged by the CPU oracle; spdp_sweep_stats says which kernel ran (tests/test_gpu_fp_sweep_oracle.py:
_check).  Linear-space results are compared where the reference's own are well defined (test_gpu_fuzz._well_defined), and
at most a third of a test's may be left out; score-only and traceback results are compared on every problem."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from spaln_amd import defaults, synth
from tests.test_gpu_fp_sweep_oracle import _check, _oracle, _serves, _share, _spec

pytestmark = pytest.mark.gpu

GLOBAL, FREE = (0, 0, 0, 0), (1, 1, 1, 1)
QUIET = -900                                        # a position that is no splice site


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
def _two_exons(rng, rows, e1, intron, lflank, rflank, donors, acceptors, exg=GLOBAL, quiet=QUIET):
    """a query of `rows` residues whose first e1 align in front of an intron of `intron` columns and the rest behind it;
    donors / acceptors: {offset from the intron's first column: signal}, every other position is `quiet`.  Returns the
    spec and the intron's first column"""
    q = synth.random_dna(rng, rows)
    w = np.concatenate([synth.random_dna(rng, lflank), q[:e1], synth.random_dna(rng, intron), q[e1:], synth.random_dna(rng, rflank)])
    s5 = np.full(w.size + 1, quiet, np.int16)
    s3 = np.full(w.size + 1, quiet, np.int16)
    d = lflank + e1
    for off, v in donors.items():
        s5[d + off] = v
    for off, v in acceptors.items():
        s3[d + off] = v
    return _spec(defaults.encode(q), defaults.encode(w), s5, s3, exg=exg), d


def _jump(wt):
    """the longest run of genome columns the oracle's traceback path crosses on one query row"""
    pts = sorted(tuple(x) for x in wt["fwd"][1])
    return max([n1 - n0 for (m0, n0), (m1, n1) in zip(pts[:-1], pts[1:]) if m1 == m0] or [0])


def _fits_fp(sc, specs):
    """DevRun's score bound for spdp_sweep_fp (rows x largest match + columns x what an intron can gain) holds"""
    for s in specs:
        gain = int(s["s5"].max()) + int(s["s3"].max()) + max(sc.qm_pen[j] for j in range(max(1, sc.nquant)))
        assert (s["q"].size + 1) * 20 + (s["w"].size + 1) * max(0, gain) + 65536 < (1 << 22) - 65536


def _cap_scorings():
    """(name, scoring, pen_cap): a flat table (pen_cap = llmt + 1), a quantile boundary at 200, and the longest table
    spdp_sweep_fp serves (qm_len[nquant - 2] = 990: entries 0 .. 991, the pad right behind the table's last entry)"""
    flat = defaults.scoring(nquant=1, llmt=20)
    q200 = defaults.scoring(nquant=2, llmt=20, qm_len=[200, 600, 900, 1300, 1400], qm_pen=[-190, -236, -281, -330, -395])
    last = defaults.scoring(nquant=4, llmt=20, qm_len=[200, 600, 990, 1300, 1400], qm_pen=[-190, -236, -281, -330, -395])
    return [("flat", flat, 21), ("q200", q200, 201), ("last990", last, 991)]


# ---- 1. the clamp, once per block -------------------------------------------------------------------------------------
def _clamp_specs(rng, sc, pen_cap):
    """planted introns of pen_cap + 1 .. pen_cap + 40 columns behind one strong donor and no further one: hil stands in
    the table's pad when the acceptor is priced.  One problem moved a column at a time through the 16 phases of a block
    (its acceptor on every step of a block; every row of a stripe is one step behind the row above, so a window also
    holds every phase of the step at which hil passes pen_cap), then 16 of other sizes and intron lengths.  Returns the
    specs and the intron each one plants"""
    specs, want_jump = [], []
    for ph in range(16):
        L = pen_cap + 24
        s, _ = _two_exons(rng, 40, 20, L, 3 + ph, 6, {0: 80}, {L: 80}, exg=GLOBAL)
        specs.append(s); want_jump.append(L)
    for ph in range(16):
        free = ph % 4 == 3                               # (free ends: exons long enough to be worth the intron)
        rows = 60 if free else 20 + (ph * 11) % 41       # 20 .. 60
        L = pen_cap + 1 + (ph * 7) % 40
        s, _ = _two_exons(rng, rows, rows // 2, L, 3 + ph, 6, {0: 80}, {L: 80}, exg=FREE if free else GLOBAL)
        specs.append(s); want_jump.append(L)
    return specs, want_jump


@pytest.mark.parametrize("which", [0, 1, 2])
def test_clamp_once_per_block(eng, pool, which):
    """the cases of _clamp_specs and two whose rows see no donor at all over 3000 columns (hil sits at the clamp block
    after block) before the planted one, under the three tables of _cap_scorings; all three flavours"""
    name, sc, pen_cap = _cap_scorings()[which]
    assert _serves(sc)
    rng = np.random.default_rng(synth.SEED + 12100 + which)
    specs, want_jump = _clamp_specs(rng, sc, pen_cap)
    # rows that never see a donor over 3000 columns, then the planted intron: with sig5 + ipen = -32768 a cell of 1024 or
    # less (40 rows of matches: 800) stays at or below `nevsel`; free ends skip the flank, global ends cross it
    for exg in (FREE, GLOBAL):
        L = pen_cap + 23
        s, _ = _two_exons(rng, 40, 20, L, 3100, 6, {0: 150}, {L: 150}, exg=exg, quiet=-32768 - sc.ipen)
        specs.append(s); want_jump.append(L)
    _fits_fp(sc, specs)
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 1)))
    # the planted intron is the oracle's path (random residues beside a site may shift a few of them)
    hit = [_jump(wt) == L for wt, L in zip(want, want_jump)]
    assert sum(hit) >= len(hit) - 3, (name, [(L, _jump(wt)) for wt, L in zip(want, want_jump)])
    _check(eng, sc, specs, want, served=True, tag=("clamp", name), n_im=1)
    _share(want, "clamp once per block, %s" % name)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_second_donor_behind_the_cap(eng, pool, which):
    """a second donor 1 .. 16 columns after hil has passed pen_cap (hil stands in the pad when it is reset), its acceptor
    llmt + 5 columns on.  A gap of pen_cap + j columns leads to it on the row of the first donor, so the gap extension is
    1 and the second signal outweighs the gap"""
    name, sc0, pen_cap = _cap_scorings()[which]
    sc = defaults.scoring(nquant=sc0.nquant, llmt=20, gep=-1, qm_len=[sc0.qm_len[j] for j in range(5)],
                          qm_pen=[sc0.qm_pen[j] for j in range(5)])
    assert _serves(sc)
    rng = np.random.default_rng(synth.SEED + 12200 + which)
    specs, without = [], []
    for j in range(1, 17):
        k = pen_cap + j                                  # columns from the first donor to the second
        L = k + sc.llmt + 5
        s, d = _two_exons(rng, 24 + j, 12, L, 2 + (5 * j) % 16, 6, {0: 80, k: 500 + k}, {L: 80}, exg=GLOBAL)
        specs.append(s)
        s5 = s["s5"].copy()
        s5[d + k] = QUIET
        without.append(dict(s, s5=s5))
    _fits_fp(sc, specs)
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 1)))
    # the second donor is what the oracle's path leaves through: without it the score is another one
    base = _oracle(pool, sc, without, ("score",))
    assert sum(wt["score"] > b["score"] for wt, b in zip(want, base)) >= 12, [(wt["score"], b["score"]) for wt, b in zip(want, base)]
    _check(eng, sc, specs, want, served=True, tag=("second_donor", name), n_im=1)
    _share(want, "second donor behind the cap, %s" % name)


# ---- 2. donors on consecutive steps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [1, 2, 3, 17])
def test_donors_on_consecutive_steps(eng, pool, run):
    """`run` adjacent donor columns, each stronger than the one before by more than the gap that leads to it (every one
    of them fires, on the row of the exon's end and on the rows below it), and an acceptor 1, 2, llmt, llmt + 1 columns
    behind the last: only the last distance is an intron, and the signals are strong enough that an acceptor which
    wrongly found a price would be taken (donor + acceptor + ipen + penalty > the gap of the same length).  With llmt = 1
    the column behind a donor is the only one without a price: the entry a donor resets hil to.  A lone donor (run 1)
    stands on a hil far beyond llmt when it fires, a donor inside a run on hil = 1.  The window start runs through the
    16 phases of a block, so a pair of donor steps falls inside a block and across its boundary in every row; the cases
    with no flank and an exon of one residue put the run on the first steps of the first stripe.  Global and free ends"""
    rng = np.random.default_rng(synth.SEED + 12300 + run)
    every = []
    for llmt in (20, 1):
        specs = []
        for gap in sorted({1, 2, llmt, llmt + 1}):
            for ph in range(16):
                first = ph >= 14                         # the run on the first steps of the first stripe
                rows = 18 + (ph * 5) % 40
                L = run - 1 + gap
                don = {i: 300 + 110 * i for i in range(run)}
                s, _ = _two_exons(rng, rows, 1 if first else rows // 2, L, 0 if first else 2 + ph, 5, don, {L: 300},
                                  exg=FREE if ph & 1 else GLOBAL)
                specs.append(s)
        sc = defaults.scoring(llmt=llmt)
        assert _serves(sc)
        _fits_fp(sc, specs)
        want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 1)))
        every += want
        _check(eng, sc, specs, want, served=True, tag=("donor_run", run, llmt), n_im=1)
    _share(every, "donors on consecutive steps, run %d" % run)


# ---- 3. intermediate rows at their edges ------------------------------------------------------------------------------
def _imd_problem(rng, rows):
    g = synth.make_gene(rng, n_exons=3, mrna_len=rows, flank=int(rng.integers(20, 60)), intron_lo=40, intron_hi=160,
                        sub=0.03, indel=0.0)
    q = defaults.encode(g.query)
    s5, s3 = synth.splice_signals(g.window)
    return _spec(q, defaults.encode(g.window), s5, s3, exg=GLOBAL)


@pytest.mark.parametrize("n_im", [8, 16])
def test_intermediate_rows_at_their_edges(eng, pool, n_im):
    """queries of 70 .. 130 rows with 8 and 16 intermediate rows: several of them in one pass, in adjacent stripes and
    on the partial last stripe, under a band shoulder of 10 (blocks that the band enters or leaves part-way); one wave
    per problem, as DevRun::build lays such problems out"""
    rng = np.random.default_rng(synth.SEED + 12400 + n_im)
    sc = defaults.scoring(sh=10)
    assert _serves(sc)
    specs = [_imd_problem(rng, rows) for rows in (70, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128, 129, 130)]
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", n_im)))
    _check(eng, sc, specs, want, served=True, tag=("imd_edges", n_im), n_im=n_im, engines=("udh",))
    _share(want, "intermediate rows at their edges, n_im %d" % n_im)


def test_intermediate_rows_in_every_geometry(eng, pool):
    """16 intermediate rows in the multi-wave geometry (>= 16 stripes), the same problems one wave each (SPDP_MULTI=0),
    and a query of 2100 rows as cross-CU groups of 4-wave blocks (SPDP_CROSS_WPB=4)"""
    rng = np.random.default_rng(synth.SEED + 12500)
    sc = defaults.scoring(sh=10)
    specs = [_imd_problem(rng, rows) for rows in (257, 300, 333)]
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 16)))
    _check(eng, sc, specs, want, served=True, tag="imd_multi", n_im=16, engines=("udh",), blocks16=None)
    _check(eng, sc, specs, want, served=True, tag="imd_one_wave", n_im=16, engines=("udh",), env=dict(SPDP_MULTI=0), blocks16=False)
    tall = [_imd_problem(rng, 2100)]
    want_t = _oracle(pool, sc, tall, ("score", "fwd", ("udh", 16)))
    cross = {}
    _check(eng, sc, tall, want_t, served=True, tag="imd_cross4", n_im=16, engines=("udh",), env=dict(SPDP_CROSS_WPB=4),
           blocks16=False, cross=cross)
    assert cross[("udh", 1)][0], cross
    _share(want + want_t, "intermediate rows in every geometry")
