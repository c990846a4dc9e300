"""The `_wip` sweeps against the int32 CPU oracle where the other tests leave them to each other: problems of 17
stripes and more (multi-wave pass pipelines, 16-wave blocks, cross-CU groups) under random gap / intron parameters,
quantile tables of up to eight entries, random signals, sub-ranges and end flags; the edges of what spdp_sweep_fp
accepts (penalty table, llmt, the score bound of DevRun::build and its intron-gain term, scores at the floor); and
the alignS_ng ladder at that size.  Every case runs with SPDP_FP=1 and SPDP_FP=0 and is judged by the oracle, never by
the other kernel; which kernel and which geometry really ran is read from spdp_sweep_stats, so that a case that
claims to test the fp32 kernel, a fallback or a geometry cannot pass without having done so.

The linear-space engine's cpos rows and ranges are the reference's own only where test_gpu_fuzz._well_defined holds
(DESIGN.md section 2); the other cases are left out for wip_udh alone, and at most a third of a test's may be (the
gainful-intron and floor cases, whose paths hug the edges by construction, say how many they compared instead)."""
import ctypes as C
import multiprocessing as mp
import os

import numpy as np
import pytest

from spaln_amd import abi, defaults, synth
from tests.envknobs import Env
from tests.test_gpu_fuzz import _well_defined

pytestmark = pytest.mark.gpu

N_WORKERS = max(1, min(16, os.cpu_count() or 1))
FP_TAB = 992                                         # SPDP_FPEN_TAB of spdp_sweep_fp.hip


@pytest.fixture(scope="module")
def eng():
    from spaln_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool():
    # fresh interpreters (no copy of a process that has the device open); they only ever load the oracle
    with mp.get_context("spawn").Pool(N_WORKERS) as p:
        yield p


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _problem_set(specs):
    ps = abi.ProblemSet()
    for s in specs:
        ps.add(s["q"], s["w"], s["s5"], s["s3"], s["al"], s["ar"], s["bl"], s["br"], s["exg"])
    return ps


def _spec(q, w, s5, s3, al=0, ar=None, bl=0, br=None, exg=(1, 1, 1, 1)):
    return dict(q=q, w=w, s5=s5, s3=s3, al=int(al), ar=int(q.size if ar is None else ar), bl=int(bl),
                br=int(w.size if br is None else br), exg=tuple(int(x) for x in exg))


def _serves(sc):
    """what spdp_sweep_fp_serves answers for this scoring, asked as DevRun::launch asks it"""
    from spaln_amd import engine
    lib = C.CDLL(engine.LIB_PATH)
    nq = max(1, min(sc.nquant, abi.MAX_QUANT))
    pen_cap = sc.qm_len[nq - 2] + 1 if nq > 1 else 0
    return bool(lib.spdp_sweep_fp_serves(int(bool(sc.local)), int(bool(sc.spj)), nq, pen_cap, sc.llmt))


def _rand_scoring(rng, served=True, **over):
    """as test_gpu_fuzz._rand_scoring_s with nquant 1 .. 8 and eight lengths / penalties; the lengths are drawn so
    that the last one the penalty table has to reach (qm_len[nquant - 2]) lies below the table's end (served) or
    beyond it (not served: needs nquant >= 2)"""
    nq = int(rng.integers(1 if served else 2, 9))
    n_lo = nq - 1 if served else nq - 2
    lo = np.sort(rng.choice(np.arange(30, FP_TAB - 1), size=n_lo, replace=False))
    hi = np.sort(rng.choice(np.arange(FP_TAB - 1, 1500), size=8 - n_lo, replace=False))
    kw = dict(gop=-int(rng.integers(20, 120)), gep=-int(rng.integers(5, 40)), ipen=-int(rng.integers(100, 400)),
              llmt=int(rng.integers(5, 40)), qm_len=[int(x) for x in np.concatenate([lo, hi])],
              qm_pen=[int(x) for x in -rng.integers(150, 400, size=8)], nquant=nq, sh=int(rng.choice([10, 30, 100])))
    kw.update(over)
    sc = defaults.scoring(**kw)
    assert _serves(sc) == served, (kw, served)
    return sc


def _rand_problem(rng, rows_lo=260, rows_hi=2600, random_signals=False):
    """a planted gene whose query sub-range has rows_lo .. rows_hi rows (17 .. 163 stripes by default): random
    sub-ranges on both sequences, random end flags, signals of the synthetic model or fully random"""
    m = int(np.exp(rng.uniform(np.log(rows_lo), np.log(rows_hi + 1))))
    extra = int(rng.integers(0, m // 4 + 1))
    L = m + extra
    g = synth.make_gene(rng, n_exons=int(rng.integers(1, 7)), mrna_len=L, flank=int(rng.integers(L // 5 + 40, L // 5 + 600)),
                        intron_hi=int(rng.integers(200, 2500)), sub=float(rng.uniform(0, 0.2)),
                        indel=float(rng.uniform(0, 0.01)))
    w, q = defaults.encode(g.window), defaults.encode(g.query)
    al = int(rng.integers(0, extra + 1)) if rng.random() < 0.75 else 0
    ar = min(q.size, al + m) if rng.random() < 0.75 else q.size
    ar = min(ar, al + rows_hi)
    al = max(0, min(al, ar - rows_lo))
    assert rows_lo <= ar - al <= rows_hi and ar <= q.size
    bl = int(rng.integers(0, max(1, w.size // 6)))
    br_lo = max(bl + (ar - al) + 5, 2 * w.size // 3)
    assert br_lo <= w.size
    br = int(rng.integers(br_lo, w.size + 1))
    if random_signals:
        s5 = rng.integers(-900, 150, size=w.size + 1).astype(np.int16)
        s3 = rng.integers(-900, 150, size=w.size + 1).astype(np.int16)
    else:
        s5, s3 = synth.splice_signals(g.window)
    return _spec(q, w, s5, s3, al, ar, bl, br, rng.integers(0, 2, size=4))


def _planted(rng, intron_len, mrna_len=400, n_exons=3, flank=100, sub=0.02, indel=0.002, exg=(1, 1, 1, 1)):
    """a gene all of whose introns have the given length (>= 14: synth's intron carries its two signals)"""
    g = synth.make_gene(rng, n_exons=n_exons, mrna_len=mrna_len, flank=flank, sub=sub, indel=indel,
                        intron_lo=intron_len, intron_hi=intron_len)
    s5, s3 = synth.splice_signals(g.window)
    return _spec(defaults.encode(g.query), defaults.encode(g.window), s5, s3, exg=exg)


# ---- the oracle, one problem per task of the pool -------------------------------------------------------------------
def _oracle_job(job):
    sc_bytes, spec, what = job
    from oracle import oracle, host_logic
    sc = abi.Scoring.from_buffer_copy(sc_bytes)
    p = _problem_set([spec]).items[0]
    out = {}
    for w in what:
        if w == "score":
            out[w] = oracle.wip_scoreonly(sc, p)
        elif w == "fwd":
            s, skl = oracle.wip_forward(sc, p)
            out[w] = (s, skl.tolist())
        elif w == "align":
            try:
                s, skl = host_logic.align_s(sc, p)
                out[w] = (s, skl or [])
            except host_logic.NeedsScalarEngine:
                out[w] = None
        else:                                        # ("udh", n_im)
            s, cpos, rng = oracle.wip_udh(sc, p, w[1])
            out["udh"] = (s, cpos.tolist(), rng.tolist())
    return out


def _oracle(pool, sc, specs, what):
    assert not sc.intpen and not sc.sigmodel          # the struct travels as bytes: no pointers inside
    want = pool.map(_oracle_job, [(bytes(sc), s, what) for s in specs], chunksize=1)
    for wt in want:
        if "udh" in wt and "fwd" in wt:
            wt["defined"] = _well_defined(wt["udh"][2], wt["udh"][1], wt["fwd"][1], 1)
    return want


# ---- one batch on the device, both generations of the sweep, against what the oracle said ----------------------------
def _kernel_check(st, fp_expected, tag):
    if fp_expected:
        assert st[0] > 0 and st[1] == 0, ("meant for spdp_sweep_fp", tag, st.tolist())
    else:
        assert st[0] == 0 and st[1] > 0, ("meant for spdp_sweep (int32)", tag, st.tolist())


def _check(eng, sc, specs, want, *, served, tag, n_im=0, env=None, blocks16=None, engines=("score", "fwd", "udh"),
           cross=None):
    """runs `engines` over the batch with SPDP_FP=1 and =0 under the knobs of `env`, compares every problem with the
    oracle and the sweep counter with what the case is meant to exercise (served: spdp_sweep_fp takes it when allowed;
    blocks16: True / False / None = don't care; cross: None = no launch may use cross-CU groups, else a dict that
    collects, per engine and generation, whether the launch was laid out across CUs and whether it also ran so, i.e.
    was not repeated).  Returns the number of wip_udh comparisons made."""
    ps = _problem_set(specs)
    n_udh = 0
    for fp in (1, 0):
        for name in engines:
            t = (tag, "SPDP_FP=%d" % fp, name)
            with Env(SPDP_FP=fp, **(env or {})):
                eng.rerun_stats(reset=True)
                eng.sweep_stats(reset=True)
                if name == "score":
                    got = eng.wip_scoreonly(sc, ps).tolist()
                elif name == "fwd":
                    got = [(int(s), skl.tolist()) for s, skl in eng.wip_forward(sc, ps)]
                else:
                    us, ucpos, urng = eng.wip_udh(sc, ps, n_im)
                st, rr = eng.sweep_stats(reset=True), eng.rerun_stats(reset=True)
            _kernel_check(st, bool(fp) and served, t)
            if cross is None:
                assert st[2] == 0, (t, st.tolist())
            else:
                cross[(name, fp)] = (bool(st[2] > 0), bool(st[2] > 0 and rr[0] == 0))
            if blocks16 is not None and (cross is None or cross[(name, fp)][1]):
                assert (st[3] > 0) == blocks16, (t, st.tolist())
            for i, wt in enumerate(want):
                if name == "score":
                    assert got[i] == wt["score"], (t, i, got[i], wt["score"])
                elif name == "fwd":
                    assert got[i][0] == wt["fwd"][0] and got[i][1] == wt["fwd"][1], (t, i, got[i][0], wt["fwd"][0])
                elif wt["defined"]:
                    ws, wcpos, wrng = wt["udh"]
                    assert int(us[i]) == ws and urng[i].tolist() == wrng, (t, i, int(us[i]), ws)
                    assert ucpos[i].tolist() == wcpos, (t, i)
                    n_udh += 1
    return n_udh


def _share(want, what):
    n_def = sum(1 for wt in want if wt["defined"])
    print("%s: wip_udh well defined %d of %d (%.0f %% skipped)" % (what, n_def, len(want), 100.0 * (len(want) - n_def) / len(want)))
    assert 3 * (len(want) - n_def) <= len(want), (what, n_def, len(want))


# ---- a. mid-size fuzz -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_mid_size_fuzz(eng, pool, seed):
    """four rounds of 12 problems of 260 .. 2600 rows and 4 of 120 .. 239 rows (one wave each) under a random scoring;
    round 1's penalty table is too long for spdp_sweep_fp and must show up as int32 launches.  Geometries: the mixed
    batch as DevRun::build lays it out (the wide problems as 4-wave pipelines, the rest one wave each), one wave per
    problem (SPDP_MULTI=0), 16-wave blocks by the knob, and the wide ones alone (few enough that build picks 16-wave
    blocks itself)"""
    rng = np.random.default_rng(synth.SEED + 9700 + seed)
    every = []
    for rnd in range(4):
        served = rnd != 1
        sc = _rand_scoring(rng, served=served)
        wide = [_rand_problem(rng, random_signals=bool(k & 1)) for k in range(12)]
        slim = [_rand_problem(rng, 120, 239, random_signals=bool(k & 1)) for k in range(4)]
        n_im = int(rng.integers(1, 8))
        want = _oracle(pool, sc, wide + slim, ("score", "fwd", ("udh", n_im)))
        every += want
        for name, specs, wt, env, b16 in (("mixed", wide + slim, want, {}, False),
                                          ("one_wave", wide + slim, want, dict(SPDP_MULTI=0), False),
                                          ("wpb16", wide + slim, want, dict(SPDP_WPB16=1), True),
                                          ("auto16", wide, want[:12], {}, True)):
            _check(eng, sc, specs, wt, served=served, tag=(seed, rnd, name), n_im=n_im, env=env, blocks16=b16)
    _share(every, "mid-size fuzz, seed %d" % seed)


# ---- b. long queries across CUs -------------------------------------------------------------------------------------
def test_long_queries_across_cus(eng, pool):
    """few queries of 2100 .. 9000 rows: DevRun::build spreads each over several CUs (cross-CU pass groups), as 4-wave or
    16-wave blocks; SPDP_CROSS=0 keeps one CU per problem.  A cross-CU launch may be repeated without groups on a busy
    device (spdp_rerun_stats): such a case still has to match, but is not counted as coverage"""
    rng = np.random.default_rng(synth.SEED + 9800)
    every, laid_out, ran = [], set(), set()
    for case, (n_q, lo, hi) in enumerate(((1, 8000, 9000), (4, 2100, 4500), (2, 3000, 6500))):
        sc = _rand_scoring(rng, served=True)
        specs = [_rand_problem(rng, lo, hi, random_signals=bool(k & 1)) for k in range(n_q)]
        want = _oracle(pool, sc, specs, ("fwd", ("udh", 7)))
        every += want
        for name, env, b16 in (("auto", {}, None), ("cross4", dict(SPDP_CROSS_WPB=4), False),
                               ("cross16", dict(SPDP_CROSS_WPB=16), True)):
            cross = {}
            _check(eng, sc, specs, want, served=True, tag=(case, name), n_im=7, env=env, blocks16=b16,
                   engines=("fwd", "udh"), cross=cross)
            # the linear-space sweep of either generation and the traceback sweep of spdp_sweep_fp are laid out across CUs
            for k in (("udh", 1), ("udh", 0), ("fwd", 1)):
                assert cross[k][0], (case, name, k, cross)
                laid_out.add(k)
                if cross[k][1]:
                    ran.add(k)
            assert not cross[("fwd", 0)][0]
        _check(eng, sc, specs, want, served=True, tag=(case, "no_cross"), n_im=7, env=dict(SPDP_CROSS=0), blocks16=True,
               engines=("fwd", "udh"))
    print("cross-CU launches that ran as such:", sorted(ran))
    assert ran == laid_out, (ran, laid_out)
    _share(every, "long queries")


# ---- c. the penalty table's end and llmt ----------------------------------------------------------------------------
@pytest.mark.parametrize("last_len", [989, 990, 991])
def test_penalty_table_end(eng, pool, last_len):
    """qm_len[nquant - 2] = 990 needs entries 0 .. 991 of the 992 there are: the last scoring spdp_sweep_fp serves.
    The planted introns sit at llmt, llmt + 1, around the first quantile boundary, at pen_cap - 2 .. pen_cap + 2
    (pen_cap = last_len + 1: from there on every length prices alike) and far beyond; the quantile penalties differ
    by tens, so a boundary or a table entry that is off by one changes the score"""
    rng = np.random.default_rng(synth.SEED + 9900 + last_len)
    llmt = 20
    sc = defaults.scoring(llmt=llmt, qm_len=[200, 600, last_len, 1300, 1400], qm_pen=[-190, -236, -281, -330, -395], nquant=4)
    served = last_len + 1 < FP_TAB
    assert _serves(sc) == served
    pen_cap = last_len + 1
    lens = [llmt, llmt + 1, 199, 200, 201, 202] + list(range(pen_cap - 2, pen_cap + 3)) + [5000]
    specs = [_planted(rng, L, exg=(1, 1, 1, 1) if k & 1 else (0, 0, 0, 0)) for k, L in enumerate(lens)]
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 3)))
    # the planted introns are what the oracle's path takes (else the lengths above test nothing)
    n_hit = 0
    for L, wt in zip(lens[1:], want[1:]):
        pts = sorted(tuple(x) for x in wt["fwd"][1])
        n_hit += any(n1 - n0 == L and m1 == m0 for (m0, n0), (m1, n1) in zip(pts[:-1], pts[1:]))
    assert n_hit >= len(lens) - 3, n_hit
    _check(eng, sc, specs, want, served=served, tag=("table_end", last_len), n_im=3)
    _share(want, "penalty table end %d" % last_len)


@pytest.mark.parametrize("llmt", [1, 0])
def test_llmt_edge(eng, pool, llmt):
    """llmt = 1: every gap of two columns and more is an intron candidate (served); llmt = 0 is turned away.  Random
    signals (half of the problems) make the shortest introns worth taking"""
    rng = np.random.default_rng(synth.SEED + 9950 + llmt)
    sc = _rand_scoring(rng, served=llmt >= 1, llmt=llmt)
    specs = [_rand_problem(rng, 260, 700, random_signals=k % 2 == 0) for k in range(12)]
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 2)))
    _check(eng, sc, specs, want, served=llmt >= 1, tag=("llmt", llmt), n_im=2)
    _share(want, "llmt %d" % llmt)


def test_flat_penalty_ignores_the_table_bound(eng, pool):
    """nquant = 1 (-A3's flat penalty): qm_len[0] is not read, however large"""
    rng = np.random.default_rng(synth.SEED + 9960)
    sc = _rand_scoring(rng, served=True, nquant=1, qm_len=[30000] + [0] * 7, llmt=20)
    assert sc.nquant == 1 and sc.qm_len[0] == 30000 and sc.llmt == 20
    specs = [_planted(rng, L) for L in (sc.llmt, sc.llmt + 1, 990, 991, 992, 5000)]
    specs += [_rand_problem(rng, 260, 700, random_signals=True) for _ in range(4)]
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 3)))
    _check(eng, sc, specs, want, served=True, tag="flat", n_im=3)
    _share(want, "flat penalty")


# ---- d. the score range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [101, 102])
def test_score_bound_straddled(eng, pool, factor):
    """the nucleotide matrix times 101: DevRun::build's bound for 2000 error-free rows is 2001 * 2020 + 65536 =
    4 107 556 < 2^22 - 2^16 = 4 128 768, spdp_sweep_fp runs and the scores (about 4 037 000) are the largest it ever
    holds; times 102 the bound is 4 147 576 and the run has to stay with the int32 sweeps"""
    rng = np.random.default_rng(synth.SEED + 9970)
    sc = defaults.scoring(mtx=defaults.NMTX * factor)
    specs = []
    for k in range(6):
        g = synth.make_gene(rng, n_exons=4, mrna_len=2000, flank=300, sub=0.0, indel=0.0, intron_hi=1500)
        s5, s3 = synth.splice_signals(g.window)
        specs.append(_spec(defaults.encode(g.query), defaults.encode(g.window), s5, s3, exg=(1, 1, 1, 1) if k & 1 else (0, 0, 0, 0)))
        assert specs[-1]["q"].size == 2000
    ub = 2001 * 20 * factor + 65536
    served = ub < (1 << 22) - 65536
    assert served == (factor == 101)
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 5)))
    assert min(wt["score"] for wt in want) > 1900 * 20 * factor
    # (six queries of 125 stripes: DevRun::build may spread the linear-space and traceback sweeps over CUs; either way)
    _check(eng, sc, specs, want, served=served, tag=("bound", factor), n_im=5, cross={})
    _share(want, "score bound x%d" % factor)


@pytest.mark.parametrize("flank", [300, 9000])
def test_gainful_introns(eng, pool, flank):
    """signals that outweigh the intron penalties (max_s5 + max_s3 + max_pen > 0, fp_gain in DevRun::build): a path may
    gain with every intron it takes, so the bound grows with the window.  A short window stays with spdp_sweep_fp, a
    long one is turned away; either way the scores are the oracle's, and they exceed what matches alone can give"""
    rng = np.random.default_rng(synth.SEED + 9980)
    sc = defaults.scoring(ipen=-100, qm_len=[80, 300, 900, 1200, 1500], qm_pen=[-150, -140, -165, -180, -200], nquant=4)
    specs, gain = [], -(1 << 30)
    for k in range(6):
        g = synth.make_gene(rng, n_exons=5, mrna_len=500, flank=flank, sub=0.0, indel=0.0, intron_hi=1200)
        s5, s3 = synth.splice_signals(g.window)
        # canonical sites inside the gene: +265 .. +330 (the guard looks at the largest signal anywhere in the window;
        # gainful sites all over the flanks would only add hundreds of introns in front of the gene)
        gene = np.zeros(s5.size, bool)
        gene[g.exons[0][0]:g.exons[-1][1] + 1] = True
        s5 = np.where(gene & (s5 > 0), s5 + 250, s5).astype(np.int16)
        s3 = np.where(gene & (s3 > 0), s3 + 250, s3).astype(np.int16)
        specs.append(_spec(defaults.encode(g.query), defaults.encode(g.window), s5, s3, exg=(1, 1, 1, 1) if k & 1 else (0, 0, 0, 0)))
        gain = max(gain, int(s5.max()) + sc.ipen + int(s3.max()) - 140)
    assert gain > 300
    cols = max(s["w"].size for s in specs)
    ub = 501 * 20 + (cols + 1) * gain + 65536
    served = ub < (1 << 22) - 65536
    assert served == (flank == 300), (ub, cols, gain)
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 3)))
    assert all(wt["score"] > 20 * 500 for wt in want), [wt["score"] for wt in want]
    _check(eng, sc, specs, want, served=served, tag=("gain", flank), n_im=3)
    # (gainful sites multiply the paths along the free edges: fewer of these are well defined than of the fuzz's; the
    # linear-space flavour is still compared on two of the six at least -- a property of the oracle's results alone)
    n_def = sum(1 for wt in want if wt["defined"])
    print("gainful introns, flank %d: wip_udh well defined %d of %d" % (flank, n_def, len(want)))
    assert n_def >= 2


@pytest.mark.parametrize("spj", [1, 0])
def test_scores_at_the_floor(eng, pool, spj):
    """global ends on an unrelated pair and on a query of Ns: H runs into SPDP_NEV16 / SPDP_FLOOR16 and stays there
    over hundreds of rows; without splice signals (spj = 0) there is no intron to restart from and the scores end at
    the floor itself.  (The linear-space engine's links are not the reference's own on such paths: score-only and
    traceback are compared on all, wip_udh where it is defined.)"""
    rng = np.random.default_rng(synth.SEED + 9990)
    sc = defaults.scoring(spj=spj)
    specs = []
    for k, exg in enumerate(((0, 0, 0, 0), (0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 1, 1), (0, 0, 0, 0))):
        m = 1200 + 300 * k
        w = synth.random_dna(rng, m + 600 + 200 * k)
        q = np.full(m, ord("N"), np.uint8) if k % 3 == 1 else synth.random_dna(rng, m)
        s5, s3 = synth.splice_signals(w)
        specs.append(_spec(defaults.encode(q), defaults.encode(w), s5, s3, exg=exg))
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", 3)))
    print("floor, spj %d: oracle scores %s" % (spj, [wt["score"] for wt in want]))
    assert sum(1 for wt in want if wt["score"] <= -32768 + 1024) >= 2, [wt["score"] for wt in want]
    _check(eng, sc, specs, want, served=True, tag=("floor", spj), n_im=3)
    print("floor, spj %d: wip_udh well defined %d of %d" % (spj, sum(1 for wt in want if wt["defined"]), len(want)))


# ---- e. the ladder at mid size --------------------------------------------------------------------------------------
def test_mid_size_ladder(eng, pool):
    """alignS_ng with a small MaxVmfSpace on problems of (a): the linear-space branch and the recursion run in the
    multi-wave geometry.  As test_gpu_fuzz.test_fuzz_cdna_ladder: only queries the library marks ALN_LEFT_EDGE itself or
    the oracle cannot restate (NeedsScalarEngine) are left out.  (Round 0, query 5: 2366 rows with a global left end, a
    band shoulder of 30 and random signals -- the score, -31705, sits at the floor, and the top
    linear-space call's chain of links ends on diagonal 0, outside the window 163 .. 687: it started in lanes the
    reference never initialises.  spdp_udh_cpos used to hand that back unmarked, as a two-record list; now it is marked.)"""
    rng = np.random.default_rng(synth.SEED + 9999)
    n_cmp = n_marked = 0
    bad = []
    for rnd in range(3):
        sc = _rand_scoring(rng, served=True)
        sc.max_vmf_space = int(rng.choice([100000, 300000, 1000000, 3000000]))
        specs = [_rand_problem(rng, random_signals=bool(k & 1)) for k in range(16)]
        want = _oracle(pool, sc, specs, ("align",))
        ps = _problem_set(specs)
        for fp in (1, 0):
            with Env(SPDP_FP=fp):
                eng.sweep_stats(reset=True)
                res = eng.align_s(sc, ps, allow_partial=True, with_flags=True)
                st = eng.sweep_stats(reset=True)
            _kernel_check(st, bool(fp), ("ladder", rnd, fp))
            for i, ((score, skl, flags), wt) in enumerate(zip(res, want)):
                if flags & abi.ALN_LEFT_EDGE:
                    n_marked += 1
                    continue
                if wt["align"] is None:
                    continue
                n_cmp += 1
                if score != wt["align"][0] or skl.ravel().tolist() != wt["align"][1]:
                    bad.append((rnd, fp, i, score, wt["align"][0], skl.ravel().tolist()[:8], wt["align"][1][:8]))
    print("ladder: compared %d, marked %d, differ %d" % (n_cmp, n_marked, len(bad)))
    assert not bad, bad
    assert n_cmp > 2 * n_marked and n_cmp >= 48
