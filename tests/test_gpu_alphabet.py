"""Every DP engine against the oracle on whole residue alphabets and substitution matrices that tell mtx[a][b] from
mtx[b][a].  The other files' sequences are A C G T N (codes 2 3 5 9 16) and the twenty amino acids, and their matrices are the
project's own -- symmetric, five distinct values on the nucleotide side; a row / column swap in a kernel's lookup, a code
that lands in another code's slot of spdp_sweep_fp's permuted LDS layout, a short copy of the matrix with two rows exchanged
would all go unseen there.  Here:

  matrices   defaults.NMTX (17 x 17), the same block inside a 32 x 32 matrix (codes 17 .. 31: all of s_perm), and
             data/aa_tron_mtx.npy (23 x 26), each entry moved by a fixed-seed offset |d| <= 9 (planted genes still align,
             scores stay in the range the int16 engines see); row 0 and column 0 stay zero (include/spdp.h).  No two rows
             and no two columns are equal, and no nucleotide entry equals its mirror image: asserted before use
  sequences  the planted genes of test_gpu_fuzz / test_gpu_fp_sweep_oracle with an independent random share of the query's
             and of the window's positions overwritten by codes drawn uniformly from 0 .. dim - 1 (protein: 0 .. rows - 1
             for the query, 0 .. cols - 1 for the tron codes, the stop codes and AMB among them): about 5 % (the paths stay
             gene-shaped) and about 40 %; one query and one window of ambiguity codes only per batch
  signals    independent random arrays, as in test_gpu_fuzz

The oracle is the only judge and every comparison is exact.  Which kernel and which geometry ran is read from
Engine.sweep_stats (test_gpu_fp_sweep_oracle._check).  The linear-space engines are compared where
test_gpu_fuzz._well_defined holds, and at most a third of a test's cases may fall outside it (MEASUREMENTS.md has the
shares)."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from spaln_amd import abi, defaults, synth
from tests.envknobs import Env
from tests.test_gpu_fuzz import _well_defined, _rand_scoring_s, _rand_scoring_h, _with_classes, _ladder_udh_n_im
from tests.test_gpu_fp_sweep_oracle import _spec, _problem_set, _oracle, _check, _kernel_check, _share, _rand_scoring

pytestmark = pytest.mark.gpu

N_WORKERS = max(1, min(16, os.cpu_count() or 1))
LIGHT, HEAVY = 0.05, 0.40
# The linear-space engine's cases: its result is the reference's own only where _well_defined holds, and a path through
# a window that is 40 % random codes, or one with free ends, mostly runs along the edges.  Measured with the oracle alone
# (MEASUREMENTS.md): random end flags skip 54 % at the light share already, global ends 6 %; global ends at 40 % skip 47 %,
# at 20 % 15 %.  So three of four of these cases have global ends, and their heavy share is 15 %.
UDH_HEAVY, UDH_GLOBAL = 0.15, 0.75
ACGT = (2, 3, 5, 9)


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


# ---- matrices -------------------------------------------------------------------------------------------------------
def _offsets(seed, rows, cols):
    d = np.random.default_rng(synth.SEED + 8600 + seed).integers(-9, 10, size=(rows, cols)).astype(np.int32)
    d[0, :] = 0
    d[:, 0] = 0
    return d


def nucleotide_matrix(dim):
    """NMTX + offsets; dim = 32: rows and columns 17 .. 31 continue the N row / column (code 16) before the offsets"""
    idx = np.minimum(np.arange(dim), 16)
    base = defaults.NMTX[np.ix_(idx, idx)].astype(np.int32)
    d = _offsets(dim, dim, dim)
    for a in range(1, dim):                              # a mirror pair the draw left equal: move one of the two by one
        for b in range(a + 1, dim):
            if base[a, b] + d[a, b] == base[b, a] + d[b, a]:
                d[a, b] += 1 if d[a, b] < 9 else -1
    m = base + d
    assert np.abs(m - base).max() <= 9 and not m[0].any() and not m[:, 0].any()
    for a in range(1, dim):
        for b in range(1, dim):
            assert a == b or m[a, b] != m[b, a], (a, b)
    _distinct_rows_and_columns(m)
    return m


def protein_matrix():
    base = np.load(os.path.join(os.path.dirname(os.path.abspath(defaults.__file__)), "data", "aa_tron_mtx.npy")).astype(np.int32)
    assert base.shape == (23, 26) and not base[0].any() and not base[:, 0].any()
    m = base + _offsets(23, *base.shape)
    assert np.abs(m - base).max() <= 9 and not m[0].any() and not m[:, 0].any()
    _distinct_rows_and_columns(m)
    return m


def _distinct_rows_and_columns(m):
    assert len({tuple(r) for r in m.tolist()}) == m.shape[0]
    assert len({tuple(c) for c in m.T.tolist()}) == m.shape[1]


# ---- sequences ------------------------------------------------------------------------------------------------------
def _spray(rng, codes, share, n_codes, lo=0, hi=None):
    """codes[lo:hi] with an independent random share of its positions overwritten by codes drawn from 0 .. n_codes - 1"""
    out = np.array(codes, dtype=np.uint8)
    part = out[lo:hi]
    hit = rng.random(part.size) < share
    part[hit] = rng.integers(0, n_codes, size=int(hit.sum()))
    return out


def _ambiguous_only(rng, n, dim):
    other = np.array([c for c in range(dim) if c not in ACGT], dtype=np.uint8)
    return other[rng.integers(0, other.size, size=n)]


def _problem_s(rng, dim, share, rows=(9, 120), cols_hi=900, kind=None, p_global=0.0):
    """test_gpu_fuzz._rand_problem_s as a spec of test_gpu_fp_sweep_oracle, query and window sprayed; kind = "q" / "w":
    the query / the window holds ambiguity codes only"""
    m = int(rng.integers(*rows))
    n = int(rng.integers(m + 20, max(m + 21, cols_hi)))
    g = synth.make_gene(rng, n_exons=int(rng.integers(1, 4)), mrna_len=max(m, 40), flank=int(rng.integers(10, 80)),
                        intron_hi=int(rng.integers(80, 400)), sub=float(rng.uniform(0, 0.3)))
    w, q = _spray(rng, defaults.encode(g.window), share, dim), _spray(rng, defaults.encode(g.query), share, dim)
    if kind == "q":
        q = _ambiguous_only(rng, q.size, dim)
    if kind == "w":
        w = _ambiguous_only(rng, w.size, dim)
    s5 = rng.integers(-900, 150, size=w.size + 1).astype(np.int16)
    s3 = rng.integers(-900, 150, size=w.size + 1).astype(np.int16)
    al = int(rng.integers(0, max(1, q.size // 4)))
    ar = int(rng.integers(max(al + 9, q.size // 2), q.size + 1))
    bl = int(rng.integers(0, max(1, w.size // 5)))
    br = int(rng.integers(max(bl + (ar - al) + 5, w.size // 2), w.size + 1))
    exg = rng.integers(0, 2, size=4)
    if rng.random() < p_global:
        exg[:] = 0
    return _spec(q, w, s5, s3, al, ar, bl, br, exg)


def _batch_s(rng, dim, n, share, **kw):
    """n problems, the last two with a query / a window of ambiguity codes only"""
    return [_problem_s(rng, dim, share, kind={n - 2: "q", n - 1: "w"}.get(k), **kw) for k in range(n)]


def _mid_problem_s(rng, dim, share, rows_lo, rows_hi, p_global=0.0):
    """test_gpu_fp_sweep_oracle._rand_problem (whole sequences, random signals and end flags), sprayed"""
    m = int(rng.integers(rows_lo, rows_hi + 1))
    g = synth.make_gene(rng, n_exons=int(rng.integers(2, 6)), mrna_len=m, flank=int(rng.integers(m // 5 + 40, m // 5 + 300)),
                        intron_hi=int(rng.integers(200, 1200)), sub=float(rng.uniform(0, 0.2)), indel=0.0)
    w, q = _spray(rng, defaults.encode(g.window), share, dim), _spray(rng, defaults.encode(g.query), share, dim)
    assert rows_lo <= q.size <= rows_hi
    s5 = rng.integers(-900, 150, size=w.size + 1).astype(np.int16)
    s3 = rng.integers(-900, 150, size=w.size + 1).astype(np.int16)
    exg = rng.integers(0, 2, size=4)
    if rng.random() < p_global:
        exg[:] = 0
    return _spec(q, w, s5, s3, exg=exg)


def _scoring_s(rng, dim, local=0):
    sc = _rand_scoring(rng, served=True, mtx=nucleotide_matrix(dim), mtx_dim=dim)
    sc.local = local                                     # (spdp_sweep_fp serves no local run: set once _rand_scoring has asked)
    return sc


# ---- 1. the _wip sweeps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [LIGHT, HEAVY], ids=["light", "heavy"])
@pytest.mark.parametrize("dim", [17, 32])
def test_wip_sweeps(eng, pool, dim, share):
    """wip_scoreonly, wip_forward, wip_udh at the fuzz file's sizes, SPDP_FP=1 (spdp_sweep_fp: sweep_stats says so) and
    SPDP_FP=0 (spdp_kernels.hip); the linear-space engine on a batch of its own (UDH_HEAVY, UDH_GLOBAL)"""
    rng = np.random.default_rng(synth.SEED + 8700 + dim + int(100 * share))
    every = []
    for rnd in range(2):
        sc = _scoring_s(rng, dim)
        specs = _batch_s(rng, dim, 32, share)
        want = _oracle(pool, sc, specs, ("score", "fwd"))
        _check(eng, sc, specs, want, served=True, tag=("wip", dim, share, rnd), engines=("score", "fwd"))
        big = _batch_s(rng, dim, 26, share if share == LIGHT else UDH_HEAVY, rows=(40, 120), p_global=UDH_GLOBAL)
        big = [s for s in big[:-2] if s["ar"] - s["al"] >= 40]
        n_im = int(rng.integers(1, 3))
        want = _oracle(pool, sc, big, ("fwd", ("udh", n_im)))
        every += want
        _check(eng, sc, big, want, served=True, tag=("wip_udh", dim, share, rnd), n_im=n_im, engines=("udh",))
    _share(every, "alphabet wip_udh, dim %d, share %.2f" % (dim, share))


@pytest.mark.parametrize("share", [LIGHT, HEAVY], ids=["light", "heavy"])
@pytest.mark.parametrize("dim", [17, 32])
def test_wip_sweeps_local(eng, pool, dim, share):
    """local = 1: spdp_kernels.hip's local variants whatever SPDP_FP says (spdp_sweep_fp does not serve them).  Score-only
    and traceback only, as test_gpu_fuzz.test_fuzz_cdna_local: the local linear-space sweep (spdp_local_udh.hip) is not called
    as wip_udh here, it runs below alignS_ng in test_ladder_mid_size[*-1]"""
    rng = np.random.default_rng(synth.SEED + 8750 + dim + int(100 * share))
    sc = _scoring_s(rng, dim, local=1)
    specs = _batch_s(rng, dim, 32, share)
    want = _oracle(pool, sc, specs, ("score", "fwd"))
    _check(eng, sc, specs, want, served=False, tag=("wip_local", dim, share), engines=("score", "fwd"))


@pytest.mark.parametrize("dim", [17, 32])
def test_wip_sweeps_mid_size_geometries(eng, pool, dim):
    """problems of 17 stripes and more, where the sweeps run as multi-wave pipelines: the batch as DevRun::build lays it out,
    one wave per problem (SPDP_MULTI=0), 16-wave blocks (SPDP_WPB16=1), and two long queries spread over CUs
    (SPDP_CROSS_WPB=4); light and heavy (UDH_HEAVY: the linear-space engine runs on all of them) problems alternate"""
    rng = np.random.default_rng(synth.SEED + 8800 + dim)
    sc = _scoring_s(rng, dim)
    specs = [_mid_problem_s(rng, dim, UDH_HEAVY if k & 1 else LIGHT, 260, 700, UDH_GLOBAL) for k in range(8)]
    n_im = 3
    want = _oracle(pool, sc, specs, ("score", "fwd", ("udh", n_im)))
    for name, env, b16 in (("mixed", {}, None), ("one_wave", dict(SPDP_MULTI=0), False), ("wpb16", dict(SPDP_WPB16=1), True)):
        _check(eng, sc, specs, want, served=True, tag=("mid", dim, name), n_im=n_im, env=env, blocks16=b16)
    _share(want, "alphabet mid size, dim %d" % dim)
    long_ = [_mid_problem_s(rng, dim, share, 2100, 2400, 1.0) for share in (LIGHT, UDH_HEAVY)]
    want = _oracle(pool, sc, long_, ("fwd", ("udh", 7)))
    _share(want, "alphabet cross-CU, dim %d" % dim)
    cross = {}
    _check(eng, sc, long_, want, served=True, tag=("cross", dim), n_im=7, env=dict(SPDP_CROSS_WPB=4), blocks16=False,
           engines=("fwd", "udh"), cross=cross)
    for k in (("udh", 1), ("udh", 0), ("fwd", 1)):       # laid out across CUs, as test_long_queries_across_cus has it
        assert cross[k][0], (k, cross)
    assert not cross[("fwd", 0)][0]


# ---- 2. the ladders and the exact engines ---------------------------------------------------------------------------
@pytest.mark.parametrize("local", [0, 1])
@pytest.mark.parametrize("dim", [17, 32])
def test_ladder_mid_size(eng, pool, dim, local):
    """alignS_ng with a small MaxVmfSpace at mid size: the linear-space branch and its recursion (local = 1:
    spdp_local_udh.hip).  As test_gpu_fp_sweep_oracle.test_mid_size_ladder: only queries the library marks ALN_LEFT_EDGE
    itself or the oracle cannot restate are left out"""
    rng = np.random.default_rng(synth.SEED + 8850 + dim + local)
    n_cmp = n_marked = 0
    sc = _scoring_s(rng, dim, local=local)
    sc.max_vmf_space = 300000
    specs = [_mid_problem_s(rng, dim, HEAVY if k & 1 else LIGHT, 260, 600) for k in range(10)]
    want = _oracle(pool, sc, specs, ("align",))
    ps = _problem_set(specs)
    for fp in (1, 0):
        with Env(SPDP_FP=fp):
            eng.sweep_stats(reset=True)
            res = eng.align_s(sc, ps, allow_partial=True, with_flags=True)
            st = eng.sweep_stats(reset=True)
        _kernel_check(st, bool(fp) and not local, ("ladder", dim, local, fp))
        for i, ((score, skl, flags), wt) in enumerate(zip(res, want)):
            if flags & abi.ALN_LEFT_EDGE:
                n_marked += 1
                continue
            if wt["align"] is None:
                continue
            n_cmp += 1
            assert score == wt["align"][0] and skl.ravel().tolist() == wt["align"][1], (dim, local, fp, i, score, wt["align"][0])
    print("alphabet ladder, dim %d local %d: compared %d, marked %d" % (dim, local, n_cmp, n_marked))
    assert n_cmp > 2 * n_marked and 3 * (2 * len(specs) - n_cmp) <= 2 * len(specs)       # at most a third of the runs uncompared


def _exact_scoring(rng, dim, **over):
    """test_gpu_fuzz._rand_exact_s (random length-penalty table and junction table) with the perturbed matrix"""
    sc0 = _rand_scoring_s(rng)
    intpen = (-rng.integers(100, 500, size=1200)).astype(np.int16)
    intpen[:int(rng.integers(5, 60))] = -32768 + 1024
    kw = dict(mtx=nucleotide_matrix(dim), mtx_dim=dim, gop=sc0.gop, gep=sc0.gep, ipen=sc0.ipen, llmt=sc0.llmt,
              qm_len=list(sc0.qm_len)[:5], qm_pen=list(sc0.qm_pen)[:5], nquant=sc0.nquant, sh=sc0.sh, intpen=intpen,
              t53=rng.integers(-80, 40, size=256).astype(np.int16), scalar_engines=1)
    kw.update(over)
    return defaults.scoring(**kw)


def _classes(rng, specs):
    return _with_classes(rng, _problem_set(specs))


@pytest.mark.parametrize("noll", [2, 3])
@pytest.mark.parametrize("dim", [17, 32])
def test_a0_engines(eng, dim, noll):
    """scorealoneS_ng, forwardS_ng and hirschbergS_ng (spdp_rowwave.hip, its short copy of the matrix) under random classes,
    length penalties and junction tables; noll = 3: the double affine gap states (-yl3)"""
    from oracle import oracle
    rng = np.random.default_rng(synth.SEED + 8900 + dim + noll)
    over = dict(noll=3, lgop=-int(rng.integers(120, 200)), lgep=-int(rng.integers(2, 8)), codonk1=int(rng.integers(5, 30))) if noll == 3 else {}
    sc = _exact_scoring(rng, dim, **over)
    ps = _classes(rng, _batch_s(rng, dim, 12, LIGHT) + _batch_s(rng, dim, 12, HEAVY))
    assert eng.scalar_scorealone(sc, ps).tolist() == [oracle.scalar_scorealone(sc, p) for p in ps.items]
    for i, ((s, skl), p) in enumerate(zip(eng.scalar_forward(sc, ps), ps.items)):
        ws, wskl = oracle.scalar_forward(sc, p)
        assert s == ws and skl.tolist() == wskl.tolist(), (dim, noll, i)
    n_udh = 0
    n_im, m = 1, 46
    # (the linear-space cases: a batch of their own, as in test_wip_sweeps -- the oracle calls 7 of 19 of the batch above
    #  undefined in the reference, flag -3)
    ups = _classes(rng, _batch_s(rng, dim, 12, LIGHT, rows=(46, 120), p_global=UDH_GLOBAL) +
                   _batch_s(rng, dim, 12, UDH_HEAVY, rows=(46, 120), p_global=UDH_GLOBAL))
    big = abi.ProblemSet()
    big._keep = ups._keep
    for p in ups.items:
        if p.a_right - p.a_left >= m:
            q = abi.Problem.from_buffer_copy(p)
            q.a_right = q.a_left + m                     # one imd_intvl for the batch
            big.items.append(q)
    intvl = (m + n_im) // (n_im + 1)
    scores, cpos, ranges, flags = eng.scalar_udh(sc, big, n_im, intvl)
    for i, p in enumerate(big.items):
        ws, wcpos, wrng, wflag = oracle.scalar_udh(sc, p, n_im, intvl)
        assert int(flags[i]) == wflag, (dim, noll, i)
        if wflag == 0:
            assert int(scores[i]) == ws and ranges[i].tolist() == wrng.tolist() and cpos[i].tolist() == wcpos.tolist(), (dim, noll, i)
            n_udh += 1
    print("alphabet a0, dim %d noll %d: hirschbergS_ng compared %d of %d" % (dim, noll, n_udh, len(big)))
    assert n_udh >= 6 and 3 * (len(big) - n_udh) <= len(big)


@pytest.mark.parametrize("dim", [17, 32])
def test_a1_engines(eng, dim):
    """scoreonlyS1 / forwardS1 (spdp_exact.hip) through HomScoreS_ng and alignS_ng with scalar_engines = 2, as
    test_gpu_noll3_a1 drives them"""
    from oracle import host_logic
    rng = np.random.default_rng(synth.SEED + 8950 + dim)
    sc = _exact_scoring(rng, dim, scalar_engines=2, max_vmf_space=1 << 30)
    ps = _classes(rng, _batch_s(rng, dim, 12, LIGHT) + _batch_s(rng, dim, 12, HEAVY))
    got_s = eng.homscore_s(sc, ps, allow_partial=True)
    res = eng.align_s(sc, ps, allow_partial=True)
    n_cmp = 0
    for i, (p, (score, skl)) in enumerate(zip(ps.items, res)):
        try:
            w = host_logic.align_s(sc, p, simd=1)
        except (host_logic.NeedsScalarEngine, host_logic.ReferenceUndefined):
            continue
        n_cmp += 1
        assert score == w[0] and skl.ravel().tolist() == (w[1] or []), (dim, i, score, w[0])
        assert int(got_s[i]) == host_logic.homscore_s(sc, p, simd=1), (dim, i)
    print("alphabet a1, dim %d: compared %d of %d" % (dim, n_cmp, len(ps)))
    assert 3 * (len(ps) - n_cmp) <= len(ps)


# ---- 3. protein x genome --------------------------------------------------------------------------------------------
def _scoring_h(rng, local=0, **over):
    sc0 = _rand_scoring_h(rng, local)
    m = protein_matrix()
    kw = dict(mtx=m, mtx_rows=m.shape[0], mtx_cols=m.shape[1], gop=sc0.gop, gep=sc0.gep, gapw1=sc0.gapw1, gapw2=sc0.gapw2,
              gapw3=sc0.gapw3, ipen=sc0.ipen, llmt=sc0.llmt, qm_len=list(sc0.qm_len)[:5], qm_pen=list(sc0.qm_pen)[:5],
              nquant=sc0.nquant, sh=sc0.sh, term_codon=sc0.term_codon, local=local)
    kw.update(over)
    return defaults.scoring_h(**kw)


def _problem_h(rng, ps, sc, share, kind=None):
    """test_gpu_fuzz._rand_problem_h with the query sprayed over 0 .. mtx_rows - 1 and the window's tron codes over
    0 .. mtx_cols - 1 (X, AMB, the AGY serines and both stop codes among them); kind as in _problem_s"""
    aa = int(rng.integers(10, 90))
    g = synth.make_protein_gene(rng, n_exons=int(rng.integers(1, 4)), aa_len=aa, flank=int(rng.integers(10, 120)),
                                sub=float(rng.uniform(0, 0.4)), intron_hi=int(rng.integers(80, 400)))
    sg = synth.protein_signals(g.window, rng)
    L = g.window.size
    q = _spray(rng, synth.encode_protein(g.query), share, sc.mtx_rows)
    b = _spray(rng, sg["b"], share, sc.mtx_cols, 1, L - 1)          # (index 0 and the last two stay the sequence's pads)
    if kind == "q":
        q[:] = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=q.size)          # nil, gap, X
    if kind == "w":
        b[1:L - 1] = rng.choice(np.array([0, 1, 2, 24, 25], dtype=np.uint8), size=L - 2)   # nil, gap, AMB, the stop codes
    al = int(rng.integers(0, max(1, q.size // 4)))
    ar = int(rng.integers(max(al + 9, q.size // 2), q.size + 1))
    bl = int(rng.integers(0, max(1, L // 5)))
    br = int(rng.integers(max(bl + 3 * (ar - al) // 2, L // 2), L + 1))
    exg = tuple(int(x) for x in rng.integers(0, 2, size=4))
    return ps.add(q, b, sg["sig5"], sg["sig3"], sg["sigS"], sg["sigT"], sg["sigE"], sg["phs5"], sg["phs3"],
                  al, ar, bl, br, exg, exin=(0, L))


def _batch_h(rng, sc, n, min_rows=0):
    """n problems, light and heavy alternating, the last two with a query / a window of ambiguity codes only"""
    ps = abi.ProblemSetH()
    while len(ps) < n:
        k = len(ps)
        p = _problem_h(rng, ps, sc, HEAVY if k & 1 else LIGHT, kind={n - 2: "q", n - 1: "w"}.get(k) if not min_rows else None)
        if p.a_right - p.a_left < min_rows:
            ps.items.pop()
    return ps


FLAGMAP = {0: 0, -2: -1, -3: -2}


@pytest.mark.parametrize("local", [0, 1])
def test_protein_forward(eng, local):
    from oracle import oracle
    rng = np.random.default_rng(synth.SEED + 9010 + local)
    for rnd in range(2):
        sc = _scoring_h(rng, local)
        ps = _batch_h(rng, sc, 32)
        for i, ((s, skl, flag), p) in enumerate(zip(eng.wip_forward_h(sc, ps), ps.items)):
            ws, wskl, wflag = oracle.wip_forward_h(sc, p)
            assert s == ws and flag == FLAGMAP[wflag], (local, rnd, i, s, ws)
            if wflag == 0:
                assert skl.tolist() == wskl.tolist(), (local, rnd, i)


def test_protein_udh(eng):
    from oracle import oracle
    rng = np.random.default_rng(synth.SEED + 9020)
    n_empty = n_full = 0
    for rnd in range(3):
        sc = _scoring_h(rng)
        ps = _batch_h(rng, sc, 24, min_rows=34)
        n_im = int(rng.integers(1, 3))
        us, ucpos, urng = eng.wip_udh_h(sc, ps, n_im)
        for i, p in enumerate(ps.items):
            ws, wcpos, wrng = oracle.wip_udh_h(sc, p, n_im)
            fs, fskl, fflag = oracle.wip_forward_h(sc, p)
            if fflag != 0 or not _well_defined(wrng, wcpos, fskl, 3):
                n_empty += 1
                continue
            n_full += 1
            assert int(us[i]) == ws and urng[i].tolist() == wrng.tolist(), (rnd, i)
            assert ucpos[i].tolist() == wcpos.tolist(), (rnd, i)
    print("alphabet wip_udh_h: well defined %d of %d (%.0f %% skipped)" % (n_full, n_full + n_empty, 100.0 * n_empty / (n_full + n_empty)))
    assert n_full > n_empty and 3 * n_empty <= n_full + n_empty


def test_protein_ladder(eng):
    """alignH_ng with a small MaxVmfSpace, as test_gpu_fuzz.test_fuzz_protein_ladder"""
    from oracle import oracle, host_logic_h as hh
    rng = np.random.default_rng(synth.SEED + 9030)
    n_cmp = n_skip = 0
    for rnd in range(2):
        sc = _scoring_h(rng)
        sc.max_vmf_space = int(rng.choice([20000, 60000]))
        ps = _batch_h(rng, sc, 32)
        res = eng.align_h(sc, ps)
        for i, (p, (score, skl, flag)) in enumerate(zip(ps.items, res)):
            m, n = p.a_right - p.a_left, p.b_right - p.b_left
            k = _ladder_udh_n_im(sc, m, n, 3)
            if k != 0 and m >= 17:
                ws, wcpos, wrng = oracle.wip_udh_h(sc, p, max(k, 1))
                fs, fskl, fflag = oracle.wip_forward_h(sc, p)
                if fflag != 0 or not _well_defined(wrng, wcpos, fskl, 3):
                    n_skip += 1
                    continue
            try:
                wscr, wskl = hh.align_h(sc, p)
                wflag = 0
            except hh.ReferenceUndefined:
                wflag = -2
            except hh.ReferenceFatal:
                wflag = -1
            except hh.NotRestated:
                wflag = 1
            n_cmp += 1
            assert flag == wflag, (rnd, i, flag, wflag)
            if wflag == 0:
                assert score == wscr and skl.ravel().tolist() == (wskl or []), (rnd, i, score, wscr)
    print("alphabet protein ladder: compared %d, skipped %d" % (n_cmp, n_skip))
    assert n_cmp > n_skip and 3 * n_skip <= n_cmp + n_skip


def test_protein_a0_engines(eng):
    """forwardH_ng (score-only and records) and hirschbergH_ng (spdp_h_rowwave.hip), as test_fuzz_protein_a0_engines"""
    from oracle import oracle
    rng = np.random.default_rng(synth.SEED + 9040)
    n_udh = n_big = 0
    for rnd in range(2):
        sc = _scoring_h(rng, intpen=(-rng.integers(100, 500, size=1500)).astype(np.int16),
                        t53=rng.integers(-80, 40, size=256).astype(np.int16), scalar_engines=1, minl=int(rng.integers(20, 60)),
                        gape1=-int(rng.integers(100, 400)), gape2=-int(rng.integers(100, 400)), extragop=-int(rng.integers(0, 200)))
        ps = _batch_h(rng, sc, 24)
        for k, p in enumerate(ps.items):
            dc = rng.integers(0, 256, size=p.b_len + 3).astype(np.uint8)
            ps._keep.append(dc)
            p.dinc = dc.ctypes.data
            ps.items[k] = p
        for tb in (False, True):
            res = eng.scalar_forward_h(sc, ps, traceback=tb)
            for i, ((s, skl), p) in enumerate(zip(res, ps.items)):
                ws, wskl = oracle.scalar_forward_h(sc, p, traceback=tb)
                assert s == ws, (rnd, tb, i, s, ws)
                if tb:
                    assert skl.tolist() == wskl.tolist(), (rnd, i)
        n_im, m = 1, 36
        big = abi.ProblemSetH()
        big._keep = ps._keep
        for p in ps.items:
            if p.a_right - p.a_left >= m:
                q = abi.ProblemH.from_buffer_copy(p)
                q.a_right = q.a_left + m
                big.items.append(q)
        intvl = (m + n_im) // (n_im + 1)
        scores, cpos, ranges, flags = eng.scalar_udh_h(sc, big, n_im, intvl)
        n_big += len(big)
        for i, p in enumerate(big.items):
            ws, wcpos, wrng, wflag = oracle.scalar_udh_h(sc, p, n_im, intvl)
            assert int(flags[i]) == wflag, (rnd, i)
            if wflag == 0:
                assert int(scores[i]) == ws and ranges[i].tolist() == wrng.tolist() and cpos[i].tolist() == wcpos.tolist(), (rnd, i)
                n_udh += 1
    print("alphabet protein a0: hirschbergH_ng compared %d of %d" % (n_udh, n_big))
    assert n_udh >= 8 and 3 * (n_big - n_udh) <= n_big
