"""The rescoring kernels (spdp_rescore_s = skl_rngS_ng, spdh_rescore = skl_rngH_ng, spaln_amd/csrc/spdp_rescore.hip) against the
oracle's restatements on the cases of tests/rescore_cases.py: total score, the five FSTAT numbers and all 21 columns of every
record, integer for integer.  Beside the recipes' corner lists: the batch layout (compaction of entries without an alignment,
offsets across problems of different sizes, a second and third block of 64 threads, pool blocks reused by a smaller call), the
protein walk's region window against whole regions, condensed lists that fill their record slot inside a batch, the aligners'
own lists, and the edit records' properties (tests/test_rescore_cases.py tries those on the reference's records first)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from spaln_amd import abi
from tests import rescore_cases as rc
from tests.test_rescore_cases import (cigar_properties, vulgar_properties, cigar_properties_h, vulgar_properties_h, intron_gaps_h,
                                      _exons)

pytestmark = pytest.mark.gpu

NO_ALIGNMENT = (rc.NEVSEL, [0, 0, 0, 0, 0], [])


@pytest.fixture(scope="module")
def eng():
    from spaln_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


def _scoring(walk):
    return rc.params_s()[1] if walk == "s" else rc.params_h()[0]


def _rescore(eng, walk, cases, lists, kw):
    """one call of spdp_skl_rng_s / _h for a batch; lists[i]: rows with the header first, or None for a null SpdpAlignment.skl
    with a count that claims corners"""
    ps = abi.ProblemSet() if walk == "s" else abi.ProblemSetH()
    for c in cases:
        c.add_to(ps)
    n = len(cases)
    arr, keep = (abi.Alignment * n)(), []
    for i, skl in enumerate(lists):
        if skl is None:
            arr[i].n_skl, arr[i].skl = 5, None
            continue
        skl = np.ascontiguousarray(skl, dtype=np.int32).reshape(-1, 2)
        keep.append(skl)
        arr[i].n_skl, arr[i].skl = skl.shape[0], C.cast(skl.ctypes.data, C.POINTER(abi.Skl))
    out = (abi.Rescored * n)()
    if walk == "s":
        rp = abi.RescoreParams(int(kw["codonk1"]), int(kw["minl"]), int(kw["jneibr"]), int(kw["lsg"]))
        fn, what = eng.lib.spdp_skl_rng_s, "spdp_skl_rng_s"
    else:
        hk = rc.params_h()[1]
        rp = abi.RescoreParamsH(int(hk["minl"]), int(kw["jneibr"]), int(hk["lcl"]), int(kw.get("sup_tcodon", 0)))
        fn, what = eng.lib.spdp_skl_rng_h, "spdp_skl_rng_h"
    sc = _scoring(walk) if walk == "s" else rc.params_h(kw.get("codonk1"))[0]
    eng._check(fn(eng.ctx, C.byref(sc), C.byref(rp), ps.array(), n, arr, out), what)
    res = []
    for i in range(n):
        k = out[i].n_exons
        ex = np.ctypeslib.as_array(C.cast(out[i].exons, C.POINTER(C.c_int32)), shape=(k, 21)).tolist() if k else []
        res.append((int(out[i].score), [out[i].mch, out[i].mmc, out[i].gap, out[i].unp, out[i].val], ex))
    eng.lib.spdp_free_rescored(out, n)
    return res


def _groups(walk):
    """the cases with a corner list, by the keywords one call shares"""
    out = {}
    for c in rc.cases(walk):
        if c.corners is not None:
            out.setdefault(tuple(sorted(c.kw.items())), []).append(c)
    return out


def _mismatches(cases, got, want):
    return [(c.name, c.recipe, g[0], w[0], g[1], w[1], len(g[2]), len(w[2])) for c, g, w in zip(cases, got, want) if tuple(g) != tuple(w)]


def test_cdna_cases(eng):
    want = rc.expected("s")
    n = 0
    for key, cases in _groups("s").items():
        got = _rescore(eng, "s", cases, [c.rows() for c in cases], dict(key))
        bad = _mismatches(cases, got, [want[c.name] for c in cases])
        assert not bad, bad[:4]
        n += len(cases)
    assert n == len(want)


@pytest.mark.parametrize("window", ["windowed", "whole"])
def test_protein_cases(eng, monkeypatch, window):
    """the default (the corners' span and a margin on the device) and SPDP_RESCORE_WINDOW=0 (whole regions): both equal the oracle; a
    refused read outside the window fails the call, and with it the test"""
    if window == "whole":
        monkeypatch.setenv("SPDP_RESCORE_WINDOW", "0")
    else:
        monkeypatch.delenv("SPDP_RESCORE_WINDOW", raising=False)
    want = rc.expected("h")
    n = 0
    for key, cases in _groups("h").items():
        got = _rescore(eng, "h", cases, [c.rows() for c in cases], dict(key))
        bad = _mismatches(cases, got, [want[c.name] for c in cases])
        assert not bad, bad[:4]
        n += len(cases)
    assert n == len(want)


def _mixed(walk, n, jneibr):
    """n entries of mixed sizes under one jneibr, every fifth without an alignment (one corner only, or a null list); the oracle's
    answer for each"""
    first = rc.cases(walk)[0].kw
    pool = [c for c in rc.cases(walk) if c.corners is not None and {**c.kw, "jneibr": 0} == {**first, "jneibr": 0}]      # what one call shares
    stride = next(q for q in (37, 41, 43, 47) if len(pool) % q)       # through all the recipes, whatever their number
    cases, lists, want = [], [], []
    for i in range(n):
        c = pool[(i * stride) % len(pool)]
        c = dataclasses.replace(c, kw=dict(c.kw, jneibr=jneibr))
        cases.append(c)
        if n > 1 and i % 5 == 2:
            lists.append(c.rows()[:2] if i % 2 else None)
            want.append(NO_ALIGNMENT)
        else:
            lists.append(c.rows())
            want.append(rc.oracle_of(c))
    return cases, lists, want


@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("walk", ["s", "h"])
def test_batches(eng, walk, n):
    cases, lists, want = _mixed(walk, n, 10)
    assert n == 1 or len({c.arrays["b"].size for c in cases}) > 10
    got = _rescore(eng, walk, cases, lists, cases[0].kw)
    bad = _mismatches(cases, got, want)
    assert not bad, bad[:4]
    assert n == 1 or sum(w is NO_ALIGNMENT for w in want) >= n // 6


@pytest.mark.parametrize("walk", ["s", "h"])
def test_small_call_after_a_large_one(eng, walk):
    """the pool blocks of a 130-problem call serve a 3-problem call"""
    cases, lists, want = _mixed(walk, 130, 2)
    assert not _mismatches(cases, _rescore(eng, walk, cases, lists, cases[0].kw), want)
    few = [127, 5, 64]
    got = _rescore(eng, walk, [cases[i] for i in few], [cases[i].rows() for i in few], cases[0].kw)
    assert not _mismatches([cases[i] for i in few], got, [rc.oracle_of(cases[i]) for i in few])


@pytest.mark.parametrize("walk", ["s", "h"])
def test_alone_and_in_a_batch(eng, walk):
    cases, lists, want = _mixed(walk, 65, 32)
    got = _rescore(eng, walk, cases, lists, cases[0].kw)
    for i in (0, 1, 63, 64):
        if lists[i] is None or len(lists[i]) < 3:
            continue
        alone, = _rescore(eng, walk, [cases[i]], [lists[i]], cases[0].kw)
        assert tuple(alone) == tuple(got[i]) == tuple(want[i]), cases[i].name


def test_condensed_lists_at_the_bound_inside_a_batch(eng):
    """lists whose every step closes an exon (as many records as corners: beyond the `corners / 2 + 3` rows of the slot of old) between
    neighbours in a 65-problem call: the list's own result and both neighbours'"""
    bound = [c for c in rc.cases("s") if c.recipe == "bound"]
    cases, lists, want = _mixed("s", 65, 10)
    at = (3, 33, 63, 64)
    for i, c in zip(at, bound):
        c = dataclasses.replace(c, kw=dict(c.kw, jneibr=10))
        cases[i], lists[i], want[i] = c, c.rows(), rc.oracle_of(c)
        assert len(want[i][2]) == len(c.corners)
    assert max(len(want[i][2]) - (len(cases[i].corners) // 2 + 3) for i in at) >= 3
    got = _rescore(eng, "s", cases, lists, cases[0].kw)
    for i in at:
        for j in (i - 1, i, i + 1):
            if j < 65:
                assert tuple(got[j]) == tuple(want[j]), (i, j, cases[j].name)
    assert not _mismatches(cases, got, want)


def test_aligners_lists_cdna(eng):
    """spdp_align_s under -A2 and -A0, then the walk on what it returned, a batch per call"""
    from oracle import host_logic
    from tests import spdg
    from spaln_amd import defaults
    cases = [c for c in rc.cases("s") if c.corners is None]
    fx, sc, kw = rc.params_s()
    intpen, t53 = defaults.exact_tables()
    n = 0
    for scalar in (0, 1):
        sca = spdg.scoring(fx, intpen=intpen, t53=t53, scalar_engines=scalar)
        ps = abi.ProblemSet()
        for c in cases:
            c.add_to(ps)
        aln = [skl for _, skl in eng.align_s(sca, ps)]
        kwc = dict(kw, jneibr=10)
        res = eng.skl_rng_s(sc, ps, aln, **kwc)
        for c, p, skl, (score, fst, ex) in zip(cases, ps.items, aln, res):
            if len(skl) < 3:
                assert score == rc.NEVSEL and len(ex) == 0
                continue
            wh, wfst, wrecs = host_logic.skl_rng_s(sc, p, [int(x) for x in skl.ravel()], **kwc)
            assert (score, fst, ex.tolist()) == (wh, wfst, wrecs), (c.name, scalar)
            n += 1
    assert n >= 16


def test_aligners_lists_protein(eng):
    from oracle import host_logic_h
    cases = [c for c in rc.cases("h") if c.corners is None]
    sc, hk = rc.params_h()
    ps = abi.ProblemSetH()
    for c in cases:
        c.add_to(ps)
    res = eng.align_h(sc, ps)
    aln = [skl if flag == 0 else np.zeros((0, 2), dtype=np.int32) for _, skl, flag in res]
    got = eng.skl_rng_h(sc, ps, aln, minl=hk["minl"], jneibr=10, lcl=hk["lcl"], sup_tcodon=0)
    n = 0
    for c, p, skl, (score, fst, ex) in zip(cases, ps.items, aln, got):
        if len(skl) < 3:
            continue
        flat = [int(x) for x in skl.ravel()]
        pts = list(zip(flat[2::2], flat[3::2]))
        p5, p3 = c.arrays["phs5"], c.arrays["phs3"]
        if any(m1 == m0 and p5[n0] == 2 and p3[n1] == 2 for (m0, n0), (m1, n1) in zip(pts, pts[1:])):
            continue                                     # the GTGT....AGAG junction: no fixture pins the oracle there
        want = host_logic_h.skl_rng_h(sc, p, flat, dinc=c.arrays["dinc"], **{**hk, "jneibr": 10})
        assert (score, fst, ex.tolist()) == tuple(want), c.name
        n += 1
    assert n >= 4


def test_edit_records_cdna(eng):
    """spdp_skl_edits_s on every list whose four end-gap flags are 0, condensed ones included: no slot overflows, the N lengths and
    the 5 / I / 3 triples are the exon records' gaps, SAM's clips and header fields are the list's ends"""
    want = rc.expected("s")
    n = n_introns = 0
    for key, cases in _groups("s").items():
        cases = [c for c in cases if c.exg == (0, 0, 0, 0)]
        if not cases:
            continue
        ps = abi.ProblemSet()
        for c in cases:
            c.add_to(ps)
        lists = [c.rows() for c in cases]
        sc = _scoring("s")
        cig = eng.skl_edits_s(sc, ps, lists, abi.FMT_CIGAR, **dict(key))
        vul = eng.skl_edits_s(sc, ps, lists, abi.FMT_VULGAR, **dict(key))
        sam = eng.skl_edits_s(sc, ps, lists, abi.FMT_SAM, **dict(key))
        for c, (cg, _), (vl, _), (sm, hdr) in zip(cases, cig, vul, sam):
            ex = _exons(want[c.name][2])
            cigar_properties(cg[:, :2], ex)
            vulgar_properties(vl, ex)
            (m0, n0), (m1, _) = c.corners[0], c.corners[-1]
            a_len = c.arrays["a"].size
            clips = [(k, int(r[1])) for k, r in enumerate(sm) if chr(r[0]) == "H"]
            assert clips == ([(0, m0)] if m0 else []) + ([(len(sm) - 1, a_len - m1)] if m1 < a_len else []), c.name
            assert (hdr[0], hdr[1], hdr[3], hdr[4]) == (0, n0, m0, m1), c.name
            fst = want[c.name][1]
            assert hdr[2] == 30 + 100 * (fst[1] + fst[3]) // max(1, a_len), c.name
            n += 1
            n_introns += len(ex) - 1
    assert n >= 100 and n_introns >= 100


def test_edit_records_protein(eng):
    """spdp_skl_edits_h on every protein list, condensed ones included: no "edit records: slot too small" (the call fails on it);
    on the lists whose four end-gap flags are 0 the properties tests/test_rescore_cases.py found the reference's records to have.
    Left out of those: the lists on which an accepted intron closes an exon of at most one nucleotide, which gets no record
    (h_back_to_back, the donor-side h_edge): the properties speak of the gaps between records"""
    want = rc.expected("h")
    n = n_introns = n_fs = n_split = 0
    for key, cases in _groups("h").items():
        kw = dict(key)
        ps = abi.ProblemSetH()
        for c in cases:
            c.add_to(ps)
        hk = rc.params_h()[1]
        sc = rc.params_h(kw.get("codonk1"))[0]
        out = {}
        for fmt in (abi.FMT_CIGAR, abi.FMT_VULGAR):
            out[fmt] = eng.skl_edits_h(sc, ps, [c.rows() for c in cases], fmt, minl=hk["minl"], jneibr=kw["jneibr"], lcl=hk["lcl"],
                                       sup_tcodon=kw.get("sup_tcodon", 0))
            assert len(out[fmt]) == len(cases) and all(len(o) for o in out[fmt])
        for c, cg, vl in zip(cases, out[abi.FMT_CIGAR], out[abi.FMT_VULGAR]):
            if c.exg != (0, 0, 0, 0) or c.recipe == "h_back_to_back" or (c.recipe == "h_edge" and c.info["side"] == 0):
                continue
            ex = _exons(want[c.name][2])
            try:
                cigar_properties_h(cg[:, :2], ex)
                vulgar_properties_h(vl, ex)
            except AssertionError as e:
                raise AssertionError((c.name, cg.tolist(), vl.tolist(), [r[:2] + r[16:19] for r in ex])) from e
            n += 1
            n_introns += len(intron_gaps_h(ex))
            n_fs += int((vl[:, 0] == ord("F")).sum())
            n_split += int((vl[:, 0] == ord("S")).sum())
    assert n >= 150 and n_introns >= 100 and n_fs >= 40 and n_split >= 2, (n, n_introns, n_fs, n_split)
