"""The unspliced aligner on the device (spdp_align_b / spdp_homscore_b + the host rescoring) against the program's recorded
output (tests/golden/b_aa_*.json.gz) and the restatement (tests/unspliced_ref).  Every test is one batch or a few."""
import itertools

import numpy as np
import pytest

from spaln_amd import abi, defaults, engine
from tests import unspliced_cases as uc
from tests import unspliced_ref as ubr

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200]


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def check_against_restatement(got, sc, up, ps, what):
    for i, ((score, skl), p) in enumerate(zip(got, ps.items)):
        wscore, wskl = ubr.align(sc, up, p)
        assert score == wscore and skl.tolist() == wskl.tolist(), (what, i, score, wscore, skl.tolist(), wskl.tolist())


def fixture_batch(eng, names):
    """all option sets of the named fixture files: one align_b call per option set"""
    for name in names:
        for k in range(len(uc.load(name)["runs"])):
            sc, up, ps, recs = uc.problems(name, k)
            yield name, k, sc, up, ps, recs, eng.align_b(sc, up, ps)


def test_fixtures_equal_the_programs_records(eng):
    for name, k, sc, up, ps, recs, got in fixture_batch(eng, [n for n in uc.SETS if n != "local"]):
        stats = eng.skl_rng_b(sc, up, ps, [s for _, s in got])
        cig = eng.skl_edits_b(sc, up, ps, [s for _, s in got], abi.FMT_CIGAR)
        for i, ((score, skl), st, rec) in enumerate(zip(got, stats, recs)):
            uc.check_record(st, skl[st["first"]:st["first"] + st["n_trim"]], rec, (name, k, i))
            assert [[chr(o), int(l)] for o, l, _ in cig[i][0]] == (rec["cigar"] or [])
            assert score == ubr.align(sc, up, ps.items[i])[0], (name, k, i)
        if up.tgapf == 1.0:
            hom = eng.homscore_b(sc, up, ps)
            assert hom.tolist() == [s for s, _ in got], (name, k)


def random_pairs(rng, n, alphabet=20, base=3):
    out = []
    for i in range(n):
        la = LENGTHS[int(rng.integers(0, len(LENGTHS)))]
        a = rng.integers(base, base + alphabet, size=la).astype(np.uint8)
        if rng.random() < 0.7:          # a relative of a: substitutions, one insertion or deletion
            b = a.copy()
            hit = rng.random(la) < 0.2
            b[hit] = rng.integers(base, base + alphabet, size=int(hit.sum()))
            if la > 4 and rng.random() < 0.6:
                at, d = int(rng.integers(0, la - 2)), int(rng.integers(1, 10))
                b = np.concatenate([b[:at], rng.integers(base, base + alphabet, size=d).astype(np.uint8), b[at:]]) if rng.random() < 0.5 else \
                    np.concatenate([b[:at], b[min(la, at + d):]])
            if b.size == 0:
                b = a[:1].copy()
        else:
            b = rng.integers(base, base + alphabet, size=LENGTHS[int(rng.integers(0, len(LENGTHS)))]).astype(np.uint8)
        out.append((a, b))
    return out


@pytest.mark.parametrize("noll,sh", [(n, s) for n in (2, 3) for s in (5, 100, -10)])
def test_random_batch_against_the_restatement_in_chunks(eng, noll, sh):
    """400 pairs in one batch: the lengths around the tile edges crossed with every end-flag combination, per gap model and
    band shoulder; neighbours in the batch differ in length; the trace budget cuts the batch into at least 3 chunks"""
    rng = np.random.default_rng(20)
    exgs = list(itertools.product((0, 1), repeat=4))
    sc = defaults.scoring_b(noll=noll, sh=sh)
    ps = abi.ProblemSet()
    for j, (a, b) in enumerate(random_pairs(rng, 400)):
        ps.add(a, b, None, None, exg=exgs[j % 16])
    need = [eng.trace_bytes_b(p, sh) for p in ps.items]
    budget = max(max(need), sum(need) // 4)
    assert sum(need) >= 3 * budget
    up = abi.UnsplicedParams(1.0, int(budget))
    got = eng.align_b(sc, up, ps)
    check_against_restatement(got, sc, up, ps, (noll, sh))
    hom = eng.homscore_b(sc, up, ps)
    assert hom.tolist() == [ubr.scorealone(sc, up, p) for p in ps.items], (noll, sh)


def test_local_ends(eng):
    for name, k, sc, up, ps, recs, got in fixture_batch(eng, ["local"]):
        stats = eng.skl_rng_b(sc, up, ps, [s for _, s in got])
        for i, ((score, skl), st, rec) in enumerate(zip(got, stats, recs)):
            uc.check_record(st, skl[st["first"]:st["first"] + st["n_trim"]], rec, (name, k, i))
        check_against_restatement(got, sc, up, ps, (name, k))
        assert eng.homscore_b(sc, up, ps).tolist() == [ubr.scorealone(sc, up, p) for p in ps.items]
    rng = np.random.default_rng(21)
    for noll in (2, 3):
        sc = defaults.scoring_b(noll=noll, local=1)
        # a matrix with negative mismatches: local optima that are proper sub-alignments, and empty ones
        m = np.full((23, 23), -30, dtype=np.int32)
        m[np.arange(23), np.arange(23)] = 40
        sc = defaults.scoring_b(noll=noll, local=1, mtx=m)
        ps = abi.ProblemSet()
        for a, b in random_pairs(rng, 50):
            ps.add(a, b, None, None, exg=(1, 1, 1, 1))
        ps.add(np.array([3, 4, 5], dtype=np.uint8), np.array([6, 7, 8, 9], dtype=np.uint8), None, None, exg=(1, 1, 1, 1))
        up = abi.UnsplicedParams(1.0, 0)
        got = eng.align_b(sc, up, ps)
        check_against_restatement(got, sc, up, ps, ("local", noll))
        assert got[-1][0] == abi.NEVSEL and got[-1][1].shape[0] == 0          # nothing positive: no alignment
        assert eng.homscore_b(sc, up, ps).tolist() == [ubr.scorealone(sc, up, p) for p in ps.items]


def test_degenerate_ranges(eng):
    rng = np.random.default_rng(22)
    a = rng.integers(3, 23, size=150).astype(np.uint8)
    b = np.concatenate([rng.integers(3, 23, size=20).astype(np.uint8), a[30:120], rng.integers(3, 23, size=25).astype(np.uint8)])
    for noll, sh in ((2, 100), (3, 0), (2, 3)):
        sc = defaults.scoring_b(noll=noll, sh=sh)
        up = abi.UnsplicedParams(1.0, 0)
        ps = abi.ProblemSet()
        for exg in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0)):
            ps.add(a, b, None, None, a_left=40, a_right=40, b_left=10, b_right=60, exg=exg)        # no rows
            ps.add(a, b, None, None, a_left=20, a_right=90, b_left=33, b_right=33, exg=exg)        # no columns
            ps.add(a, b, None, None, a_left=40, a_right=40, b_left=10, b_right=10, exg=exg)        # neither
            ps.add(a, b, None, None, a_left=30, a_right=120, b_left=20, b_right=110, exg=exg)      # sh = 0: one diagonal
            ps.add(a, b, None, None, a_left=25, a_right=131, b_left=11, b_right=118, exg=exg)      # sub-ranges inside
            ps.add(a, b, None, None, a_left=0, a_right=150, b_left=7, b_right=135, exg=exg)
            ps.add(a, b, None, None, a_left=64, a_right=129, b_left=50, b_right=51, exg=exg)       # one column
            ps.add(a, b, None, None, a_left=64, a_right=65, b_left=1, b_right=130, exg=exg)        # one row
        got = eng.align_b(sc, up, ps)
        check_against_restatement(got, sc, up, ps, (noll, sh))


def test_problem_above_the_budget_is_not_computed(eng):
    rng = np.random.default_rng(23)
    sc = defaults.scoring_b()
    ps = abi.ProblemSet()
    small = random_pairs(rng, 12)
    big = rng.integers(3, 23, size=600).astype(np.uint8)
    for j, (a, b) in enumerate(small):
        if j == 5:
            ps.add(big, big[::-1].copy(), None, None, exg=(0, 0, 0, 0))
        ps.add(a, b, None, None, exg=(0, 0, 0, 0))
    need = [eng.trace_bytes_b(p, sc.sh) for p in ps.items]
    budget = sorted(need)[-2]
    assert need[5] > budget
    up = abi.UnsplicedParams(1.0, int(budget))
    with pytest.raises(RuntimeError):
        eng.align_b(sc, up, ps)
    got = eng.align_b(sc, up, ps, allow_partial=True)
    assert got[5][0] == abi.NEVSEL and got[5][1].shape[0] == 0
    for i, p in enumerate(ps.items):
        if i != 5:
            wscore, wskl = ubr.align(sc, up, p)
            assert got[i][0] == wscore and got[i][1].tolist() == wskl.tolist()


def test_nucleotide_batch(eng):
    rng = np.random.default_rng(24)
    for noll in (2, 3):
        sc = abi.make_scoring(mtx=defaults.NMTX, mtx_dim=defaults.NSIMD, gop=defaults.GOP, gep=defaults.GEP, lgop=defaults.LGOP,
                              lgep=defaults.LGEP, noll=noll, spj=0, scalar_engines=1, sh=30, codonk1=7)
        codes = np.array([2, 3, 5, 9], dtype=np.uint8)
        ps = abi.ProblemSet()
        for j, (a, b) in enumerate(random_pairs(rng, 60, alphabet=4, base=0)):
            ps.add(codes[a], codes[b], None, None, exg=((j >> 0) & 1, (j >> 1) & 1, (j >> 2) & 1, (j >> 3) & 1))
        up = abi.UnsplicedParams(1.0, 0)
        check_against_restatement(eng.align_b(sc, up, ps), sc, up, ps, ("dna", noll))
        assert eng.homscore_b(sc, up, ps).tolist() == [ubr.scorealone(sc, up, p) for p in ps.items]


@pytest.mark.parametrize("tgapf", [0.5, 0.0])
def test_terminal_gap_factor(eng, tgapf):
    rng = np.random.default_rng(25)
    exgs = list(itertools.product((0, 1), repeat=4))
    for noll in (2, 3):
        sc = defaults.scoring_b(noll=noll, sh=20)
        ps = abi.ProblemSet()
        for j, (a, b) in enumerate(random_pairs(rng, 64)):
            ps.add(a, b, None, None, exg=exgs[j % 16])
        up = abi.UnsplicedParams(tgapf, 0)
        check_against_restatement(eng.align_b(sc, up, ps), sc, up, ps, (tgapf, noll))


def test_bundles_are_refused_by_name(eng):
    sc, up, ps, _ = uc.problems("shapes1", 0)
    for field, value in (("spj", 1), ("scalar_engines", 0)):
        with pytest.raises(RuntimeError, match=field):
            eng.align_b(defaults.scoring_b(**{field: value}), up, ps)
        with pytest.raises(RuntimeError, match=field):
            eng.homscore_b(defaults.scoring_b(**{field: value}), up, ps)
