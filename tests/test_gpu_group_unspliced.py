"""The unspliced aligner on a device group (spdp_group_homscore_b / _align_b / _align_b_seeded): what one context returns for the same
problems, in the caller's order, whatever the number of members; the trace budget per member; the balance of the shards.  The groups
are several contexts on ONE card: this shows that the records are the same, not that anything scales."""
import ctypes as C

import numpy as np
import pytest

from spaln_amd import abi, defaults, engine
from tests import unspliced_cases as uc
from tests import unspliced_seeded_cases as usc
from tests.test_gpu_unspliced import random_pairs

pytestmark = pytest.mark.gpu

SETS = ("shapes1", "shapes2", "local", "tgapf")
SEEDED = ("gaps_q3", "mid_q2", "local_q1")


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


@pytest.fixture(scope="module")
def model():
    return defaults.wilip_model_b()


@pytest.fixture(scope="module")
def one_context(eng):
    """Engine.align_b / homscore_b of every option set of the four fixture files: computed once, compared with every group size"""
    out = {}
    for name in SETS:
        for k in range(len(uc.load(name)["runs"])):
            sc, up, ps, recs = uc.problems(name, k)
            out[(name, k)] = (eng.align_b(sc, up, ps), eng.homscore_b(sc, up, ps))
    return out


def same(x, y):
    return len(x) == len(y) and all(a[0] == b[0] and a[1].tolist() == b[1].tolist() for a, b in zip(x, y))


@pytest.mark.parametrize("members", [1, 2, 3, 5])
def test_group_equals_one_context(eng, grp, one_context, members):
    g = grp if members == 3 else engine.Group([0] * members)
    try:
        for (name, k), (want, want_hom) in one_context.items():
            sc, up, ps, recs = uc.problems(name, k)
            got = g.align_b(sc, up, ps)
            assert same(got, want), (name, k, members)
            assert len(set(g.shards(len(ps)).tolist())) == min(members, len(ps))
            assert g.homscore_b(sc, up, ps).tolist() == want_hom.tolist(), (name, k, members)
            if members == 3:                            # the program's recorded output, as tests/test_gpu_unspliced.py holds one context to it
                stats = eng.skl_rng_b(sc, up, ps, [s for _, s in got])
                for i, ((score, skl), st, rec) in enumerate(zip(got, stats, recs)):
                    uc.check_record(st, skl[st["first"]:st["first"] + st["n_trim"]], rec, (name, k, i))
    finally:
        if g is not grp:
            g.close()


def test_an_empty_call_and_a_refusal_go_through(grp):
    sc, up = defaults.scoring_b(), abi.UnsplicedParams(1.0, 0)
    assert grp.align_b(sc, up, abi.ProblemSet()) == [] and grp.homscore_b(sc, up, abi.ProblemSet()).tolist() == []
    bad = defaults.scoring_b()
    bad.spj = 1
    ps = abi.ProblemSet()
    for a, b in random_pairs(np.random.default_rng(3), 7):
        ps.add(a, b, None, None, exg=(0, 0, 0, 0))
    with pytest.raises(RuntimeError, match="device 0: .*spj"):
        grp.align_b(bad, up, ps)
    n = len(ps)
    arr = (abi.Alignment * n)()
    assert grp.lib.spdp_group_align_b(grp.h, C.byref(bad), C.byref(up), ps.array(), n, arr) == -1
    assert all(not arr[i].skl and arr[i].n_skl == 0 for i in range(n))


@pytest.mark.parametrize("name", SEEDED)
def test_seeded_group_equals_one_context(eng, grp, model, name):
    """the library's own search on three members = one context = the program's records; then every pair with the HSPs of a level-0
    search for every other pair and a source for everything else, asked with the CALLER's pair numbers: the source searches the
    pair it is asked for, so a member's own numbering would seed pairs with the HSPs of others"""
    lib = eng.lib
    lib.spdp_wilip.restype = C.c_int
    lib.spdp_wilip.argtypes = [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for k in range(len(usc.load(name)["runs"])):
        sc, up, sp, ps, recs, opts = usc.problems(name, k)
        want = eng.align_b_seeded(sc, up, sp, ps, model=model)
        got = grp.align_b_seeded(sc, up, sp, ps, model=model)
        assert same(got, want), (name, opts)
        assert len(set(grp.shards(len(ps)).tolist())) == 3
        assert sum(grp.context(r).seeded_stats_b()["walks"] for r in range(3)) == len(ps)       # (the counters stay per context)
        skls = [s for _, s in got]
        stats = eng.skl_rng_b(sc, up, ps, skls)
        edits = eng.skl_edits_b(sc, up, ps, skls, abi.FMT_CIGAR)
        for i, rec in enumerate(recs):
            usc.check_alignment(stats[i], skls[i], [[chr(o), int(l)] for o, l, _ in edits[i][0].tolist()], rec, (name, opts, i))
        # ---- recorded HSPs + a source
        hsps = [eng.wilip_b(model, p, sc, 0) if i % 2 == 0 else None for i, p in enumerate(ps.items)]    # every other pair asks the source
        assert sum(h is not None for h in hsps) >= 3
        asked = []

        def source(pair, level, span):
            asked.append(pair)
            flat = C.POINTER(C.c_int32)()
            n = lib.spdp_wilip(C.addressof(model), C.addressof(ps.items[pair]), C.addressof(sc), None, None, level, (C.c_int32 * 4)(*span[:4]),
                               (C.c_int32 * 2)(*span[4:6]), C.byref(flat))
            if n < 1:
                return None
            v = np.array(flat[:n], dtype=np.int32)
            libc.free(flat)
            return v
        levels = [0] * len(ps)
        # (the model goes along: with qck > 1 the levels' tuple sizes come from it; where a source answers, the library's search does not)
        want_src = eng.align_b_seeded(sc, up, sp, ps, model=model, hsps=hsps, lowest_levels=levels, source=source)
        asked_one = sorted(asked)
        del asked[:]
        got_src = grp.align_b_seeded(sc, up, sp, ps, model=model, hsps=hsps, lowest_levels=levels, source=source)
        assert same(got_src, want_src), (name, opts)
        assert sorted(asked) == asked_one, (name, opts, len(asked), len(asked_one))
        assert len(set(asked_one)) >= len(ps) // 2 and max(asked_one) > len(ps) // 2, (name, opts, len(asked_one))


def test_trace_budget_holds_per_member(eng, grp):
    """exactly the largest problem exceeds max_trace_bytes: the group returns 1, that problem is "not computed", all others as before,
    all of it what one context says under the same budget"""
    rng = np.random.default_rng(23)
    sc = defaults.scoring_b()
    ps = abi.ProblemSet()
    big = rng.integers(3, 23, size=600).astype(np.uint8)
    for j, (a, b) in enumerate(random_pairs(rng, 12)):
        if j == 5:
            ps.add(big, big[::-1].copy(), None, None, exg=(0, 0, 0, 0))
        ps.add(a, b, None, None, exg=(0, 0, 0, 0))
    need = [eng.trace_bytes_b(p, sc.sh) for p in ps.items]
    budget = sorted(need)[-2]
    assert need[5] > budget and sum(1 for x in need if x > budget) == 1
    free = eng.align_b(sc, abi.UnsplicedParams(1.0, 0), ps)
    up = abi.UnsplicedParams(1.0, int(budget))
    n = len(ps)
    arr = (abi.Alignment * n)()
    assert grp.lib.spdp_group_align_b(grp.h, C.byref(sc), C.byref(up), ps.array(), n, arr) == 1
    assert arr[5].score == abi.NEVSEL and arr[5].n_skl == 0
    grp.lib.spdp_free_alignments(arr, n)
    with pytest.raises(RuntimeError):
        grp.align_b(sc, up, ps)
    got = grp.align_b(sc, up, ps, allow_partial=True)
    want = eng.align_b(sc, up, ps, allow_partial=True)
    assert same(got, want)
    assert got[5][0] == abi.NEVSEL and got[5][1].shape[0] == 0
    assert same(got[:5] + got[6:], free[:5] + free[6:])


def test_shards_are_balanced_on_eight_members(eng):
    """240 generated pairs on eight members: the longest-processing-time rule leaves no member more than one problem's cost above
    another (the member that ends heaviest was the lightest when it got its last problem, which costs at most max(cost))"""
    rng = np.random.default_rng(29)
    sc, up = defaults.scoring_b(), abi.UnsplicedParams(1.0, 0)
    ps = abi.ProblemSet()
    for a, b in random_pairs(rng, 240):
        ps.add(a, b, None, None, exg=(0, 0, 0, 0))
    cost = np.array([eng.cells_b(p, sc.sh) for p in ps.items], dtype=np.int64)
    g = engine.Group([0] * 8)
    try:
        hom = g.homscore_b(sc, up, ps)
        member = g.shards(len(ps))
    finally:
        g.close()
    assert hom.tolist() == eng.homscore_b(sc, up, ps).tolist()
    load = np.array([cost[member == r].sum() for r in range(8)], dtype=np.int64)
    print("loads", load.tolist(), "largest cost", int(cost.max()))
    assert set(member.tolist()) == set(range(8))
    assert load.max() - load.min() <= cost.max()
