"""The seeded path of the unspliced aligner on the device (spdp_align_b_seeded: `spaln -Q1 .. -Q3` on protein pairs) against
the program's recorded output, and against itself across the ways a call can be cut: thin kernel on and off, batch sizes
around a wave's four requests, HSPs brought by the caller, rounds split by the trace budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from spaln_amd import abi, defaults, engine
from tests import unspliced_cases as uc
from tests import unspliced_seeded_cases as usc
from tools import b_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVSEL = -(2 ** 31) // 16 * 7


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model():
    return defaults.wilip_model_b()


def _same(x, y):
    return len(x) == len(y) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(x, y))


@pytest.mark.parametrize("name,k", usc.runs(), ids=lambda v: str(v))
def test_every_record_of_every_option_set(eng, model, name, k):
    """align_b_seeded + skl_rng_b + skl_edits_b: corners after trimskl, score, mch / mmc / gap / unp and the Cigar are the
    program's; a pair it printed nothing for comes back without corners"""
    sc, up, sp, ps, recs, opts = usc.problems(name, k)
    alns = eng.align_b_seeded(sc, up, sp, ps, model=model)
    skls = [s for _, s in alns]
    have = [i for i, s in enumerate(skls) if s.shape[0] >= 3]
    stats = eng.skl_rng_b(sc, up, ps, skls)
    edits = eng.skl_edits_b(sc, up, ps, skls, abi.FMT_CIGAR)
    for i, rec in enumerate(recs):
        cigar = [[chr(o), int(l)] for o, l, _ in edits[i][0].tolist()]
        usc.check_alignment(stats[i], skls[i], cigar, rec, (name, opts, i))
    assert len(have) == sum(r is not None for r in recs)
    st = eng.seeded_stats_b()
    assert st["walks"] == len(ps) and st["hsp_searches"] >= len(ps)


def _child(name, k, thin):
    env = dict(os.environ)
    if thin:
        env.pop("SPDP_B_THIN", None)
    else:
        env["SPDP_B_THIN"] = "0"
    r = subprocess.run([sys.executable, "-m", "tests.unspliced_seeded_child", name, str(k)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_thin_kernel_on_and_off_give_the_same_alignments():
    """the `gaps` set alone (a planted block between two HSPs; where it stands for two residues of the other copy lspB_ng gets
    a request of about the block's height or width: on both sides of the 16-row boundary) with the thin kernel and with
    SPDP_B_THIN=0, each in a fresh process"""
    k = next(i for i, r in enumerate(usc.load("gaps_q3")["runs"]) if r["opts"] == ["-L15", "-Q3"])
    on, off = _child("gaps_q3", k, True), _child("gaps_q3", k, False)
    assert on["alignments"] == off["alignments"]
    assert on["stats"]["thin_requests"] > 0 and on["stats"]["wide_requests"] > 0
    assert off["stats"]["thin_requests"] == 0
    assert off["stats"]["wide_requests"] == on["stats"]["thin_requests"] + on["stats"]["wide_requests"]
    assert on["stats"]["requests_le16_rows"] == off["stats"]["requests_le16_rows"] == on["stats"]["thin_requests"]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_batch_sizes_around_a_wave(eng, model, n):
    """the first n pairs as a call of their own (the `shapes` set holds 48: the list goes round): a wave of the thin kernel with one,
    three, four and four-plus-one requests; every pair's result is its record from the call on the whole set"""
    k = next(i for i, r in enumerate(usc.load("shapes_q3")["runs"]) if r["opts"] == ["-L15", "-Q3"])
    sc, up, sp, ps_all, recs, _ = usc.problems("shapes_q3", k)
    full = eng.align_b_seeded(sc, up, sp, ps_all, model=model)
    doc = usc.load("shapes_q3")
    ps = abi.ProblemSet()
    for j in range(n):
        pr = doc["pairs"][j % len(doc["pairs"])]
        ps.add(uc.encode(pr["a"]), uc.encode(pr["b"]), None, None, exg=b_pairs.exg_of(15))
    got = eng.align_b_seeded(sc, up, sp, ps, model=model)
    assert _same(got, [full[j % len(full)] for j in range(n)])


def test_hsps_brought_by_the_caller(eng, model):
    """qck = 1, no model, no source: every pair brings the HSPs of a level-0 search (spdp_wilip); same result as the call that
    searches itself"""
    k = next(i for i, r in enumerate(usc.load("mid_q1")["runs"]) if r["opts"] == ["-L15", "-Q1"])
    sc, up, sp, ps_all, recs, _ = usc.problems("mid_q1", k)
    hsps_all = [eng.wilip_b(model, p, sc, 0) for p in ps_all.items]
    pick = [i for i, h in enumerate(hsps_all) if h is not None]
    assert len(pick) >= 6                                   # (mutated copies, deletions, embedded domains: they share words)
    doc = usc.load("mid_q1")
    ps = abi.ProblemSet()
    for i in pick:
        ps.add(uc.encode(doc["pairs"][i]["a"]), uc.encode(doc["pairs"][i]["b"]), None, None, exg=b_pairs.exg_of(15))
    own = eng.align_b_seeded(sc, up, sp, ps, model=model)
    searches_own = eng.seeded_stats_b()["hsp_searches"]
    brought = eng.align_b_seeded(sc, up, sp, ps, model=None, hsps=[hsps_all[i] for i in pick], lowest_levels=[0] * len(pick))
    assert _same(own, brought)
    assert searches_own >= len(pick) and eng.seeded_stats_b()["hsp_searches"] == 0


def _unrelated(n_pairs, length, seed):
    rng = np.random.default_rng(seed)
    ps = abi.ProblemSet()
    for _ in range(n_pairs):
        a, b = b_pairs.random_protein(rng, length), b_pairs.random_protein(rng, length)
        ps.add(uc.encode(a), uc.encode(b), None, None, exg=b_pairs.exg_of(15))
    return ps


def test_trace_budget_splits_a_round_and_refuses_what_exceeds_it(eng, model):
    """six unrelated pairs of 200 residues have no HSP (a 5-tuple chain would have to score above 500): under -Q1 each walk
    asks for its whole pair at once, six tiled requests in one round.  With a budget of one pair's trace store the round runs
    as six launch sets and gives the same records; one byte less and every request is above the budget: "not computed"."""
    sc, up, sp = defaults.scoring_b(), abi.UnsplicedParams(1.0, 0), defaults.seed_params_b(1, 15)
    ps = _unrelated(6, 200, 11)
    one = max(eng.trace_bytes_b(p, sc.sh) for p in ps.items)
    assert one == min(eng.trace_bytes_b(p, sc.sh) for p in ps.items)
    full = eng.align_b_seeded(sc, up, sp, ps, model=model)
    st = eng.seeded_stats_b()
    assert (st["wide_requests"], st["thin_requests"], st["device_batches"]) == (6, 0, 1)
    assert all(skl.shape[0] >= 3 for _, skl in full)
    split = eng.align_b_seeded(sc, abi.UnsplicedParams(1.0, one), sp, ps, model=model)
    assert _same(split, full) and eng.seeded_stats_b()["device_batches"] == 6
    direct = eng.align_b(sc, up, ps)
    assert _same(direct, full)                              # (no HSP, 5' end, nothing to creep into: the walk's one request is the -Q0 problem)
    n = len(ps)
    arr = (abi.Alignment * n)()
    import ctypes as C
    tight = abi.UnsplicedParams(1.0, one - 1)
    sp.wilip = C.addressof(model)
    rc = eng.lib.spdp_align_b_seeded(eng.ctx, C.byref(sc), C.byref(tight), C.byref(sp), ps.array(), n, None, None, None, None, arr)
    sp.wilip = None
    assert rc == 1 and b"max_trace_bytes" in eng.lib.spdp_last_error(eng.ctx)
    assert all(arr[i].n_skl == 0 and arr[i].score == NEVSEL for i in range(n))
    assert eng.seeded_stats_b()["requests_not_computed"] == 6
    eng.lib.spdp_free_alignments(arr, n)
