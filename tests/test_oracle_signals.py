"""the CPU restatement of the splice-signal precompute (oracle/signals.py: Exinon::intron53_c /
intron53_n over PatMat::calcPatMat) against the arrays the reference itself produced for every S fixture.

Two cells per window are excluded: sig5 / cano5 of position right - 1 (and cano5 of `right`) and sig3 / cano3 of
position left -- the reference's loops never assign the class cells behind them, so what it dumps there is whatever
the allocation held (it differs between runs of the same input; the DP never reads a donor there / an acceptor
there)."""
import numpy as np
import pytest

from oracle import signals
from tests import spdg
from tests.conftest import golden_files, golden_ids

# sg_: dumps for the signal precompute alone (algmode.any = 1 / 2 / 3 with the sites' levels, range ends within a matrix width
# of the sequence ends, Ns there); no engine test reads them
FILES = [p for pre in ("s1_", "c2_", "o3_", "sg_") for p in golden_files(pre)]
IDS = [i for pre in ("s1_", "c2_", "o3_", "sg_") for i in golden_ids(pre)]


def _stale(n, left, right):
    ok5 = np.ones(n + 1, dtype=bool); ok3 = np.ones(n + 1, dtype=bool)
    ok5[right - 1:right + 1] = False
    ok3[left] = False
    return ok5, ok3


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_signals_equal_reference(path):
    fx = spdg.load(path)
    md = signals.model_of(fx)
    b = fx["b_codes"]
    n = b.size
    left, right = fx["prm"]["b_left"], fx["prm"]["b_right"]
    ok5, ok3 = _stale(n, left, right)
    d5, d3, c5, c3 = signals.classes(b, left, right, md["any"], md["both_ori"])
    assert np.array_equal(d5, fx["dinc5"]) and np.array_equal(d3, fx["dinc3"])
    assert np.array_equal((c5 > 0)[ok5], (fx["cano5"] > 0)[ok5])
    assert np.array_equal((c3 > 0)[ok3], (fx["cano3"] > 0)[ok3])
    # the pure-Python scan costs ~50 us per position: whole window when short, both ends + a slice otherwise
    spans = [(left, right)] if right - left <= 3000 else [(left, left + 700), ((left + right) // 2, (left + right) // 2 + 700),
                                                            (right - 700, right)]
    for lo, hi in spans:
        s5, s3 = signals.splice_signals(md, b, left, right, lo, hi)
        sel = np.zeros(n + 1, dtype=bool); sel[lo:hi] = True
        assert np.array_equal(s5[sel & ok5], fx["sig5"][sel & ok5]), (path, lo, hi)
        assert np.array_equal(s3[sel & ok3], fx["sig3"][sel & ok3]), (path, lo, hi)
    outside = np.ones(n + 1, dtype=bool); outside[left:right] = False
    assert not fx["sig5"][outside].any() and not fx["sig3"][outside].any()
    if "cano5_lvl" in fx:                           # (ref_dump -a) the sites' LEVELS, as Exinon::isCanon reads them
        assert np.array_equal(c5[ok5], fx["cano5_lvl"][ok5]) and np.array_equal(c3[ok3], fx["cano3_lvl"][ok3])
    if "sigphase" in fx or md["any"] != 2:          # the phases of intron53_n's loop, outside the cells the stale classes reach
        s5, s3 = (fx["sig5"], fx["sig3"]) if right - left > 3000 else (s5, s3)
        p5, p3 = signals.phases(md, b, left, right, s5, s3)
        okp5, okp3 = np.zeros(n + 1, dtype=bool), np.zeros(n + 1, dtype=bool)
        okp5[left:right + 1] = okp3[left:right + 1] = True              # (the cells the dump reads; -2 elsewhere by construction)
        okp5[max(right - 2, 0):right + 1] = False
        okp3[max(left - 1, 0):left + 2] = False
        assert np.array_equal(p5[okp5], fx["phs5"][okp5]) and np.array_equal(p3[okp3], fx["phs3"][okp3])


def _fixture(name):
    return spdg.load([f for f in FILES if f.endswith("/" + name + ".spdg")][0])


def test_any_changes_levels_and_phases():
    """the four `any` dumps share one window: every level table is in use, and any = 2 alone has the threshold rule"""
    fxs = {a: _fixture(f"sg_any{a}") for a in (1, 2, 3)}
    assert all(np.array_equal(fxs[1]["b_codes"], fxs[a]["b_codes"]) for a in (2, 3))
    assert [int(fxs[a]["sigmodel"][1]) for a in (1, 2, 3)] == [1, 2, 3] and int(_fixture("sg_any2_ori3")["sigmodel"][3]) == 1
    lv = {a: (set(np.unique(fxs[a]["cano5_lvl"]).tolist()), set(np.unique(fxs[a]["cano3_lvl"]).tolist())) for a in fxs}
    assert lv[1] == ({0, 2, 3}, {0, 2, 3}) and lv[3] == ({0, 1, 2, 3}, {0, 1, 2, 3})
    assert np.count_nonzero(fxs[3]["cano5_lvl"] == 0) <= 3              # any = 3: every other cell the loop assigns is a level-1 site
    for a, b in ((1, 2), (2, 3), (1, 3)):
        assert np.count_nonzero(fxs[a]["cano5_lvl"] != fxs[b]["cano5_lvl"]) > 100
        assert np.count_nonzero(fxs[a]["phs3"] != fxs[b]["phs3"]) > 100
    o3 = _fixture("sg_any2_ori3")
    assert np.count_nonzero(o3["cano5_lvl"] != fxs[2]["cano5_lvl"]) >= 20 and np.count_nonzero(o3["cano3_lvl"] != fxs[2]["cano3_lvl"]) >= 20


def test_threshold_rule_fires_without_a_class():
    """any = 2: `sig > th` makes a phase-0 cell where the dinucleotide has no level at all.  The planted acceptor contexts do
    that at 20 or more cells.  No donor can: under the reference's tables the best context around any dinucleotide without a
    level scores below th5 (exact bound, oracle.signals.best_context: AC reaches -216 of -200 with the cDNA scale), so the
    donor side of the rule is decided by the device tests against the oracle alone (tests/signal_cases.py, random matrices)"""
    fx = _fixture("sg_any2")
    md = signals.model_of(fx)
    b = fx["b_codes"]
    _, _, c5, c3 = signals.classes(b, 0, b.size, 2, 0)
    n3 = int(np.count_nonzero((fx["phs3"] == 0) & (c3 == 0)))
    n5 = int(np.count_nonzero((fx["phs5"] == 0) & (c5 == 0)))
    th5 = int(np.float32(md["fS"] * md["tonic5"]))
    best = max(int(np.float32(md["fs"]) * np.float32(signals.best_context(md["pm5"], {md["pm5"].offset: x, md["pm5"].offset + 1: y})[0]
                                                     + float(md["pm5"].tonic))) + int(md["tab"][4 * x + y])
               for x in range(4) for y in range(4) if signals.cano_tables(2, 0)[0][4 * x + y] == 0)
    print(f"sg_any2: threshold-only cells phs3 {n3}, phs5 {n5}; best level-less donor {best} vs th5 {th5}")
    assert n3 >= 20
    assert best + 2 < th5 and n5 == 0              # (+ 2: float64 bound of a float32 sum of 26 terms, then truncation)


def test_model_is_the_same_in_every_fixture():
    """one species table behind all fixtures: the model is data of the parameter set, not of the window"""
    ref = None
    for path in FILES:
        fx = spdg.load(path)
        key = (fx["pm5_hdr"].tolist(), fx["pm3_hdr"].tolist(), fx["pm5_f32"].tobytes(), fx["pm3_f32"].tobytes(),
               fx["sig53tab01"].tolist(), int(fx["sigmodel"][0]))
        ref = ref or key
        assert key == ref, path


def test_scan_edge_rules():
    fx = spdg.load(golden_files("s1_basic")[0])
    md = signals.model_of(fx)
    pm = md["pm5"]
    x = signals.RED_STRICT[fx["b_codes"][:200]].copy()
    floor = np.float32(np.float32(pm.cols) * pm.min_elem) + pm.tonic
    assert signals.scan(pm, x, x.size - 1) == floor              # the window runs off the end: "bad"
    x[100] = 4                                                   # an N anywhere under the window: "bad"
    assert signals.scan(pm, x, 100) == floor and signals.scan(pm, x, 100 - pm.cols) != floor
    assert signals.scan(pm, x, 0) != floor                       # a window starting before base 0 just skips columns
