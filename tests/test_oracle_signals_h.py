"""SURVEY 8 f1, protein side: the CPU restatement of Exinon::intron53_p (oracle/signals_h.py: position weight matrices of
order 1 and 2 on the tron sequence, the 5th-order coding potential, stop-codon rules, dinucleotide classes, phases)
against the SGPT6 arrays the reference produced for every protein fixture -- h1_* with the generic tables, c1_* with the
Dictyostelium set: all seven arrays, every position."""
import numpy as np
import pytest

from oracle import signals_h
from tests import spdg
from tests.conftest import golden_files

def stale_mask(b_len, left, right):
    """the cells the reference's class loop never assigns (acceptor class of `left`, donor class of `right - 1`: whatever
    the allocation held, as on the cDNA path) and the phases derived from them"""
    ok = {k: np.ones(b_len + 3, dtype=bool) for k in ("sig5", "sig3", "phs5", "phs3")}
    ok["sig3"][left] = False
    ok["phs3"][max(left - 1, 0):left + 2] = False
    ok["sig5"][right - 1] = False
    ok["phs5"][max(right - 2, 0):right + 1] = False
    return ok


# sgh_: dumps for the signal precompute alone (any = 1 / 2 / 3, runs of N, range ends at the sequence ends, stop codons either side
# of the range end, the branch-point reach); no engine test reads them
FILES = [f for pre in ("h1_", "c1_", "hb_", "sgh_") for f in golden_files(pre) if "pm5_hdr" in spdg.load(f)]   # hb_: branch-point term on (own intron-penalty table: not batched with h1_)


@pytest.mark.parametrize("path", FILES, ids=[f.split("/")[-1][:-5] for f in FILES])
def test_signals_h_equal_reference(path):
    fx = spdg.load(path)
    md = signals_h.model_of(fx)
    q = fx["prm"]
    b_len = len(fx["b_codes"]) - 1
    got = signals_h.splice_signals_h(md, fx["b_codes"], b_len, q["b_left"], q["b_right"])
    ok = stale_mask(b_len, q["b_left"], q["b_right"])
    for k in ("sig5", "sig3", "sigS", "sigT", "sigE", "phs5", "phs3"):
        m = ok[k] if k in ok else np.ones(b_len + 3, dtype=bool)
        assert np.array_equal(got[k][m], fx[k][:b_len + 3][m]), k


def test_fixture_count():
    assert len(FILES) >= 34 + 13


def test_branch_point_term_is_exercised():
    """hb_branch*: `ref_dump -b` (-yB) switches the branch-point matrix on; the acceptor signal then differs from the plain one
    at hundreds of positions, and the reach limit (-yD) matters"""
    fa, fb = (spdg.load([f for f in golden_files("hb_branch") if f.endswith(n + ".spdg")][0]) for n in ("hb_branch", "hb_branch_d20"))
    md = signals_h.model_of(fa)
    assert md["pmB"].present and md["fB"] > 0
    q = fa["prm"]
    b_len = len(fa["b_codes"]) - 1
    with_b = signals_h.splice_signals_h(md, fa["b_codes"], b_len, max(0, q["b_left"]), q["b_right"])["sig3"]
    md0 = dict(md)
    md0["pmB"] = signals_h.PatMat([0, 0, 0, 0, 0], fa["pmB_f32"][:2])
    without = signals_h.splice_signals_h(md0, fa["b_codes"], b_len, max(0, q["b_left"]), q["b_right"])["sig3"]
    assert int(np.count_nonzero(with_b != without)) > 200
    assert int(np.count_nonzero(np.asarray(fa["sig3"]) != np.asarray(fb["sig3"]))) > 100


def _fx(name):
    return spdg.load([f for f in FILES if f.endswith("/" + name + ".spdg")][0])


def test_any2_threshold_rule_fires_without_a_class():
    """sgh_any2: the planted acceptor contexts make phase-0 cells where the dinucleotide has no level (20 or more); no donor
    context can under the reference's tables (best level-less donor: AC, -434 of th5 = -400 with the protein scale), see
    tests/test_oracle_signals.py::test_threshold_rule_fires_without_a_class"""
    from oracle import signals
    fx = _fx("sgh_any2")
    md = signals_h.model_of(fx)
    b_len = len(fx["b_codes"]) - 1
    _, _, c5, c3 = signals_h.classes(fx["b_codes"][:b_len], 0, b_len, 2)
    n3 = int(np.count_nonzero((fx["phs3"][:b_len + 3] == 0) & (c3 == 0)))
    n5 = int(np.count_nonzero((fx["phs5"][:b_len + 3] == 0) & (c5 == 0)))
    th5 = int(np.float32(md["fS"] * md["tonic5"]))
    pm = md["pm5"]
    best = max(int(np.float32(md["fs"]) * np.float32(signals.best_context(pm, {pm.offset: x, pm.offset + 1: y})[0] + float(pm.tonic)))
               + int(md["tab"][4 * x + y]) for x in range(4) for y in range(4) if signals.cano_tables(2, 0)[0][4 * x + y] == 0)
    print(f"sgh_any2: threshold-only cells phs3 {n3}, phs5 {n5}; best level-less donor {best} vs th5 {th5}")
    assert md["any"] == 2 and n3 >= 20
    assert best + 4 < th5 and n5 == 0
    assert [signals_h.model_of(_fx(f"sgh_any{a}"))["any"] for a in (1, 3)] == [1, 3]
    assert np.count_nonzero(_fx("sgh_any1")["phs5"] != fx["phs5"]) > 100 and np.count_nonzero(_fx("sgh_any3")["phs3"] != fx["phs3"]) > 100


def test_nruns_window_has_its_runs():
    fx = _fx("sgh_nruns")
    b_len = len(fx["b_codes"]) - 1
    bad = signals_h.TNRED[fx["b_codes"][:b_len]] > 3
    assert bad[0] and bad[b_len - 1]
    edges = np.flatnonzero(np.diff(np.concatenate([[1], bad.astype(np.int8), [1]])))
    runs = (edges[1::2] - edges[0::2]).tolist()                # lengths of the good stretches
    assert all(runs.count(k) >= 2 for k in range(1, 10)), runs
    for cols in (3, 20, 24):                                     # an N within each matrix width of either end
        assert bad[1:cols].any() and bad[b_len - cols:b_len - 1].any()
    assert int(np.count_nonzero(fx["phs5"] == 2)) >= 2 and int(np.count_nonzero(fx["phs3"] == 2)) >= 1      # GTGT(GT), AGAG


def test_range_edges_place_stops_either_side_of_the_range_end():
    """sgh_range_edges_a .. e: a termination code at every offset right - 4 .. right + 3 (two stop codons lie at least three
    bases apart: five windows); f .. h: six good bases between two Ns ending at right, right + 1, right + 2; b_left in {1, 2, 12}
    and b_right in {len - 1, len - 2, len - 25} among them"""
    seen, lefts, ends, six = set(), set(), set(), set()
    for tag in "abcdefgh":
        fx = _fx("sgh_range_edges_" + tag)
        q, b = fx["prm"], fx["b_codes"]
        b_len = len(b) - 1
        trm = set(int(v) for v in fx["sigmodel_i32"][5:7])
        lefts.add(q["b_left"]); ends.add(b_len - q["b_right"])
        seen |= {k for k in range(-4, 4) if q["b_right"] + k < b_len and int(b[q["b_right"] + k]) in trm}
        bad = signals_h.TNRED[b[:b_len]] > 3
        for k in (0, 1, 2):
            e = q["b_right"] + k
            if bad[e - 6] and bad[e + 1] and not bad[e - 5:e + 1].any():
                six.add(k)
    assert seen == set(range(-4, 4)) and six == {0, 1, 2}
    assert {1, 2, 12} <= lefts and {1, 2, 25} <= ends


def test_branch_reach_is_decided_by_one_position():
    """sgh_branch_n (-yB 2.0 -yD 20): the oracle with the reach one shorter or one longer no longer gives the reference's sig3"""
    fx = _fx("sgh_branch_n")
    md = signals_h.model_of(fx)
    q = fx["prm"]
    b_len = len(fx["b_codes"]) - 1
    assert md["pmB"].present and md["maxb3d"] == 20
    assert int(np.count_nonzero(signals_h.TNRED[fx["b_codes"][:b_len]] > 3)) >= 3
    ok = stale_mask(b_len, q["b_left"], q["b_right"])["sig3"]
    for reach, same in ((19, False), (20, True), (21, False)):
        got = signals_h.splice_signals_h(dict(md, maxb3d=reach), fx["b_codes"], b_len, q["b_left"], q["b_right"])["sig3"]
        assert np.array_equal(got[ok], fx["sig3"][:b_len + 3][ok]) == same, reach
