"""The generator of tests/signal_cases.py held to its effects, with the oracle alone (no device): every class of case the
device test relies on is reached, the two numeric conditions on the random models hold, and recipes one step apart give
different arrays.  `-s` prints the counts."""
import numpy as np
import pytest

from oracle import signals, signals_h
from tests import signal_cases as sc

KEYS_S = ("sig5", "sig3", "cano5", "cano3", "dinc")
KEYS_H = ("sig5", "sig3", "sigS", "sigT", "sigE", "phs5", "phs3", "dinc")


def _h_model(c):
    return signals_h.model_of(c["model"])


def test_lengths_ranges_and_budget():
    for kind, lens in (("s", sc.LEN_S), ("h", sc.LEN_H)):
        cs = sc.cases(kind)
        got = [c["codes"].size - (kind == "h") for c in cs if c["group"] == "length"]
        assert got == list(lens)
        n = 300
        ranges = {(c["left"], c["right"]) for c in cs if c["group"] == "range"}
        offs = (3, 23) if kind == "s" else (3, 11, 23)
        for lf in {0, 1, 2, 3} | {o + d for o in offs for d in (-1, 0, 1)}:
            assert (lf, n) in ranges
        for rt in (n, n - 1, n - 2, n - 3, n - 25, n - 23):
            assert (0, rt) in ranges
        assert {(0, 0), (150, 150), (n, n), (0, 1), (n - 1, n)} <= ranges
        # what the oracle evaluates per kind stays near 40 kb (0.08 / 0.11 s per kb)
        evaluated = sum(int(np.count_nonzero(sc.expected(c)["mask"][c["left"]:c["right"]])) if kind == "s" else c["right"] - c["left"]
                        for c in cs)
        print(f"kind {kind}: {len(cs)} cases, {evaluated} positions evaluated by the oracle")
        assert evaluated <= 45000


def test_every_class_is_reached():
    counts = {}
    for kind in ("s", "h"):
        for c in sc.cases(kind):
            e = sc.expected(c)
            g = counts.setdefault(f"{kind}/{c['group']}", [0, 0])
            g[0] += 1
            g[1] += int(np.count_nonzero(e["mask"][c["left"]:c["right"]])) if kind == "s" else c["right"] - c["left"]
    for k, (n_cases, n_pos) in sorted(counts.items()):
        print(f"group {k:10s} {n_cases:3d} cases {n_pos:6d} positions")
        assert max(n_cases, n_pos) >= 20
    assert set(counts) == {f"s/{g}" for g in sc.GROUPS[:5] + ("order",)} | {f"h/{g}" for g in sc.GROUPS}
    # classes counted in positions (cells of the expected arrays)
    pos = dict.fromkeys(("s/floor", "s/columns_skipped", "s/runs_off_the_end", "s/level1", "s/level2", "s/level3", "s/both_ori_level1",
                         "h/phase_gtgt", "h/phase_agag", "h/threshold_only5", "h/threshold_only3", "h/stop_here", "h/stop_ahead_zeroes",
                         "h/stop_ahead_beyond_right", "h/branch_carried", "h/branch_reset", "h/bad_in_branch_window", "h/code_above_31",
                         "h/hash_restart", "h/any3_unassigned_cell_above_threshold"), 0)
    for c in sc.cases("s"):
        e, md = sc.expected(c), signals.model_of(c["model"])
        x = signals.RED_STRICT[c["codes"]]
        inside = np.zeros(x.size + 1, dtype=bool); inside[c["left"]:c["right"]] = True
        inside &= e["mask"]
        for p in np.flatnonzero(inside):
            lo, hi = p - md["pm5"].offset, p - md["pm5"].offset + md["pm5"].cols + 2
            pos["s/columns_skipped"] += lo < 0
            pos["s/runs_off_the_end"] += hi - 2 >= x.size
            pos["s/floor"] += bool((x[max(lo, 0):min(hi, x.size)] > 3).any())
        for lv in (1, 2, 3):
            pos[f"s/level{lv}"] += int(np.count_nonzero(e["cano5"] == lv) + np.count_nonzero(e["cano3"] == lv))
        if md["both_ori"]:
            pos["s/both_ori_level1"] += int(np.count_nonzero((e["cano5"] == 1) & ((e["dinc"] >> 4) == 1)))
    for c in sc.cases("h"):
        e, md = sc.expected(c), _h_model(c)
        b_len = c["codes"].size - 1
        seq = c["codes"][:b_len]
        x = signals_h.TNRED[seq]
        _, _, c5, c3 = signals_h.classes(seq, c["left"], c["right"], md["any"])
        pos["h/phase_gtgt"] += int(np.count_nonzero(e["phs5"] == 2))
        pos["h/phase_agag"] += int(np.count_nonzero(e["phs3"] == 2))
        if md["any"] == 2:
            pos["h/threshold_only5"] += int(np.count_nonzero((e["phs5"] == 0) & (c5 == 0)))
            pos["h/threshold_only3"] += int(np.count_nonzero((e["phs3"] == 0) & (c3 == 0)))
        if md["any"] == 3 and c["right"] > c["left"]:               # where `any >= 2` in place of `any == 2` would show
            th5, th3 = int(np.float32(md["fS"] * md["tonic5"])), int(np.float32(md["fS"] * md["tonic3"]))
            pos["h/any3_unassigned_cell_above_threshold"] += int(e["phs5"][c["right"] - 1] == -2 and e["sig5"][c["right"] - 1] > th5)
            pos["h/any3_unassigned_cell_above_threshold"] += int(e["phs3"][c["left"]] == -2 and e["sig3"][c["left"]] > th3)
        pos["h/code_above_31"] += int(np.count_nonzero(seq > 31))
        stop = np.isin(seq, md["trm"])
        for p in range(c["left"], c["right"]):
            if md["pot"].size:
                pos["h/stop_here"] += bool(stop[p])
                if not stop[p] and p + 3 < b_len and stop[p + 3]:
                    pos["h/stop_ahead_zeroes" if p + 3 < c["right"] else "h/stop_ahead_beyond_right"] += 1
                pos["h/hash_restart"] += bool(p >= 1 and x[p - 1] > 3 and (x[p:p + 6] < 4).all() and p + 5 < min(c["right"] + 1, b_len))
        if md["pmB"].present:
            plain = signals_h.splice_signals_h(dict(md, pmB=signals_h.PatMat([0] * 5, [])), c["codes"], b_len, c["left"], c["right"])["sig3"]
            pos["h/branch_carried"] += int(np.count_nonzero(plain != e["sig3"]))
            other = signals_h.splice_signals_h(dict(md, maxb3d=md["maxb3d"] + 1), c["codes"], b_len, c["left"], c["right"])["sig3"]
            pos["h/branch_reset"] += int(np.count_nonzero(other != e["sig3"]))
            pm = md["pmB"]
            for p in np.flatnonzero(x > 3):
                pos["h/bad_in_branch_window"] += int(np.count_nonzero((np.arange(p + pm.offset - pm.cols - pm.order + 1, p + pm.offset + 1) >= c["left"])
                                                                      & (np.arange(p + pm.offset - pm.cols - pm.order + 1, p + pm.offset + 1) < c["right"])))
    for k, v in sorted(pos.items()):
        print(f"class {k:28s} {int(v):6d} positions")
        assert v >= 20, k


def test_order_of_additions_matters_and_nothing_leaves_int16():
    """(1) summing the matrix columns last to first instead of first to last changes sig5 at 50 or more of the checked positions:
    a kernel that reassociates or fuses the sum is caught; (2) |fs * P| + |tab| < 32 000 at every position of every case (beyond
    the range of a short, the reference's cast of the scaled score is undefined)"""
    differ = checked = 0
    for c in sc.cases("s"):
        same = sc.sig5_with_order(c, reverse=False)
        assert np.array_equal(same, sc.expected(c)["sig5"]), c["name"]           # the term list is the oracle's sum
        other = sc.sig5_with_order(c, reverse=True)
        differ += int(np.count_nonzero(other != same))
        checked += int(np.count_nonzero(sc.expected(c)["mask"][c["left"]:c["right"]]))
    print(f"order of additions: sig5 differs at {differ} of {checked} positions")
    assert differ >= 50
    # the scaled score of a cell is its signal minus the class term (the oracle adds them as Python integers and refuses a sum
    # that does not fit); the start / stop contexts and the coding potential have no class term
    worst = 0
    for kind in ("s", "h"):
        for c in sc.cases(kind):
            e = sc.expected(c)
            md = signals.model_of(c["model"]) if kind == "s" else _h_model(c)
            tab = np.asarray(md["tab"], dtype=np.int64)
            inside = np.zeros(e["sig5"].size, dtype=bool); inside[c["left"]:c["right"]] = True
            if kind == "s":
                inside &= e["mask"]
            d5, d3 = (e["dinc"] >> 4).astype(np.int64), (e["dinc"] & 15).astype(np.int64)
            parts = [e["sig5"].astype(np.int64) - tab[d5]]
            if kind == "s" or not md["pmB"].present:               # (with a branch term sig3 carries that as well: its own range below)
                parts.append(e["sig3"].astype(np.int64) - tab[16 + d3])
            for v in parts:
                worst = max(worst, int(np.abs(v[inside]).max(initial=0)) + int(np.abs(tab).max()))
            if kind == "h":
                worst = max(worst, *(int(np.abs(e[k].astype(np.int64)).max(initial=0)) for k in ("sig3", "sigS", "sigT", "sigE")))
    print(f"largest |scaled score| + |class term|: {worst}")
    assert worst < 32000


@pytest.mark.parametrize("a,b", sc.NEIGHBOURS, ids=[f"{a}~{b}" for a, b in sc.NEIGHBOURS])
def test_neighbouring_recipes_differ(a, b):
    ca, cb = sc.case(a), sc.case(b)
    ea, eb = sc.expected(ca), sc.expected(cb)
    keys = KEYS_S if ca["kind"] == "s" else KEYS_H
    n = min(ea["sig5"].size, eb["sig5"].size)
    m = ea["mask"][:n] & eb["mask"][:n] if ca["kind"] == "s" else np.ones(n, dtype=bool)
    assert any(not np.array_equal(ea[k][:n][m], eb[k][:n][m]) for k in keys)


def test_models_are_accepted_by_both_readers():
    """a case's model dict is fixture-shaped: the oracle's reader and the ctypes reader take it"""
    from spaln_amd import abi
    for kind, reader, oracle_reader in (("s", abi.signal_model_from_fixture, signals.model_of),
                                        ("h", abi.signal_model_h_from_fixture, signals_h.model_of)):
        seen = set()
        for c in sc.cases(kind):
            if c["model_name"] in seen:
                continue
            seen.add(c["model_name"])
            m, md = reader(c["model"]), oracle_reader(c["model"])
            assert int(m.any) == int(md["any"])
            if kind == "s":
                assert (m.cols5, m.off5, m.cols3, m.off3) == (md["pm5"].cols, md["pm5"].offset, md["pm3"].cols, md["pm3"].offset)
                assert np.float32(m.fs) == md["fs"]
            else:
                assert (m.pm5.cols, m.pm5.offset, m.pm5.order) == (md["pm5"].cols, md["pm5"].offset, md["pm5"].order)
                assert bool(m.pmB.rows) == md["pmB"].present and int(m.pot_ndata) == md["pot_ndata"] and int(m.maxb3d) == md["maxb3d"]
        print(f"kind {kind}: {len(seen)} models")
