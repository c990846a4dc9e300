"""tests/thin_cases.py held to its effects, without a GPU: the recipes are what they are named for only if the restatement's
result and the window say so.  Uses ubr.align, ubr.stripe and arithmetic on the problems; nothing of the product runs.

The classes counted below are conditions on the inputs: each must hold for at least 20 generated cases, so that the device
test meets the branch it names more than by accident.

What the committed generator measures per class: the docstring of test_every_class_is_well_populated."""
import collections

import pytest

from tests import thin_cases as tc
from tests import unspliced_ref as ubr

CLASS_FLOOR = 20
CLASSES = ("long_gap_noll3", "local_proper_subrange", "local_empty", "corner_on_band_edge", "end_mode_bit0", "end_mode_bit1",
           "terminal_gap", "top_hi_below_cols", "steps_mod4_0", "steps_mod4_1", "steps_mod4_2", "steps_mod4_3")


def classes_of(sc, up, p):
    """the classes one case falls into, from the restatement's result and the window"""
    g = tc.geometry(p, sc.sh)
    out = set()
    if g["host"]:
        return out
    score, skl = ubr.align(sc, up, p)
    corners = skl[1:].tolist()
    thin = 1 <= g["rows"] <= 16
    local_l, local_r = sc.local and p.a_exgl and p.b_exgl, sc.local and p.a_exgr and p.b_exgr
    if not corners:
        if local_l and local_r and thin:
            out.add("local_empty")
    else:
        segs = [(m1 - m0, n1 - n0) for (m0, n0), (m1, n1) in zip(corners, corners[1:])]
        gaps = [max(dm, dn) for dm, dn in segs if dm == 0 or dn == 0]
        if thin and sc.noll == 3 and any(d > sc.codonk1 for d in gaps):
            out.add("long_gap_noll3")
        first_off = corners[0] != [p.a_left, p.b_left]
        last_off = corners[-1] != [p.a_right, p.b_right]
        if thin and local_l and local_r and first_off and last_off:
            out.add("local_proper_subrange")
        if thin and any(n - m in (g["lw"], g["up"]) for m, n in corners[1:-1]):
            out.add("corner_on_band_edge")                       # (an inner corner: the path itself runs into the band's edge)
        # a terminal gap taken: the path leaves the range's own corner along an edge, or (free or local end) does not start / end there
        starts_with_gap = bool(segs) and (segs[0][0] == 0 or segs[0][1] == 0)
        ends_with_gap = bool(segs) and (segs[-1][0] == 0 or segs[-1][1] == 0)
        if thin and not (local_l and local_r) and (first_off or last_off or starts_with_gap or ends_with_gap):
            out.add("terminal_gap")
    fb = 0.0 if p.b_exgr else up.tgapf
    fa = 0.0 if p.a_exgr else up.tgapf
    if thin and not local_r:                                      # (LocalR: lastB_ng's passes do not run)
        if p.b_right == p.b_len and fb < 1:
            out.add("end_mode_bit0")
        if p.a_right == p.a_len and fa < 1:
            out.add("end_mode_bit1")
    if thin and g["top_hi"] < g["cols"]:
        out.add("top_hi_below_cols")
    if thin:
        out.add("steps_mod4_%d" % (g["steps"] % 4))
    return out


@pytest.fixture(scope="module")
def census():
    count = collections.Counter()
    per_recipe = {}
    for name in tc.names():
        sc, up, ps, tags = tc.build(name)
        assert len(tags) == len(ps) > 0, name
        c = collections.Counter()
        for p in ps.items:
            c.update(classes_of(sc, up, p))
        per_recipe[name] = c
        count.update(c)
    return count, per_recipe


def test_every_class_is_well_populated(census):
    """Counts of the committed generator (6 493 cases): long_gap_noll3 2333, local_proper_subrange 106, local_empty 47,
    corner_on_band_edge 435, end_mode_bit0 1650, end_mode_bit1 1533, terminal_gap 4402, top_hi_below_cols 915,
    steps mod 4 = 0 / 1 / 2 / 3: 1384 / 1757 / 1785 / 1748"""
    count, _ = census
    print({k: count[k] for k in CLASSES})
    for k in CLASSES:
        assert count[k] >= CLASS_FLOOR, (k, count[k])


def test_the_window_arithmetic_is_the_restatements():
    for name in tc.names():
        sc, up, ps, _ = tc.build(name)
        for i, p in enumerate(ps.items):
            w = ubr.stripe(p, sc.sh)
            assert (w.lw, w.up) == tc.window(p, sc.sh), (name, i)
            g = tc.geometry(p, sc.sh)
            if not g["host"]:
                assert ubr.cells(p, sc.sh) > 0 and g["steps"] > 0, (name, i)


def test_only_the_named_recipes_have_requests_without_a_cell():
    seen = collections.Counter()
    for name in tc.names():
        sc, up, ps, tags = tc.build(name)
        for p, t in zip(ps.items, tags):
            g = tc.geometry(p, sc.sh)
            if "without_cells" not in name:
                assert not g["host"], (name, t)
            elif g["host"]:
                seen[t["branch"]] += 1
            else:
                assert t["branch"] == "sweep", (name, t)
    assert all(seen[b] >= 16 for b in ("no_rows", "no_cols", "neither", "diagonal")), seen


def test_every_request_lies_inside_unrelated_flanks():
    for name in tc.names():
        sc, up, ps, tags = tc.build(name)
        for p, t in zip(ps.items, tags):
            left_a, right_a, left_b, right_b = p.a_left, p.a_len - p.a_right, p.b_left, p.b_len - p.b_right
            for flank, at_end in zip((left_a, right_a, left_b, right_b), t["at_end"]):
                assert flank == 0 if at_end else 5 <= flank <= 40, (name, t)
            assert (t["rows"], t["cols"]) == (p.a_right - p.a_left, p.b_right - p.b_left)


def test_the_recipes_cover_what_they_are_named_for(census):
    _, per_recipe = census
    # grid: every named shape, both ways round, on both alphabets; rows 17 is the first tiled request
    for alpha in ("aa", "nt"):
        sc, up, ps, tags = tc.build(f"grid/{alpha}")
        shapes = {(t["rows"], t["cols"]) for t in tags}
        assert {(r, c) for r in tc.GRID_ROWS for c in tc.GRID_COLS} <= shapes
        assert {(c, r) for r in tc.GRID_ROWS for c in tc.GRID_COLS if c <= 16} <= shapes
        steps16 = {tc.geometry(p, sc.sh)["steps"] for p, t in zip(ps.items, tags) if t["rows"] == 16}
        assert min(steps16) <= 16 and max(steps16) > 64 and {s % 4 for s in steps16} == {0, 1, 2, 3}
        assert any(lo < s <= lo + 16 for s in steps16 for lo in (16,)) and any(32 < s <= 48 for s in steps16) and any(48 < s <= 64 for s in steps16)
    # ends: every flag tuple at every combination of sequence ends, per terminal gap factor
    for alpha in ("aa", "nt"):
        for t in (1.0, 0.5, 0.0):
            sc, up, ps, tags = tc.build(f"ends/{alpha}/tgapf{t}")
            assert up.tgapf == t and {(g["exg"], g["at_end"]) for g in tags} == {(e, a) for e in tc.EXGS for a in tc.EXGS}
            for p, g in zip(ps.items, tags):
                assert ((p.a_left == 0), (p.a_right == p.a_len), (p.b_left == 0), (p.b_right == p.b_len)) == tuple(bool(x) for x in g["at_end"])
        for noll in (2, 3):
            sc, up, ps, tags = tc.build(f"ends/{alpha}/steep_top/noll{noll}")
            assert up.tgapf == 2.0 and sc.noll == noll and all(p.a_left == 0 and not p.a_exgl and not p.b_exgl and 1 <= t["rows"] <= 16 for p, t in zip(ps.items, tags))
    # band: the band, not the range, bounds the rows
    for alpha in ("aa", "nt"):
        for sh in tc.BAND_SH:
            sc, up, ps, tags = tc.build(f"band/{alpha}/sh{sh}")
            assert sc.sh == sh and set(tc.BAND_SHAPES) <= {(t["rows"], t["cols"]) for t in tags}
            if sh != 100:
                clipped = sum(1 for p in ps.items if (lambda g: g["lw"] > p.b_left - p.a_right and g["up"] < p.b_right - p.a_left)(tc.geometry(p, sh)))
                assert clipped >= 40, (alpha, sh, clipped)
    # long gaps: both gap models, both k1, the indel at the very start of the range too
    for alpha in ("aa", "nt"):
        for noll in (2, 3):
            for k1 in (3, 7):
                sc, up, ps, tags = tc.build(f"long/{alpha}/noll{noll}/k{k1}")
                assert (sc.noll, sc.codonk1) == (noll, k1)
                assert {abs(t["indel"]) for t in tags} == set(range(1, 13)) and {t["where"] for t in tags} == {"start", "mid", "end"}
                assert all(t["rows"] <= 16 for t in tags)
                if noll == 3:
                    assert per_recipe[f"long/{alpha}/noll{noll}/k{k1}"]["long_gap_noll3"] >= CLASS_FLOOR
    # local: proper sub-ranges, empty results, equal maxima, one-sided requests
    for alpha in ("aa", "nt"):
        name = f"local/{alpha}"
        sc, up, ps, tags = tc.build(name)
        assert sc.local == 1
        assert per_recipe[name]["local_proper_subrange"] >= CLASS_FLOOR and per_recipe[name]["local_empty"] >= 15
        parts = collections.Counter(t["part"] for t in tags)
        assert parts["same_row"] >= 10 and parts["two_rows"] >= 20 and parts["one_side"] >= 40
        for p, t in zip(ps.items, tags):
            if t["part"] == "empty":
                assert ubr.align(sc, up, p)[1].shape[0] == 0
    # waves: exactly that many thin requests in one call
    for alpha in ("aa", "nt"):
        for n in tc.WAVE_SIZES:
            for v in range(3):
                sc, up, ps, tags = tc.build(f"waves/{alpha}/n{n}/v{v}")
                assert tc.predict(sc, up, ps) == dict(thin_requests=n, wide_requests=0, host_requests=0, requests_not_computed=0, requests_le16_rows=n)
                if n in (4, 5):
                    assert sorted((t["rows"], t["cols"]) for t in tags) == sorted(tc.UNLIKE[:n])
                    steps = [tc.geometry(p, sc.sh)["steps"] for p in ps.items]
                    assert min(steps) == 1 and max(steps) >= 70
                    assert steps.index(max(steps)) == v + 1               # as given, the longest sits in slot 1, 2, 3 of the first wave
                    assert len({t["exg"] for t in tags}) == n and (1, 1, 1, 1) in {t["exg"] for t in tags} and (0, 0, 0, 0) in {t["exg"] for t in tags}
    # rounds: thin and tiled interleaved; the tight form needs several launch sets and leaves nothing out
    for alpha in ("aa", "nt"):
        sc, up, ps, tags = tc.build(f"rounds/{alpha}/mixed")
        sct, upt, pst, _ = tc.build(f"rounds/{alpha}/mixed_tight")
        want = tc.predict(sc, up, ps)
        assert want["thin_requests"] >= 40 and want["wide_requests"] >= 25
        kinds = [t["rows"] <= 16 for t in tags]
        assert sum(1 for x, y in zip(kinds, kinds[1:]) if x != y) >= 40           # interleaved
        assert [(p.a_left, p.a_right, p.b_left, p.b_right) for p in ps.items] == [(p.a_left, p.a_right, p.b_left, p.b_right) for p in pst.items]
        needs = [tc.tiled_need(p, sc.sh) for p in ps.items]
        assert upt.max_trace_bytes == max(needs) and up.max_trace_bytes == 0
        for thin_on in (True, False):
            assert tc.predict(sct, upt, pst, thin_on)["requests_not_computed"] == 0
            used = sum(tc.thin_need(p, sc.sh) if thin_on and t["rows"] <= 16 else tc.tiled_need(p, sc.sh) for p, t in zip(ps.items, tags))
            assert used > 2 * upt.max_trace_bytes
    sc, up, ps, tags = tc.build("rounds/big")
    assert all(t["rows"] == 200 and t["cols"] == 200 for t in tags) and tc.predict(sc, up, ps)["wide_requests"] == len(ps) >= 3
    sc, up, ps, tags = tc.build("rounds/after_big")
    assert tc.predict(sc, up, ps)["thin_requests"] == len(ps)
