"""The thin form of the unspliced sweep (spdp_b_sweep_thin) on the device, request by request: every recipe of
tests/thin_cases.py through spdp_lsp_b against the restatement (tests/unspliced_ref), against spdp_align_b on the same problems
(the tiled kernel) and against itself under SPDP_B_THIN_SORT=0 and SPDP_B_THIN=0; the call's counters against what arithmetic on the requests
predicts.  One test per recipe group; scores and corner lists are integers, compared exactly."""
import functools

import pytest

from spaln_amd import abi, defaults, engine
from tests import thin_cases as tc
from tests import unspliced_ref as ubr

pytestmark = pytest.mark.gpu
COUNTERS = ("thin_requests", "wide_requests", "host_requests", "requests_not_computed", "requests_le16_rows")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def wanted(name):
    """the restatement's (score, corner list) of every request of the recipe, computed once"""
    sc, up, ps, _ = tc.build(name)
    return [(s, skl.tolist()) for s, skl in (ubr.align(sc, up, p) for p in ps.items)]


def same(got, want, what, tags):
    assert len(got) == len(want)
    for i, ((score, skl), (wscore, wskl)) in enumerate(zip(got, want)):
        assert score == wscore and skl.tolist() == wskl, (what, i, tags[i], score, wscore, skl.tolist(), wskl)


def check(eng, monkeypatch, name):
    """the recipe with the thin kernel on (its requests sorted by length, and as given), through spdp_align_b, and with the thin
    kernel off; the counters of the first and the last lsp_b call"""
    sc, up, ps, tags = tc.build(name)
    monkeypatch.delenv("SPDP_B_THIN", raising=False)
    got, st = eng.lsp_b(sc, up, ps)
    same(got, wanted(name), (name, "thin"), tags)
    assert {k: st[k] for k in COUNTERS} == tc.predict(sc, up, ps, True), (name, st)
    same(eng.align_b(sc, up, ps), wanted(name), (name, "align_b"), tags)
    # the thin requests in the order given instead of sorted by length: other requests share a wave, the longest of a wave sits in any slot
    monkeypatch.setenv("SPDP_B_THIN_SORT", "0")
    got1, st1 = eng.lsp_b(sc, up, ps)
    monkeypatch.delenv("SPDP_B_THIN_SORT", raising=False)
    same(got1, wanted(name), (name, "SPDP_B_THIN_SORT=0"), tags)
    assert {k: st1[k] for k in COUNTERS} == tc.predict(sc, up, ps, True), (name, st1)
    monkeypatch.setenv("SPDP_B_THIN", "0")
    got0, st0 = eng.lsp_b(sc, up, ps)
    monkeypatch.delenv("SPDP_B_THIN", raising=False)
    same(got0, wanted(name), (name, "SPDP_B_THIN=0"), tags)
    assert st0["thin_requests"] == 0 and {k: st0[k] for k in COUNTERS} == tc.predict(sc, up, ps, False), (name, st0)
    assert st["cells"] == st0["cells"] == sum(ubr.cells(p, sc.sh) for p in ps.items if not tc.geometry(p, sc.sh)["host"]), name
    return st, st0


def check_group(eng, monkeypatch, group):
    """every recipe of the group; the thin kernel served exactly the generated cases of 1 .. 16 rows that need a DP cell"""
    n_thin = n_le16 = 0
    for name in tc.names(group):
        sc, up, ps, tags = tc.build(name)
        n_thin += check(eng, monkeypatch, name)[0]["thin_requests"]
        n_le16 += sum(1 for p, t in zip(ps.items, tags) if 1 <= t["rows"] <= 16 and t["cols"] >= 1 and not tc.geometry(p, sc.sh)["host"])
    assert n_thin == n_le16 > 0, (group, n_thin, n_le16)


def test_grid(eng, monkeypatch):
    """rows 1 .. 17 x cols 1 .. 64 and the transposed shapes: step counts across 16, 32, 48, 64 and every residue mod 4"""
    check_group(eng, monkeypatch, "grid")


def test_ends(eng, monkeypatch):
    """every end-flag tuple at every combination of sequence ends, tgapf 1, 0.5 and 0; a top edge steeper than the gap extension"""
    check_group(eng, monkeypatch, "ends")


def test_band(eng, monkeypatch):
    """band shoulders 100, 5, 2, 1 and -10 %: the band bounds the rows, the top boundary ends before the columns do"""
    check_group(eng, monkeypatch, "band")


def test_long_gaps(eng, monkeypatch):
    """both gap models at codonk1 3 and 7 with an indel of 1 .. 12 residues, at the start of the range too"""
    check_group(eng, monkeypatch, "long")


def test_local(eng, monkeypatch):
    """local at both ends, at one, at none; nothing positive; equal maxima on one row and on two"""
    check_group(eng, monkeypatch, "local")


def test_waves(eng, monkeypatch):
    """calls of exactly 1 .. 9 thin requests; very unlike members, local and global, in one wave"""
    for name in tc.names("waves"):
        st, _ = check(eng, monkeypatch, name)
        assert st["thin_requests"] == int(name.split("/")[2][1:]) and st["device_batches"] == 1, (name, st)


def test_rounds(eng, monkeypatch):
    """thin and tiled requests in one call; the same call in several launch sets; a thin-only call on a pool that an earlier,
    larger call has filled; the requests lspB_ng serves without a cell; a request above the budget"""
    for alpha in ("aa", "nt"):
        st, st0 = check(eng, monkeypatch, f"rounds/{alpha}/mixed")
        assert st["device_batches"] == 1 and st0["device_batches"] == 1 and st["thin_requests"] > 0 and st["wide_requests"] > 0
        sc, up, ps, tags = tc.build(f"rounds/{alpha}/mixed_tight")
        assert up.max_trace_bytes == max(eng.trace_bytes_b(p, sc.sh) for p in ps.items)
        st, st0 = check(eng, monkeypatch, f"rounds/{alpha}/mixed_tight")
        assert st["device_batches"] > 1 and st0["device_batches"] > 1, (st, st0)
        st, _ = check(eng, monkeypatch, f"rounds/{alpha}/without_cells")
        assert st["host_requests"] == 4 * 16 and st["thin_requests"] == 16
        # one byte below the largest tiled request's need: those requests come back not computed, the others as before
        need = [tc.thin_need(p, sc.sh) if t["rows"] <= 16 else tc.tiled_need(p, sc.sh) for p, t in zip(ps.items, tags)]
        tight = abi.UnsplicedParams(1.0, max(n for n, t in zip(need, tags) if t["rows"] > 16) - 1)
        with pytest.raises(RuntimeError, match="max_trace_bytes"):
            eng.lsp_b(sc, tight, ps)
        got, st = eng.lsp_b(sc, tight, ps, allow_partial=True)
        out = [i for i, n in enumerate(need) if n > tight.max_trace_bytes]
        assert out and st["requests_not_computed"] == len(out) == tc.predict(sc, tight, ps)["requests_not_computed"]
        for i, ((score, skl), (wscore, wskl)) in enumerate(zip(got, wanted(f"rounds/{alpha}/mixed_tight"))):
            assert (score, skl.tolist()) == ((abi.NEVSEL, []) if i in out else (wscore, wskl)), i
    st, _ = check(eng, monkeypatch, "rounds/big")
    assert st["wide_requests"] == 3
    st, _ = check(eng, monkeypatch, "rounds/after_big")
    assert st["thin_requests"] == 64 and st["wide_requests"] == 0


def test_bundles_are_refused_by_name(eng):
    sc, up, ps, _ = tc.build("waves/aa/n3/v0")
    for field, value in (("spj", 1), ("scalar_engines", 0)):
        with pytest.raises(RuntimeError, match=field):
            eng.lsp_b(defaults.scoring_b(**{field: value}), up, ps)
    with pytest.raises(RuntimeError, match="max_trace_bytes"):
        eng.lsp_b(sc, abi.UnsplicedParams(1.0, -1), ps)
    bad = abi.ProblemSet()
    bad._keep.append(ps)
    q = abi.Problem.from_buffer_copy(ps.items[0])
    q.a_left = q.a_right + 1
    bad.items.append(q)
    with pytest.raises(RuntimeError, match="a range outside the sequence"):
        eng.lsp_b(sc, up, bad)
