"""What holds the scores of the finds vote on the device (spdp_blk_finds, DESIGN.md 5b "What holds rscr"): the slab of nseg + 1
slots a wave, or the open-addressed table keyed by block (SPDP_FINDS_RSCR=hash; above 2^24 blocks the only form).  The records
must not depend on the form, on the table's size or on how often a query had to be run again: every recipe of
tests/finds_cases.py against the restatement under the table form, a first table of 64 slots that most recipes overflow, both forms
byte for byte on batches, the program's own index files, a database of more than 2^24 sequences, and one map + align call.
spdp_blk_finds_store_stats says what a call did."""
import numpy as np
import pytest

from spaln_amd import blocks, engine
from tests import aa_fixture as af
from tests import finds_cases as fc
from tests import finds_restate as fr
from tests import finds_store_cases as sc
from tests.test_gpu_finds_cases import library_arrays, params_of, same_records

pytestmark = pytest.mark.gpu
WIDE = 1 << 24


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def search(eng, fx, queries, out_cap=64):
    """a fresh index of fx (the form is read from the environment when an index is first searched), one finds call -> records, stats"""
    dix = blocks.BlockIndex(eng, library_arrays(fx))
    try:
        got, ms = blocks.finds(dix, params_of(fx), [q for q, _, _ in queries], ranges=[(l, r) for _, l, r in queries], out_cap=out_cap)
        stats = blocks.finds_store_stats(eng)
    finally:
        dix.free()
    assert ms > 0
    return got, stats


@pytest.mark.parametrize("name", fc.names())
def test_every_recipe_equals_the_restatement_under_the_table(eng, name, monkeypatch):
    """the default first table (2^15 slots) holds every query of the recipes: one launch, nothing run again"""
    monkeypatch.setenv("SPDP_FINDS_RSCR", "hash")
    rcp = fc.recipes()[name]
    got, st = search(eng, rcp["fx"], rcp["queries"], rcp["out_cap"])
    same_records(got, [fc.wanted_record(x, rcp["out_cap"]) for x in fc.wanted(name)], name)
    flagged = [k for k in range(got.shape[0]) if got[k, 2] & (fr.TABLE | fr.CUT)]
    assert flagged == (list(range(got.shape[0])) if name == "cut" else []), (name, flagged)
    assert st["form"] == 1 and st["launches"] == 1 and st["rerun_queries"] == 0 and st["first_slots"] == st["last_slots"] == 1 << 15, st
    searched = any(not x["flags"] & fr.SHORT for x in fc.wanted(name))
    assert st["most_blocks"] == (sc.MOST_BLOCKS[name] if searched else 0), st


@pytest.mark.parametrize("name", sc.OVER_SMALL)
def test_a_full_table_is_run_again_and_leaves_no_trace(eng, name, monkeypatch):
    """a first table of 64 slots under queries that score more blocks than that (tests/test_finds_hash_host.py counts them)"""
    monkeypatch.setenv("SPDP_FINDS_RSCR", "hash")
    monkeypatch.setenv("SPDP_FINDS_RSCR_SLOTS", str(sc.SMALL))
    rcp = fc.recipes()[name]
    got, st = search(eng, rcp["fx"], rcp["queries"], rcp["out_cap"])
    same_records(got, [fc.wanted_record(x, rcp["out_cap"]) for x in fc.wanted(name)], name)
    assert not any(got[k, 2] & (fr.TABLE | fr.CUT) for k in range(got.shape[0]))
    assert st["form"] == 1 and st["first_slots"] == sc.SMALL and st["rerun_queries"] >= 1 and st["launches"] >= 2, st
    assert st["last_slots"] > st["first_slots"] and st["last_slots"] >= st["most_blocks"] == sc.MOST_BLOCKS[name], st


def test_the_first_table_is_rounded_up_to_a_power_of_two_of_at_least_64(eng, monkeypatch):
    rcp = fc.recipes()["edge_ns3"]
    monkeypatch.setenv("SPDP_FINDS_RSCR", "hash")
    for asked, slots in (("1", 64), ("65", 128), ("1000", 1024)):
        monkeypatch.setenv("SPDP_FINDS_RSCR_SLOTS", asked)
        _, st = search(eng, rcp["fx"], rcp["queries"])
        assert st["first_slots"] == slots, (asked, st)
    monkeypatch.setenv("SPDP_FINDS_RSCR", "neither")
    with pytest.raises(RuntimeError, match="SPDP_FINDS_RSCR is neither slab nor hash"):
        search(eng, rcp["fx"], rcp["queries"])


def test_a_block_twice_in_a_list_ends(eng, monkeypatch):
    """a malformed index (tests/test_finds_hash_host.py runs the same under the sanitizers): the call returns, every query searched"""
    monkeypatch.setenv("SPDP_FINDS_RSCR", "hash")
    monkeypatch.setenv("SPDP_FINDS_RSCR_SLOTS", str(sc.SMALL))
    rcp = fc.recipes()["lists_129"]
    got, st = search(eng, sc.twice_in_a_list("lists_129"), rcp["queries"])
    assert all(got[k, 2] & fr.REACHED and got[k, 0] >= 6 for k in range(got.shape[0])) and st["rerun_queries"] >= 1, st


@pytest.fixture(scope="module")
def mixed():
    """the construction of tests/test_gpu_finds_cases.py: queries of two recipes on one index, refused ones among them"""
    rcp, edge = fc.recipes()["phase_ns3"], fc.recipes()["edge_ns3"]
    qs = rcp["queries"] + edge["queries"]
    want = [fc.wanted_record(x, 64) for x in fc.wanted("phase_ns3") + fc.wanted("edge_ns3")]
    assert any(w[2] & fr.SHORT for w in want)
    return rcp["fx"], qs, want


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_both_forms_byte_for_byte_on_batches_and_their_reversal(eng, mixed, n, monkeypatch):
    fx, qs, want = mixed
    pick = [(7 * k + 3) % len(qs) for k in range(n)]
    out = {}
    for form, code in (("slab", 0), ("hash", 1)):
        monkeypatch.setenv("SPDP_FINDS_RSCR", form)
        dix = blocks.BlockIndex(eng, library_arrays(fx))
        try:
            for order in (pick, pick[::-1]):
                got, _ = blocks.finds(dix, params_of(fx), [qs[i][0] for i in order], ranges=[qs[i][1:] for i in order])
                st = blocks.finds_store_stats(eng)
                assert st["form"] == code and st["launches"] == 1 and (st["first_slots"] > 0) == bool(code), (form, st)
                same_records(got, [want[i] for i in order], (form, n, order is pick))
                out[form, order is pick] = got
        finally:
            dix.free()
    for fwd in (True, False):
        assert out["slab", fwd].tobytes() == out["hash", fwd].tobytes()


@pytest.mark.parametrize("name", af.SETS)
@pytest.mark.parametrize("max_out,local", [(1, 0), (4, 0), (2, 1)])
def test_the_programs_indexes_under_the_table(eng, tmp_path, name, max_out, local, monkeypatch):
    """the index files `spaln -W -KA` wrote (their run hash lives in the wave's area, beside the table)"""
    monkeypatch.setenv("SPDP_FINDS_RSCR", "hash")
    arrays, prm = blocks.read_protein_db_index(eng.lib, af.bka_path(name, str(tmp_path)), max_out=max_out, local=local)
    ix = af.index(name, max_out, local)
    queries = [af.encode(q["seq"]) for q in af.search(name)["queries"]]
    want = [fr.record(fr.finds(ix, q)) for q in queries]
    dix = blocks.BlockIndex(eng, arrays)
    try:
        got, _ = blocks.finds(dix, prm, queries, out_cap=64)
        st = blocks.finds_store_stats(eng)
    finally:
        dix.free()
    same_records(got, want, (name, max_out, local))
    assert not any(got[k, 2] & (fr.TABLE | fr.CUT) for k in range(got.shape[0]))
    assert st["form"] == 1 and st["rerun_queries"] == 0, st


def wide_index(fx: dict) -> dict:
    """fx's database behind 2^24 sequences of one residue: no words, one block each.  Every block number of the postings and the
    first blocks of the sequence table move up by 2^24; the bracket of findChrNo stays (it falls back to the whole table)"""
    out = dict(fx)
    chr_tab = np.asarray(fx["blk_chr"], dtype=np.int64).reshape(-1, 2)
    front = np.stack([np.arange(WIDE, dtype=np.int64), np.arange(1, WIDE + 1, dtype=np.int64)], axis=1)
    out["blk_chr"] = np.concatenate([front, chr_tab + WIDE]).astype(np.int32).reshape(-1)
    blkb = np.asarray(fx["blk_blkb"], dtype=np.uint32)
    out["blk_blkb"] = np.where(blkb != 0, blkb + np.uint32(WIDE), blkb).astype(np.uint32)
    out["nseg"], out["n_chr"] = int(fx["nseg"]) + WIDE, int(fx["n_chr"]) + WIDE
    return out


def wide_record(rec: list) -> list:
    """a record of the recipe with 2^24 added to every block and sequence number"""
    out = list(rec)
    if not out[2] & fr.REACHED or out[2] & fr.SHORT:
        return out
    sigm = out[5]
    for i in range(sigm):
        out[6 + 2 * i] += WIDE
    at = 6 + 2 * sigm
    for k in range(at + 1, at + 1 + out[at]):
        out[k] = out[k] + WIDE if out[k] >= 0 else out[k] - WIDE
    return out


def test_a_database_of_more_than_2_24_sequences(eng, monkeypatch):
    name = "family_m4"
    rcp = fc.recipes()[name]
    fx = wide_index(rcp["fx"])
    assert fx["nseg"] - 1 > WIDE
    want = [wide_record(fc.wanted_record(x, rcp["out_cap"])) for x in fc.wanted(name)]
    assert all(w[6] > WIDE and w[6 + 2 * w[5] + 1] >= WIDE for w in want)
    dix = blocks.BlockIndex(eng, library_arrays(fx))
    try:
        qs, rng = [q for q, _, _ in rcp["queries"]], [(l, r) for _, l, r in rcp["queries"]]
        monkeypatch.setenv("SPDP_FINDS_RSCR", "slab")
        with pytest.raises(RuntimeError, match=r"a database of more than 2\^24 blocks \(the score slab of a wave holds 8 bytes a block\)"):
            blocks.finds(dix, params_of(fx), qs, ranges=rng, out_cap=rcp["out_cap"])
        monkeypatch.delenv("SPDP_FINDS_RSCR")            # unset: the table above 2^24 blocks
        got, ms = blocks.finds(dix, params_of(fx), qs, ranges=rng, out_cap=rcp["out_cap"])
        st = blocks.finds_store_stats(eng)
    finally:
        dix.free()
    same_records(got, want, "wide")
    assert not any(got[k, 2] & (fr.TABLE | fr.CUT) for k in range(got.shape[0]))
    assert st["form"] == 1 and st["area_bytes"] < 4_000_000 and st["rerun_queries"] == 0 and st["most_blocks"] == sc.MOST_BLOCKS[name], st


def test_map_align_under_the_table_gives_the_slabs_hit_lists(eng, tmp_path, monkeypatch):
    """spdp_map_align_b reaches the vote through spdp_blk_finds: the smaller search fixture, default options, both forms"""
    from tests.test_gpu_aa_search import RUNS, Setup, printed_form
    max_out, local, qck, all_out = RUNS["default"]
    lists = {}
    for form in ("slab", "hash"):
        monkeypatch.setenv("SPDP_FINDS_RSCR", form)
        s = Setup(eng, str(tmp_path), "b", max_out, local, qck)
        try:
            got, _ = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries, all_out=bool(all_out))
            st = blocks.finds_store_stats(eng)
        finally:
            s.free()
        assert st["form"] == (form == "hash"), st
        lists[form] = [[(h["seq"], h["a_rng"], h["b_rng"], h["score"], h["val"], h["corners"].tolist()) for h in hits] for hits in got]
        want = s.doc["runs"]["default"]["o4"]
        for q, hits in zip(s.doc["queries"], got):
            assert printed_form(s, hits) == [dict(b=r["b"], val=r["val"], corners=r["corners"]) for r in want.get(q["name"], [])], (form, q["name"])
    assert lists["slab"] == lists["hash"] and any(lists["hash"])
