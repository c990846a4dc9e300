"""The block vote on the device (spdp_blk_vote) on the indexes of tests/vote_cases.py: every record against the oracle's, int for
int, and the kernel's own path counters (spdp_blk_vote_stats) against what the oracle walked -- the counters say that the second
chunk, both merges, the split of a chunk, the one-lane path under a growing table, the epoch wipe and the uncached query ran."""
import os

import numpy as np
import pytest

from oracle import blk as oblk
from spaln_amd import blocks, engine
from tests import vote_cases as vc

pytestmark = pytest.mark.gpu
OUT_CAP = 1 << 13


def _header_constant(name):
    """a #define of spaln_amd/csrc/spdp_blk_dev.h"""
    import re
    txt = open(os.path.join(os.path.dirname(os.path.abspath(blocks.__file__)), "csrc", "spdp_blk_dev.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", txt).group(1))


RES_CAP = _header_constant("SPDP_BLK_RES_CAP")                  # residues of a query a wave keeps in LDS
HASH_LEVELS = _header_constant("SPDP_BLK_HASH_LEVELS")          # the growth of one table that ends a query as TABLE


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class env:
    """environment variables set for a block, put back afterwards"""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def vote(eng, index, entries, out_cap=OUT_CAP, **knobs):
    """a fresh BlockIndex (SPDP_BLK_HH_LDS is read when it is made), one vote call -> records, counters"""
    with env(**knobs):
        dix = blocks.BlockIndex(eng, index["fx"])
        try:
            out, _ = dix.vote([e["codes"] for e in entries], [(e["left"], e["right"]) for e in entries], [e["stop_at"] for e in entries],
                              out_cap=out_cap)
            return out, dix.vote_stats()
        finally:
            dix.free()


def check_records(index, out, ms, tag=""):
    """every record against the oracle's: head, run lists in heap order, all pairs, the run scores around them, calls, reached,
    FORCED; TABLE exactly where one table of the oracle's call grew four times or more (nothing else asked of those)"""
    ix = vc.oracle_index(index["fx"])
    n_table = 0
    for i, (c, e, m) in enumerate(ms):
        where = (index["name"], c, i, tag)
        flags = int(out[i, 2])
        want_table = max(m["grows"].values()) >= blocks_levels()
        assert bool(flags & blocks.TABLE) == want_table, where + (m["grows"],)
        if want_table:
            n_table += 1
            continue
        assert not flags & blocks.CUT, where
        got = blocks.split_record(out[i])
        assert got["calls"] == m["calls"], where + (got["calls"], m["calls"])
        if m["want"] is None:
            assert not got["reached"] and not flags & blocks.FORCED, where
            continue
        assert got["reached"] and bool(flags & blocks.FORCED) == m["forced"], where
        w = oblk.split_recorded(*m["want"])
        assert np.array_equal(got["head"], w["head"]), where
        assert all(np.array_equal(a, b) for a, b in zip(got["qb"], w["qb"])), where
        assert np.array_equal(got["pairs"], m["want"][1][2:].reshape(-1, 9)), where
        assert got["runs"] == [sorted(x) for x in oblk.runs_near_pairs(ix, w["runs"], got["pairs"])], where
    return n_table


def blocks_levels():
    return HASH_LEVELS


def host_counts(index, ms):
    """the counters the host can tell from the tables and the oracle, for an index none of whose queries ends as TABLE"""
    fx = index["fx"]
    width, ns = int(fx["blk_bitpat"][1]), vc.prm_of(fx, "nshift")
    paths = lambda k: sum(m["paths"][k] for _, _, m in ms)
    return dict(queries=len(ms), zero_ended=paths("zero_ended"),
                lds_merges=paths("lds_merges"), lane_merges=paths("lane_merges"), hash_growths=sum(m["grows"]["run_hash"] for _, _, m in ms),
                # the epoch of the run hash is a byte and every query starts at its end: a wipe at the first phase, then every 255th
                # (block numbers of 2^24 and more leave no room for the epoch: every phase wipes)
                wipes=sum(m["paths"]["phases"] if vc.prm_of(fx, "nseg") >= 1 << 24 else -(-m["paths"]["phases"] // 255) for _, _, m in ms),
                hbm_queries=sum(len(e["codes"]) > RES_CAP and e["right"] - e["left"] - (ns + width) >= 1 for _, e, _ in ms), table=0)


def assert_same_records(out, first, where):
    """byte for byte, but for the queries ended as TABLE: of those only that they ended so"""
    assert np.array_equal(out[:, 2] & blocks.TABLE, first[:, 2] & blocks.TABLE), where
    plain = (first[:, 2] & blocks.TABLE) == 0
    differ = np.nonzero((out[plain] != first[plain]).any(axis=1))[0]
    assert differ.size == 0, where + (np.nonzero(plain)[0][differ][:8].tolist(),)


def run_index(eng, index, nonzero=(), **knobs):
    ms = vc.measured(index)
    out, stats = vote(eng, index, [e for _, e, _ in ms], **knobs)
    n_table = check_records(index, out, ms)
    print(index["name"], stats)
    assert stats["table"] == n_table and stats["queries"] == len(ms)
    if not n_table:
        want = host_counts(index, ms)
        assert {k: stats[k] for k in want} == want, index["name"]
    for k in nonzero:
        assert stats[k] > 0, (index["name"], k, stats)
    return out, stats


def test_long_lists_are_read_chunk_by_chunk(eng):
    _, stats = run_index(eng, vc.long_index(), nonzero=("splits", "lane_entries", "hash_growths", "zero_ended"))
    # (the kernel does not count words and chunks, which its inner loops would pay for: that these queries read second chunks is
    # the oracle's to say)
    assert sum(m["paths"]["more_chunks"] for _, _, m in vc.measured(vc.long_index())) > 500
    assert stats["lds_merges"] == stats["lane_merges"] == 0      # (kk = 1: nothing to merge)


def test_two_lists_are_merged_both_ways(eng):
    run_index(eng, vc.merge_index(), nonzero=("lds_merges", "lane_merges", "zero_ended", "splits"))


@pytest.mark.parametrize("which", range(len(vc.GROW_GEOMETRIES)))
def test_tables_grow_and_give_up_like_the_oracle_says(eng, which):
    """... with a wave per CU and the batch repeated until there are several queries per wave: a query that ended as TABLE is
    followed on its wave by ordinary ones, which must be right"""
    index = vc.grow_indexes()[which]
    ms = vc.measured(index)
    reps = -(-1200 // len(ms))
    entries = [e for _, e, _ in ms] * reps
    out, stats = vote(eng, index, entries, SPDP_BLK_WAVES_PER_CU=1)
    n_table = reps * check_records(index, out[:len(ms)], ms)
    for r in range(1, reps):                                    # (the repeats: the records of the first round again)
        assert_same_records(out[r * len(ms):(r + 1) * len(ms)], out[:len(ms)], (index["name"], "repeat", r))
    print(index["name"], stats)
    assert stats["table"] == n_table and stats["queries"] == len(entries)
    assert n_table * vc.TABLE_SHARE <= len(entries)
    table = index["table"]
    assert stats[{"run_hash": "hash_growths", "hits": "hits_growths", "runs": "runs_growths"}[table]] > 0
    if table == "run_hash":
        assert stats["lane_entries"] > 0
        if index["name"] != "grow_hh127":
            assert n_table > 0
    if not n_table:
        want = host_counts(index, ms)
        assert {k: stats[k] for k in want} == {k: v * reps for k, v in want.items()}


@pytest.mark.parametrize("which", range(5))
def test_many_phases(eng, which):
    index = vc.phases_indexes()[which]
    ns = vc.prm_of(index["fx"], "nshift")
    _, stats = run_index(eng, index, nonzero=("wipes",) + (("no_prefetch",) if ns > 12 else ()))
    assert (stats["no_prefetch"] > 0) == (ns > 12)
    if index["name"] == "phases_epochs":
        assert stats["wipes"] > stats["queries"]                 # the epoch came round within a query


def test_many_chromosomes(eng):
    run_index(eng, vc.chromosomes_index())


def test_queries_longer_than_the_residue_cache(eng):
    _, stats = run_index(eng, vc.long_queries_index(), nonzero=("hbm_queries",))
    assert stats["hbm_queries"] == 24                            # the classes of 2049 and 5000 residues


@pytest.mark.parametrize("name", ["long", "grow_hh7", "grow_hh13", "grow_hh31", "grow_hb", "grow_ha"])
def test_placement_and_scheduling_do_not_matter(eng, name):
    """level 0 of the run hash in LDS or in HBM, one wave per CU or sixteen, the batch reversed: the same records byte for byte
    (a query ended as TABLE says no more than that)"""
    index = next(ix for ix in vc.all_indexes() if ix["name"] == name)
    entries = [e for _, e, _ in vc.measured(index)]
    first, _ = vote(eng, index, entries)
    for knobs in (dict(SPDP_BLK_HH_LDS=0), dict(SPDP_BLK_HH_LDS=1), dict(SPDP_BLK_WAVES_PER_CU=1), dict(SPDP_BLK_WAVES_PER_CU=16)):
        out, _ = vote(eng, index, entries, **knobs)
        assert_same_records(out, first, (name, str(knobs)))
    out, _ = vote(eng, index, entries[::-1])
    assert_same_records(out[::-1], first, (name, "reversed"))


def test_protein_queries_on_the_translated_index(eng):
    """level 0 of the run hash in HBM as the index has it (157 291 slots), and at 31 slots, where it grows"""
    index, small = vc.protein_indexes()
    run_index(eng, index, nonzero=("splits",))
    run_index(eng, small, nonzero=("hash_growths", "lane_entries"))


def test_bracket_of_the_chromosome_search(eng):
    run_index(eng, vc.bracket_index())


def test_block_numbers_beyond_the_epoch_byte(eng):
    """nseg >= 2^24: no epochs, every phase wipes the run hash; one wave, its slab a GiB"""
    index = vc.wide_index()
    _, stats = run_index(eng, index, SPDP_BLK_SLAB_GB=1)
    assert stats["wipes"] == sum(m["paths"]["phases"] for _, _, m in vc.measured(index)) > 5 * 28


def test_largest_record_is_cut_without_a_write_past_its_row(eng):
    """the query with the largest record, out_cap one below its length, through the resident entry into the first row of a
    two-row buffer filled with a pattern: CUT, and the second row -- which no query owns -- keeps every int of the pattern"""
    import ctypes as C
    index = vc.merge_index()
    ms = vc.measured(index)
    out, _ = vote(eng, index, [e for _, e, _ in ms])
    big = int(np.argmax(out[:, 0]))
    n = int(out[big, 0])
    assert n > 60 and not int(out[big, 2]) & blocks.CUT
    e = ms[big][1]
    cap = n - 1
    hip = blocks._hip_runtime()
    host = [np.ascontiguousarray(e["codes"], dtype=np.uint8), np.array([0, len(e["codes"])], dtype=np.int64), np.array([e["left"]], dtype=np.int32),
            np.array([e["right"]], dtype=np.int32), np.array([e["stop_at"]], dtype=np.int32), np.full((2, cap), 0x5a5a5a5a, dtype=np.int32)]
    bufs = [C.c_void_p() for _ in host]
    dix = blocks.BlockIndex(eng, index["fx"])
    try:
        for b, a in zip(bufs, host):
            assert hip.hipMalloc(C.byref(b), C.c_size_t(max(a.nbytes, 16))) == 0
            assert hip.hipMemcpy(b, a.ctypes.data, C.c_size_t(a.nbytes), 1) == 0
        dix.vote_resident(*bufs[:5], 1, bufs[5], cap)
        got = np.zeros((2, cap), dtype=np.int32)
        assert hip.hipMemcpy(got.ctypes.data, bufs[5], C.c_size_t(got.nbytes), 2) == 0
    finally:
        dix.free()
        for b in bufs:
            if b:
                hip.hipFree(b)
    assert int(got[0, 2]) & blocks.CUT and int(got[0, 0]) == cap
    assert np.array_equal(got[0, 3:23], out[big, 3:23])          # (what fits is what the full record holds)
    assert (got[1] == 0x5a5a5a5a).all()
