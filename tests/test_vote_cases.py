"""The recipes of tests/vote_cases.py held to the effects they are named for, by the oracle alone (no device): the longest list a
query votes with, the growths of each table, the phases a scan opens, the chromosomes among the candidate pairs, the calls
reached.  Prints the census: per class how many queries there are and how many reach each stop_at."""
import collections

import numpy as np
import pytest

from oracle import blk as oblk
from tests import vote_cases as vc

INDEXES = {ix["name"]: ix for ix in vc.all_indexes()}
# floors of the whole set: reaching queries per class, queries that do not reach the call they ask for, closing calls
MIN_REACHING, MIN_NOT_REACHING, MIN_FORCED = 10, 30, 20
MIN_REACHING_WIDE = 3
# A class is counted over the indexes that hold it: the growth classes (run_hash_0 .. 4, runs_0 .. 3, hits_3) are the growths of
# one table whatever the geometry and are pooled over the six grow geometries; every other class belongs to one index.
POOLED = ("run_hash_", "runs_", "hits_")


def by_class(index):
    per = collections.defaultdict(list)
    for c, e, m in vc.measured(index):
        per[c].append((e, m))
    return per


def test_census_and_floors(capsys):
    reach, not_reaching, forced, total = collections.Counter(), 0, 0, 0
    lines, stops = [], collections.defaultdict(set)
    for index in INDEXES.values():
        for c, v in by_class(index).items():
            got = [sum(1 for e, m in v if e["stop_at"] == s and m["want"] is not None) for s in range(5)]
            asked = [sum(1 for e, m in v if e["stop_at"] == s) for s in range(5)]
            reach[c] += sum(got); total += len(v)
            not_reaching += sum(m["want"] is None for _, m in v)
            forced += sum(m["forced"] for _, m in v)
            stops[c] |= {e["stop_at"] for e, _ in v}
            lines.append(f"{index['name']:14s} {c:12s} queries {len(v):3d}  reaching / asked per stop_at 0..4: " +
                         " ".join(f"{g}/{a}" for g, a in zip(got, asked)) + f"  closing calls {sum(m['forced'] for _, m in v)}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print(f"{len(reach)} classes on {len(INDEXES)} indexes, {total} queries, {sum(reach.values())} reach their call, "
              f"{not_reaching} do not, {forced} end in findblock's closing call")
    assert all(len(v) >= 3 for v in stops.values()), stops                          # several stop_at values per class
    held_by = collections.Counter(c for ix in INDEXES.values() for c in ix["classes"])
    assert all(n == 1 or c.startswith(POOLED) for c, n in held_by.items()), held_by
    assert all(n >= (MIN_REACHING_WIDE if c == "wide" else MIN_REACHING) for c, n in reach.items()), sorted(reach.items(), key=lambda x: x[1])[:3]
    # findblock makes four calls inside its scan at the most (the `notry` rule) and its closing call only when fewer were made:
    # a fifth call does not exist, the queries that ask for it are among those that do not reach their call
    assert not any(e["stop_at"] == 4 and m["want"] is not None for ix in INDEXES.values() for _, e, m in vc.measured(ix))
    assert not_reaching >= MIN_NOT_REACHING and forced >= MIN_FORCED
    # classes that hold queries which do not reach the asked call, and classes with closing calls: several of each
    assert sum(1 for ix in INDEXES.values() for v in by_class(ix).values() if any(m["want"] is None for _, m in v)) >= 5
    assert sum(1 for ix in INDEXES.values() for v in by_class(ix).values() if any(m["forced"] for _, m in v)) >= 5


@pytest.mark.parametrize("name", sorted(INDEXES))
def test_records_are_well_formed(name):
    index = INDEXES[name]
    ix = vc.oracle_index(index["fx"])
    nseg, n_chr, ncand = ix.nseg, ix.n_chr, ix.ncand
    for c, e, m in vc.measured(index):
        assert 0 <= e["left"] <= e["right"] <= len(e["codes"]) and 0 <= e["stop_at"] <= 4
        if m["want"] is None:
            assert not m["forced"] and m["calls"] <= e["stop_at"]
            continue
        assert m["calls"] == e["stop_at"] + 1
        w = oblk.split_recorded(*m["want"])
        assert w["head"].size == 20 and (w["head"][:4] >= 0).all()
        for d in range(4):
            assert len(w["qb"][d]) == w["head"][d] <= ncand
            assert all(0 < b < nseg for b, _ in w["qb"][d]) and all(0 <= b < nseg for b, _ in w["runs"][d])
        pairs = w["pairs"]
        assert len(pairs) <= ncand and int(m["want"][1][1]) == len(pairs)
        for bscr, chrom, lb, rb, ub, db, zl, zr, rvs in pairs:
            assert 0 <= chrom < n_chr and zr < nseg and rvs in (0, 1)
            # (the bracket index gives blocks to chromosomes that do not hold them: that is what it is for)
            assert name == "bracket" or zl <= ub <= lb <= rb <= db <= zr
        assert all(pairs[i][0] >= pairs[i + 1][0] for i in range(len(pairs) - 1))      # best first


def test_long_classes_vote_with_the_list_they_name():
    index = INDEXES["long"]
    per = by_class(index)
    for n in vc.LONG_MARKS:
        assert all(m["paths"]["longest"] == n for _, m in per[str(n)]), n
        more = sum(m["paths"]["more_chunks"] for _, m in per[str(n)])
        assert (more > 0) == (n > 64), (n, more)                                     # a second chunk from 65 entries on
    top = int(vc.list_lengths(index["fx"]).max())
    assert top > 256 and sum(m["paths"]["longest"] == top for _, m in per["longest"]) >= 3
    assert all(m["paths"]["zero_ended"] > 0 and m["paths"]["longest"] == 61 for _, m in per["end_mark"])
    # the element's own words: lists read in two chunks without any patching
    assert sum(64 < m["paths"]["longest"] < 128 for _, m in per["longest"]) >= 5


def test_merge_classes_merge_as_named():
    index = INDEXES["merge"]
    per = by_class(index)
    lens = vc.list_lengths(index["fx"])
    assert (lens > 64).sum() > 500 and (lens > 128).sum() > 200
    assert all(m["paths"]["lds_merges"] > 0 for _, m in per["lds"])
    assert all(m["paths"]["lane_merges"] > 0 for _, m in per["lane"])
    assert all(m["paths"]["zero_ended"] > 0 for _, m in per["zero"])
    share = {c: sum(m["paths"]["in_both"] for _, m in per[c]) / sum(m["paths"]["words"] for _, m in per[c]) for c in ("shared", "disjoint")}
    assert share["shared"] > 1.5 * share["disjoint"], share


def test_grow_classes_grow_the_table_under_test():
    seen = collections.Counter()
    for index in vc.grow_indexes():
        ms = vc.measured(index)
        for c, e, m in ms:
            table, k = c.rsplit("_", 1)
            assert table == index["table"] and min(4, m["grows"][table]) == int(k), (index["name"], c, m["grows"])
            seen[c] += 1
        # what the product will call TABLE: at most a tenth of the index's queries
        n_table = sum(max(m["grows"].values()) >= 4 for _, _, m in ms)
        assert n_table * vc.TABLE_SHARE <= len(ms), (index["name"], n_table, len(ms))
    assert {f"run_hash_{k}" for k in range(5)} <= set(seen) and any(c.startswith("runs_") and c[-1] in "123" for c in seen) and \
        any(c.startswith("hits_") and c[-1] in "123" for c in seen), seen
    # every table is met at its fourth growth or beyond by some query of the set
    assert seen["run_hash_4"] >= 10


def test_phases_indexes_open_the_phases_they_name():
    got = {}
    for index in vc.phases_indexes():
        ns = vc.prm_of(index["fx"], "nshift")
        got[index["name"]] = ns
        for c, e, m in vc.measured(index):
            assert m["paths"]["phases"] <= 4 * ns * m["rounds"]
        if index["name"] == "phases_epochs":
            # the epoch of the run hash is a byte: more than 255 phases in one scan bring it round (rounds x 4 directions x Nshift)
            over = [m for _, _, m in vc.measured(index) if m["paths"]["phases"] > 255]
            assert ns == 7 and len(over) >= 8 and all(m["rounds"] * 28 >= m["paths"]["phases"] for m in over)
    assert sorted(got.values()) == [1, 7, 12, 13, 32]


def test_chromosomes_appear_in_the_pairs():
    index = INDEXES["chromosomes"]
    fx = index["fx"]
    assert vc.prm_of(fx, "n_chr") == 300
    first = np.asarray(fx["blk_chr"]).reshape(-1, 2)[:, 1]
    starts_shared = sum(1 for c in range(1, 300) if first[c] == first[c - 1])
    assert starts_shared >= 20                                                     # chromosomes that begin in a block another one begins in
    chroms, nseg = set(), vc.prm_of(fx, "nseg")
    edge = collections.Counter()
    for c, e, m in vc.measured(index):
        if m["want"] is None:
            continue
        for p in oblk.split_recorded(*m["want"])["pairs"]:
            chroms.add(int(p[1]))
            edge["first"] += int(p[2]) <= 1; edge["last"] += int(p[3]) >= nseg - 1
    assert len(chroms) >= 30 and edge["first"] and edge["last"], (len(chroms), edge)


def test_protein_classes_vote_with_the_list_they_name_and_grow():
    index, small = vc.protein_indexes()
    assert vc.prm_of(index["fx"], "drna") == 0 and vc.prm_of(index["fx"], "hh_size1") > 100000
    per = by_class(index)
    for n in vc.P_MARKS:
        assert all(m["paths"]["longest"] == n for _, m in per[f"p_{n}"]), n
    got = by_class(small)
    assert {"p_run_hash_0", "p_run_hash_1", "p_run_hash_2"} <= set(got)
    for c, v in got.items():
        assert all(min(4, m["grows"]["run_hash"]) == int(c[-1]) for _, m in v), c


def test_bracket_class_tells_the_bracket_from_a_bisection():
    index = vc.bracket_index()
    assert len(index["blocks"]) >= 3
    differ = 0
    for c, e, m in vc.measured(index):
        plain = vc.measure(index["plain"], e)
        if m["want"] is not None and plain["want"] is not None:
            differ += not np.array_equal(m["want"][1], plain["want"][1])
    assert differ >= 10                                                            # the pairs name another chromosome


def test_wide_index_has_no_room_for_epochs():
    index = vc.wide_index()
    assert vc.prm_of(index["fx"], "nseg") >= 1 << 24
    b = np.asarray(index["fx"]["blk_blkb"])
    assert (b[b != 0] > 1 << 24).all()
    assert sum(m["want"] is not None for _, _, m in vc.measured(index)) >= MIN_REACHING_WIDE


def test_long_queries_pass_the_residue_cache():
    index = INDEXES["long_queries"]
    per = by_class(index)
    for n in (2047, 2048, 2049, 5000):
        assert all(len(e["codes"]) == n for e, _ in per[str(n)])
        assert {(e["left"] == 0, e["right"] == n) for e, _ in per[str(n)]} == {(True, True), (False, False), (False, True), (True, False)}
    shortq = vc.prm_of(index["fx"], "shortquery")
    assert sum(e["right"] - e["left"] < shortq and m["want"] is not None for e, m in per["short"]) >= 10
    assert sum(m["paths"]["phases"] == 0 for _, m in per["short"]) == 8              # too short for a word of every phase
