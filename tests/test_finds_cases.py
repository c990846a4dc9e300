"""Every recipe of tests/finds_cases.py held to the effect it is built to have, by the restatement alone (tests/finds_restate.py):
no product code, no GPU.  What the recipes are then used for -- the host emulation and the device vote against the same records --
is only worth something if the recipes do what they say."""
import collections

import pytest

from tests import finds_cases as fc
from tests import finds_restate as fr


@pytest.mark.parametrize("name", fc.names())
def test_recipe_has_its_effect(name):
    rcp = fc.recipes()[name]
    res = fc.wanted(name)
    assert len(res) == len(rcp["queries"])
    rcp["check"](rcp, res)
    for x in res:                               # what every result must be, whatever the recipe
        assert x["sigm"] <= rcp["fx"]["max_out"] + 10 and len(x["cands"]) == min(rcp["fx"]["max_out"], x["sigm"])
        scores = [s for _, s in x["heap"]]
        assert scores == sorted(scores, reverse=True)


def test_at_least_ten_cases_per_class():
    n = collections.Counter()
    for rcp in fc.recipes().values():
        n[rcp["cls"]] += len(rcp["queries"])
    want = {"phase", "endings", "ambiguous", "ubiquitous", "lists", "family", "ties", "tiny_sequences", "local", "geometry"}
    assert want <= set(n) and all(n[c] >= 10 for c in want), n


def test_both_endings_occur():
    res = fc.wanted("endings")
    ix = fc.restate_index(fc.recipes()["endings"]["fx"])
    assert any(x["nmmc"] == 1 for x in res) and any(x["nmmc"] == ix.maxmmc for x in res)


def test_run_hash_sizes_cover_both_homes():
    """the small tables live in the wave's LDS and have collisions (more blocks than slots is possible); one recipe has the
    program's large table, which lives in the slab"""
    sizes = {name: rcp["fx"]["hh_size"] for name, rcp in fc.recipes().items()}
    assert min(sizes.values()) * 8 <= 24 << 10 < max(sizes.values()) * 8
    assert any(rcp["fx"]["nseg"] > rcp["fx"]["hh_size"] for rcp in fc.recipes().values())


def test_the_cut_record():
    rcp = fc.recipes()["cut"]
    for x in fc.wanted("cut"):
        rec = fc.wanted_record(x, rcp["out_cap"])
        assert len(rec) == rcp["out_cap"] and rec[2] & fr.CUT
