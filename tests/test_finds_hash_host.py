"""The finds vote's wave with its scores in the open-addressed table (spaln_amd/csrc/spdp_blk_finds.h, FindsWave::store = 1) on the
CPU: tests/finds_hash_host_check.cpp -- a program with its own main around the header's host flavour, with the grow-and-run-again
loop the library's host side has -- is built with -fsanitize=address,undefined and run on the text dump of every recipe of
tests/finds_cases.py, in order and reversed, with a first table of 64 slots and of 2^15.  Every int of every record must be the
restatement's, a run that filled its table must have written nothing, and the sanitizers must have nothing to say.  At 64 slots
the recipes of finds_store_cases.OVER_SMALL must run again.  No GPU; nothing is loaded into Python."""
import collections
import os
import subprocess

import pytest

from tests import finds_cases as fc
from tests import finds_store_cases as sc
from tests.test_finds_host import dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("finds_hash_host") / "finds_hash_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", out, os.path.join(ROOT, "tests", "finds_hash_host_check.cpp")])
    return out


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """the two dumps, written once: reversed -> (path, ids)"""
    out = {}
    for reverse in (False, True):
        text, ids = dump(reverse)
        path = tmp_path_factory.mktemp("finds_hash_dump") / "cases.txt"
        path.write_text(text)
        out[reverse] = (str(path), ids)
    return out


@pytest.mark.parametrize("slots", [64, 1 << 15])
@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "reversed"])
def test_every_recipe_equals_the_restatement(exe, dumps, reverse, slots):
    """reversed: the same records whatever the wave worked on before (the tags in tables of every size, run-hash epochs, the heap)"""
    path, ids = dumps[reverse]
    r = subprocess.run([exe, path, str(slots)], capture_output=True, text=True)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    bad = [(ids[int(f[0])], " ".join(f)) for f in lines if f[1] != "OK"]
    assert not bad, bad[:5]
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])      # a clean sanitizer exit
    assert len(lines) == len(ids)
    again, most, last = collections.Counter(), collections.Counter(), collections.Counter()
    for f in lines:
        name = ids[int(f[0])][0]
        again[name] += int(f[2])
        most[name] = max(most[name], int(f[3]))
        last[name] = max(last[name], int(f[4]))
    # the blocks a query scores do not depend on the table: the count is the same at both sizes and in both orders
    assert dict(most) == sc.MOST_BLOCKS
    if slots == sc.SMALL:
        for name in sc.MUST_OVERFLOW:
            assert name in sc.OVER_SMALL and most[name] > slots and again[name] >= 1, (name, most[name], again[name])
        assert sorted(n for n in fc.names() if again[n]) == sorted(sc.OVER_SMALL)
        assert all(last[n] >= most[n] and last[n] > slots for n in sc.OVER_SMALL)
    else:
        assert not any(again.values()) and set(last.values()) == {slots}


@pytest.mark.parametrize("slots", [64, 1 << 15])
def test_a_block_twice_in_a_list_ends_inside_the_table(exe, tmp_path, slots):
    """a malformed index: the lanes of a chunk that hold one block end on one slot; the run ends, no probe leaves the table"""
    rcp = fc.recipes()["lists_129"]
    fx = sc.twice_in_a_list("lists_129")
    text = [fc.dump_index(fx)]
    for k, (q, l, r) in enumerate(rcp["queries"]):
        text.append(fc.dump_query(k, q, l, r, rcp["out_cap"], []))
    path = tmp_path / "twice.txt"
    path.write_text("".join(text))
    r = subprocess.run([exe, str(path), str(slots), "any"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == len(rcp["queries"]) and all(f[1] == "OK" for f in lines)
