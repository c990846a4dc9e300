"""Every recipe of tests/finds_cases.py through the host emulation of the finds vote's wave: tests/finds_host_check.cpp (a program
with its own main around spaln_amd/csrc/spdp_blk_finds.h -- the very statements the kernel runs, a per-lane value an array of 64)
is built with -fsanitize=address,undefined and run on a text dump of the recipes; every int of every record must be the
restatement's and the sanitizers must have nothing to say.  No GPU; nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests import finds_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("finds_host") / "finds_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", out, os.path.join(ROOT, "tests", "finds_host_check.cpp")])
    return out


def dump(reverse: bool):
    text, ids = [], []
    for name in fc.names():
        rcp = fc.recipes()[name]
        text.append(fc.dump_index(rcp["fx"]))
        order = list(range(len(rcp["queries"])))
        for k in (reversed(order) if reverse else order):
            q, l, r = rcp["queries"][k]
            text.append(fc.dump_query(len(ids), q, l, r, rcp["out_cap"], fc.wanted_record(fc.wanted(name)[k], rcp["out_cap"])))
            ids.append((name, k))
    return "".join(text), ids


@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "reversed"])
def test_every_recipe_equals_the_restatement(exe, tmp_path, reverse):
    """reversed: the same records whatever the wave worked on before (slab tags, run-hash epochs, the heap's memory)"""
    text, ids = dump(reverse)
    path = tmp_path / "cases.txt"
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    bad = [(ids[int(ln.split()[0])], ln) for ln in lines if ln.split()[1] != "OK"]
    assert not bad, bad[:5]
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])      # a clean sanitizer exit
    assert len(lines) == len(ids)
