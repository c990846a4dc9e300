"""The words pass of the amino-acid index builder on the CPU: tests/aa_index_host_check.cpp (a program with its own main: the tiles,
threads and prefix maximum of blkidx_words_a around the product's per-residue rule, spaln_amd/csrc/spdp_blk_build_a.h) is built with
-fsanitize=address,undefined and run on a text dump of every fixture and of the cases of tests/aa_index_cases.py; the word counts
and the sorted unique (word, block) set must be the restatement's, and the sanitizers must have nothing to say.  No GPU; nothing is
loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import aa_index_cases as cases
from tests import aa_index_restate as air

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("aa_index_host") / "aa_index_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", out, os.path.join(ROOT, "tests", "aa_index_host_check.cpp")])
    return out


def dump(seqs, prm):
    """what the device is handed: the codes without the residues the scan skips, the offsets, the rule"""
    table = cases.class_table(prm["nalpha"])
    codes, offs = air.encode_db(seqs)
    keep = table[codes] <= prm["nalpha"]
    new_offs = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), offs[:-1]))]) if len(codes) else offs
    codes = codes[keep]
    exam = [w for w in range(32) if prm["bitpat"] >> w & 1]
    width = max(exam) + 1
    cls = np.full(32, prm["nalpha"] + 1, dtype=np.int64)
    cls[:26] = table
    return "\n".join(["R " + " ".join(str(x) for x in [prm["nalpha"], len(exam), width, int(width > len(exam)), prm["nshift"]] + exam),
                      "T " + " ".join(str(int(x)) for x in cls),
                      "S " + " ".join(str(int(x)) for x in [len(seqs)] + new_offs.tolist()),
                      "C " + str(len(codes)) + " " + " ".join(map(str, codes.tolist()))]) + "\n"


@pytest.mark.parametrize("name", ("a", "b", "edge", "wide") + cases.NAMES)
def test_counts_and_keys_equal_the_restatement(exe, tmp_path, name):
    seqs, prm, want = cases.restated(name)
    path = tmp_path / "case.txt"
    path.write_text(dump(seqs, prm))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])      # a clean sanitizer exit
    rows = np.array([[int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln[0] == "T"], dtype=np.int64).reshape(-1, 2)
    keys = np.array([[int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln[0] == "K"], dtype=np.int64).reshape(-1, 2)
    tcount = np.zeros_like(want["tcount"])
    tcount[rows[:, 0]] = rows[:, 1]
    assert np.array_equal(tcount, want["tcount"]), name
    wanted_keys = sorted((w, b + 1) for b, blk in enumerate(want["blocks"]) for w in blk)
    assert [tuple(k) for k in keys.tolist()] == wanted_keys, name
