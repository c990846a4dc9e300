"""The fixtures of the unspliced aligner (tests/golden/b_aa_*.json.gz, written by tests/golden/make_b_goldens.py) as problems
and expected records, shared by the CPU and the GPU tests."""
import functools
import glob
import gzip
import json
import os

import numpy as np

from spaln_amd import abi, defaults, synth
from tools import b_pairs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = sorted(os.path.basename(p)[5:-8] for p in glob.glob(os.path.join(GOLDEN, "b_aa_*.json.gz")))


def encode(s: str) -> np.ndarray:
    return synth.encode_protein(np.frombuffer(s.encode(), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def load(name: str):
    with gzip.open(os.path.join(GOLDEN, f"b_aa_{name}.json.gz"), "rt") as f:
        return json.load(f)


def runs():
    """(set name, run index) of every option set of every fixture file"""
    return [(name, k) for name in SETS for k in range(len(load(name)["runs"]))]


def problems(name: str, k: int):
    """(scoring bundle, UnsplicedParams, ProblemSet, expected records) of one option set"""
    doc = load(name)
    run = doc["runs"][k]
    sc = defaults.scoring_b(noll=run["noll"], local=1 if run["lcl"] & 16 else 0)
    up = abi.UnsplicedParams(float(run["tgapf"]), 0)
    ps = abi.ProblemSet()
    for pr in doc["pairs"]:
        ps.add(encode(pr["a"]), encode(pr["b"]), None, None, exg=b_pairs.exg_of(run["lcl"]))
    return sc, up, ps, run["records"]


def check_record(stat, corners, rec, what):
    """a rescored alignment (stat dict, 0-based trimmed corners) against the program's printed record"""
    assert (np.asarray(corners) + 1).tolist() == rec["corners"], what
    assert stat["val"] == rec["val"], what
    assert abs(stat["val"] / defaults.B_SCALE - rec["score"]) <= 0.005 + 1e-9, what
    assert stat["mch"] == rec["mch"] and stat["mmc"] == rec["mmc"], what
    assert abs(stat["gap"] - rec["gap"]) <= 0.05 + 1e-6 and abs(stat["unp"] - rec["unp"]) <= 0.05 + 1e-6, what   # (printed with one decimal)
