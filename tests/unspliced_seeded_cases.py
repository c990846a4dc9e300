"""The fixtures of the unspliced aligner's seeded path (tests/golden/b_aas_<set>_q<n>.json.gz, written by
tests/golden/make_b_seeded_goldens.py) as problems and expected records, shared by the CPU and the GPU tests."""
import functools
import glob
import gzip
import json
import os

import numpy as np

from spaln_amd import abi, defaults
from tests import unspliced_cases as uc
from tools import b_pairs

GOLDEN = uc.GOLDEN
FILES = sorted(os.path.basename(p)[6:-8] for p in glob.glob(os.path.join(GOLDEN, "b_aas_*.json.gz")))      # "<set>_q<n>"


@functools.lru_cache(maxsize=None)
def load(name: str):
    with gzip.open(os.path.join(GOLDEN, f"b_aas_{name}.json.gz"), "rt") as f:
        return json.load(f)


def runs():
    """(file name, run index) of every option set of every fixture file"""
    return [(name, k) for name in FILES for k in range(len(load(name)["runs"]))]


def problems(name: str, k: int, first=None):
    """(scoring bundle, UnsplicedParams, SeedParams, ProblemSet, expected records, option strings) of one option set; first:
    only that many pairs"""
    doc = load(name)
    run = doc["runs"][k]
    sc = defaults.scoring_b(noll=run["noll"], local=1 if run["lcl"] & 16 else 0)
    up = abi.UnsplicedParams(float(run["tgapf"]), 0)
    sp = defaults.seed_params_b(run["qck"], run["lcl"])
    ps = abi.ProblemSet()
    pairs = doc["pairs"] if first is None else doc["pairs"][:first]
    for pr in pairs:
        ps.add(uc.encode(pr["a"]), uc.encode(pr["b"]), None, None, exg=b_pairs.exg_of(run["lcl"]))
    return sc, up, sp, ps, run["records"][:len(pairs)], run["opts"]


def check_alignment(stat, skl, cigar, rec, what):
    """one pair's result (skl = header + corners, stat of skl_rng_b, Cigar records as [[op, len] ..]) against the program's
    printed record; a pair the program printed nothing for must have come back without corners"""
    if rec is None:
        assert np.asarray(skl).reshape(-1, 2).shape[0] == 0, what
        return
    skl = np.asarray(skl).reshape(-1, 2)
    assert skl.shape[0] >= 3, what
    uc.check_record(stat, skl[stat["first"]:stat["first"] + stat["n_trim"]], rec, what)
    assert cigar == (rec["cigar"] or []), what          # (no Cigar line for an alignment without a leg)
