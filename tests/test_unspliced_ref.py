"""The restatement of the unspliced aligner (tests/unspliced_ref) against what the program printed (tests/golden/b_aa_*.json.gz):
corner lists, fstat and the Cigar; the rescoring identity that proves the protein-pair parameters of defaults.py; the
score-only engine against the forward engine."""
import numpy as np
import pytest

from spaln_amd import abi, defaults
from tests import unspliced_cases as uc
from tests import unspliced_ref as ubr


@pytest.fixture(scope="module")
def restated():
    """per option set: the restatement's (score, skl, stat, trimmed corners, cigar records) of every pair, computed once"""
    out = {}
    for name, k in uc.runs():
        sc, up, ps, recs = uc.problems(name, k)
        rows = []
        for p in ps.items:
            score, skl = ubr.align(sc, up, p)
            stat, trimmed, ed, _ = ubr.rescore(sc, up, p, skl, abi.FMT_CIGAR)
            rows.append((score, skl, stat, trimmed, ed))
        out[(name, k)] = rows
    return out


def test_fixture_sets_are_complete():
    assert {"shapes1", "shapes2", "mid", "long", "tgapf", "local"} <= set(uc.SETS)
    for name in ("shapes1", "shapes2"):
        doc = uc.load(name)
        assert len(doc["pairs"]) == 48
        assert sorted((r["lcl"], r["noll"]) for r in doc["runs"]) == sorted((l, n) for l in (15, 0, 3, 5, 10) for n in (2, 3))
    assert len(uc.load("mid")["pairs"]) == 12 and len(uc.load("long")["pairs"]) == 2
    for doc in (uc.load(n) for n in uc.SETS):
        for run in doc["runs"]:
            assert len(run["records"]) == len(doc["pairs"])
    for pr in uc.load("local")["pairs"]:
        assert min(len(pr["a"]), len(pr["b"])) >= 5


@pytest.mark.parametrize("name,k", uc.runs())
def test_restatement_gives_the_programs_record(restated, name, k):
    _, _, _, recs = uc.problems(name, k)
    for i, ((score, skl, stat, trimmed, ed), rec) in enumerate(zip(restated[(name, k)], recs)):
        what = f"{name} run {k} pair {i}"
        assert skl.shape[0] >= 3, what
        uc.check_record(stat, trimmed, rec, what)
        assert [[chr(o), int(l)] for o, l, _ in ed] == (rec["cigar"] or []), what      # (no Cigar line for an alignment without a leg)


@pytest.mark.parametrize("name,k", [(n, k) for n, k in uc.runs() if not uc.load(n)["runs"][k]["lcl"] & 16])
def test_rescoring_identity_proves_the_parameters(restated, name, k):
    """with all ends global (-L0) and tgapf = 1 the engine's score is the corner list's score recomputed with the parameters of
    defaults.py -- gap terms, matrix and band alike.  (Free ends: the engine does not charge what skl_rngB_ng trims away or
    charges; tgapf != 1: forwardB_ng truncates the factor per gap position, skl_rngB_ng per gap, and lastB_ng prices a closing
    end gap by its own rule -- there the two differ in the reference itself, e.g. 379 against 514 on pair 6 of the -yt0.5 set.)
    The recomputed val equals the program's printed one on every set."""
    run = uc.load(name)["runs"][k]
    for i, (score, skl, stat, trimmed, ed) in enumerate(restated[(name, k)]):
        if run["lcl"] == 0 and run["tgapf"] == 1.0:
            assert score == stat["val"], (name, k, i)
        assert stat["val"] == run["records"][i]["val"]


def test_tgapf_is_honoured_by_the_program():
    """-yt0.5 changes records of the global set: the fixtures do test tgapf != 1"""
    sc, up, ps, recs = uc.problems("tgapf", 0)
    assert up.tgapf == 0.5
    up1 = abi.UnsplicedParams(1.0, 0)
    differ = 0
    for p, rec in zip(ps.items, recs):
        score, skl = ubr.align(sc, up1, p)
        stat, trimmed, _, _ = ubr.rescore(sc, up1, p, skl)
        differ += (trimmed + 1).tolist() != rec["corners"] or stat["val"] != rec["val"]
    assert differ > 0


# (scorealoneB_ng does not read tgapf: the two engines agree at 1.0 only)
@pytest.mark.parametrize("name,k", [(n, k) for n, k in uc.runs() if uc.load(n)["runs"][k]["tgapf"] == 1.0])
def test_scorealone_equals_the_forward_score(restated, name, k):
    sc, up, ps, _ = uc.problems(name, k)
    for i, p in enumerate(ps.items):
        assert ubr.scorealone(sc, up, p) == restated[(name, k)][i][0], (name, k, i)
