"""Dispersed loci end to end (tools/e2e_dispersed.py): cDNA queries joined from the transcripts of two different genes -- whole +
whole, whole + first third, last quarter + whole -- and unjoined controls, against a genome of 40 planted genes.  `spaln -Q7 -O4 -pr`
of the compiled reference (oracle/_ref/spaln: test infrastructure, prebuilt) aligns a query, looks at which stretch of it was
covered and searches the genome again with what is left over on each side; spdp_map_align_s_dispersed / _h_dispersed must report the
same records in the same order.  The data must be able to tell the feature from its absence: the program prints records from left
and from right rests, two or more for most joined queries, and the entry that reports one locus per query reports fewer than the
program for at least one query.  Each case is one run of the tool as a child process.

`part` and `covered` are held to quick4's rule (spdp_dispersed_rests) and blkaln's narrowing (tools/e2e_dispersed.py,
parts_against_rests): part 0 first, the parts ascending; `covered` equal to the range of the first record wherever the first search
aligned one locus, which is where the output determines it; a record of part 1 / 2 only where the rule gives a left / right rest
for `covered`, with its far end inside that rest and more of it inside the rest than outside.  That it lies wholly INSIDE the rest,
as the issue of this feature asked, does not hold for the program's own records (on these cases 33 of 113 rest records of the cDNA
sets and 8 of 25 of the protein set reach past the rest at the end towards the covered stretch: by 1 or 2 residues mostly, by 25
where the covered stretch cuts into a gene): the block search looks for words inside the range, but Wlp::eval extends an HSP back to
the query's first residue and forward to its tlen whatever the range is (src/wln.cc:365-367, 383, 394, 404).  DESIGN.md 5b says the
same."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "S1": (["--ori", "1"], 120, 30, 2),
    "default-orientation": (["--ori", "3"], 120, 30, 2),
    "S1-tails-prep": (["--ori", "1", "--tails"], 120, 30, 2),
    "default-orientation-T-heads-prep": (["--ori", "3", "--tails"], 120, 30, 2),    # (a third of the queries: antisense reads the preparation turns)
    "protein": (["--protein"], 60, 20, 4),          # (the share of joined queries with two records: a half, for proteins a quarter)
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_record_of_spaln_pr(case):
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "spaln")) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "spaln_blktap")):
        pytest.skip("oracle/_ref/spaln and spaln_blktap are not built")
    extra, joined, controls, share = CASES[case]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e_dispersed.py"), "--joined", str(joined), "--controls", str(controls),
                        "--genes", "40"] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-600:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(d))
    n = joined + controls
    assert d["queries"] == n and d["joined"] == joined and d["controls"] == controls
    # every query's record list is the program's, and so are the counts
    assert d["identical_of_all_queries"] == n and d["different"] == 0, (d, r.stderr[-800:])
    assert d["library_records"] == d["reference_records"]
    # the data: both kinds of rest, two records for most joined queries
    assert d["reference_left_rest_records"] >= 1 and d["reference_right_rest_records"] >= 1
    assert d["joined_with_two_or_more_records"] * share >= joined, d
    # every control: one record, the single entry's
    assert d["controls_with_one_record_equal_to_the_single_entry"] == controls
    # part 0 first; `covered` the first record's range where one locus was aligned; the rests' records on the ranges
    # spdp_dispersed_rests gives for `covered`, far end inside, the overhang shorter than what lies inside (the module's docstring)
    assert d["parts_inconsistent"] == []
    assert 2 * d["covered_held_exactly"] >= d["library_queries"], d
    assert d["turned_by_the_preparation"] == (n // 3 if extra == ["--ori", "3", "--tails"] else 0)
    # without the feature a query gets fewer records than the program prints
    assert d["single_entry_fewer_records"] >= 1
    assert d["return_code"] == 0


@pytest.fixture(scope="module")
def small():
    """the set-up of tests/test_gpu_e2e.py::test_one_call_equals_its_steps on the blk_k1 fixture: inputs the entry accepts"""
    from oracle import blk
    from spaln_amd import abi, blocks, engine
    from tests import spdg
    from tests.conftest import golden_files
    from tests.test_blk_find import CASES as BLK_CASES, genome_of
    name, n_genes, seed, par = [c for c in BLK_CASES if c[0] == "blk_k1"][0]
    eng = engine.Engine(0)
    fx = spdg.load([f for f in golden_files("blk_") if f.endswith(name + ".spdg")][0])
    fq = spdg.load(os.path.join(ROOT, "tests", "golden", "q_c2_seed0.spdg"))
    gen, off = genome_of(name, n_genes, seed, par)
    dix = blocks.BlockIndex(eng, fx)
    model = abi.wilip_model_from_fixture(fx)
    sc = spdg.scoring(fq, intpen=np.ascontiguousarray(fx["find_intpen"], dtype=np.int16), scalar_engines=1, llmt=model.llmt, minl=model.minl)
    sp = abi.seed_params_from_fixture(fq)
    sp.minl, sp.ip_maxl = model.minl, model.maxl
    sp.wilip = C.addressof(model)
    fs = fq["rng_fstat_A0"] if "rng_fstat_A0" in fq else [0, 0, 0, 0, 0, 0, 3, 1]
    queries = [q["codes"][q["left"]:q["right"]] for q in blk.parse_log(fx)][:8]
    yield dict(eng=eng, dix=dix, gen=gen, off=off, sc=sc, sp=sp, sig=abi.signal_model_from_fixture(fq), prm=blocks.find_params_from_fixture(fx),
               model=model, rescore=(fq["prm"]["codonk1"], model.minl, int(fs[6]), int(fs[7])), queries=queries)
    dix.free()
    eng.close()


def _stats(s):
    v = (C.c_int64 * 12)()
    s["eng"].lib.spdp_seeded_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    s["eng"].lib.spdp_seeded_stats(s["eng"].ctx, v, 12)
    return list(v)


@pytest.mark.parametrize("what,message", [("max_out", "max_out must be 1"), ("min_seg_len", "min_seg_len must be > 0"), ("q_mns", "q_mns = 2")])
def test_refused_calls_launch_nothing(small, what, message):
    from spaln_amd import blocks
    s = small
    prm = blocks.BlkFindParams.from_buffer_copy(s["prm"])
    assert prm.max_out == 1
    kw = dict(min_seg_len=21, ori=1, prep=None)
    if what == "max_out":
        prm.max_out, prm.max_out2 = 2, max(2, prm.max_out2)
    elif what == "min_seg_len":
        kw["min_seg_len"] = 0
    else:
        kw["prep"] = (2, 12)
    before = _stats(s)
    with pytest.raises(RuntimeError) as e:
        blocks.map_align_dispersed(s["dix"], s["gen"], s["off"], s["sc"], s["sp"], s["sig"], prm, s["rescore"], s["queries"], **kw)
    assert message in str(e.value), str(e.value)
    assert _stats(s) == before                      # no seeded call has run


def test_the_same_inputs_are_served(small):
    """... and with the three values in order the call runs: unjoined queries, one record each, part 0, covered inside the query"""
    from spaln_amd import blocks
    s = small
    lists, covered, sec, rc, rec = blocks.map_align_dispersed(s["dix"], s["gen"], s["off"], s["sc"], s["sp"], s["sig"], s["prm"], s["rescore"],
                                                             s["queries"], min_seg_len=21, ori=1)
    assert rc == 0 and rec is None and len(lists) == len(s["queries"]) and covered.shape == (len(s["queries"]), 2)
    assert sum(1 for lst in lists if lst) >= len(s["queries"]) // 2
    for lst, cov, q in zip(lists, covered, s["queries"]):
        assert [g["part"] for g in lst[:1]] == [0] * len(lst[:1])
        assert 0 <= cov[0] <= cov[1] <= len(q)
        assert len(lst) <= 3


@pytest.mark.parametrize("what,message", [("max_out", "max_out must be 1"), ("min_seg_len", "min_seg_len must be > 0")])
def test_the_protein_twin_refuses_the_same(small, what, message):
    """the two checks stand in front of everything the entry reads: the cDNA set-up's structs are never looked at"""
    from spaln_amd import blocks
    s = small
    prm = blocks.BlkFindParams.from_buffer_copy(s["prm"])
    if what == "max_out":
        prm.max_out, prm.max_out2 = 2, max(2, prm.max_out2)
    before = _stats(s)
    with pytest.raises(RuntimeError) as e:
        blocks.map_align_h_dispersed(s["dix"], s["gen"], s["off"], s["sc"], s["sp"], s["sig"], prm, s["sc"], s["queries"],
                                     0 if what == "min_seg_len" else 12)
    assert "spdp_map_align_h_dispersed" in str(e.value) and message in str(e.value), str(e.value)
    assert _stats(s) == before
