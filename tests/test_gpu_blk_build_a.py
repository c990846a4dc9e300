"""The amino-acid index of a protein database built on the device (spdp_blk_index_build_a, `spaln -W -KA`): against the program's own
files (the databases of the protein search fixtures and tests/golden/aa_idx_edge / _wide, byte for byte outside the bytes that hold
the program's heap), against the search (the vote and the hit lists do not change with whose index they run on), against the
restatement tests/aa_index_restate.py on parameters the program cannot be made to choose, and its refusals by name.

The heap bytes (tests/aa_index_restate.py has the reasons): the five pointers of ContBlk, the padding behind ConvTS, ContBlk::MaxBlk
(the program's files carry e.g. 17 746 for 300 sequences; the built index carries the longest kept list, and the program's number is
never smaller), ConvTab entries 0, 1, 2 and 23.

Not tested: "more than 2^32 - 1 residues" and "more postings than blkp can address" -- a database that large does not fit a test."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from spaln_amd import blocks, engine
from tests import aa_fixture as af
from tests import aa_index_cases as cases
from tests import aa_index_restate as air

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("blk_nblk", "nblk"), ("blk_wscr", "wscr"), ("blk_blkp", "blkp"), ("blk_blkb", "blkb"), ("blk_chr", "chrid"))


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def params_of(eng, prm):
    """the library's parameters for a case of tests/aa_index_cases.py (or the program's own choice)"""
    p = blocks.build_params_default_a(eng.lib, prm["total"])
    p.b.ktuple, p.b.nshift, p.b.bitpat, p.b.afact, p.b.maxgene, p.nalpha = prm["ktuple"], prm["nshift"], prm["bitpat"], prm["afact"], prm["maxgene"], prm["nalpha"]
    for i, v in enumerate(cases.class_table(prm["nalpha"])):
        p.convtab[i] = int(v)
    return p


def same_arrays(built, want):
    for a, b in PAIRS:
        assert np.array_equal(np.asarray(built[a]).astype(np.int64), np.asarray(want[b]).astype(np.int64)), a


# ---- 1. the program's files ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("a", "b", "edge", "wide"))
def test_the_built_file_is_the_programs(eng, tmp_path, name):
    seqs = air.golden_db(name)
    raw = air.golden_bka(name)
    want = air.parse(raw)
    codes, offs = air.encode_db(seqs)
    prm = blocks.build_params_default_a(eng.lib, want["glen"])
    assert (prm.nalpha, prm.b.ktuple, prm.b.nshift, prm.b.bitpat, prm.b.afact, prm.b.maxgene, prm.b.nbitpat, prm.convts) == \
        tuple(want[k] for k in ("nalpha", "ktuple", "nshift", "bitpat", "afact", "maxgene", "nbitpat", "convts")), name
    keep = [i for i in range(26) if i not in air.UNASSIGNED_CONVTAB]
    assert np.array_equal(np.frombuffer(bytes(prm.convtab), dtype=np.uint8)[keep], want["convtab"][keep])
    path = str(tmp_path / "built.bka")
    built, fprm, sec = blocks.build_index_a(eng, codes, offs, prm, write_to=path)
    mine = open(path, "rb").read()
    assert len(mine) == len(raw) and air.masked(mine) == air.masked(raw), (name, air.differences(air.parse(mine), want))
    same_arrays(built, want)
    assert built["blklen"] == want["blklen"] and built["nseg"] == len(seqs) + 1 and built["tabsize"] == want["tabsize"]
    assert want["maxblk"] >= built["maxblk"] == int(want["nblk"].max())
    assert len(sec) == 3 and sec[2] >= sec[0] > 0


# ---- 2. the search does not change with whose index it runs on ------------------------------------------------------------------------
@pytest.mark.parametrize("name", af.SETS)
@pytest.mark.parametrize("run", sorted(af.PW_RUNS))
def test_the_vote_is_the_same_on_the_built_index(eng, tmp_path, name, run):
    max_out, local = af.PW_RUNS[run]
    doc = af.search(name)
    queries = [af.encode(q["seq"]) for q in doc["queries"]]
    codes, offs = air.encode_db([d["seq"] for d in doc["db"]])
    read, fprm_r = blocks.read_protein_db_index(eng.lib, af.bka_path(name, str(tmp_path)), max_out=max_out, local=local)
    built, fprm_b, _ = blocks.build_index_a(eng, codes, offs, blocks.build_params_default_a(eng.lib, len(codes)), max_out=max_out, local=local)
    assert bytes(fprm_r) == bytes(fprm_b)
    out = []
    for arrays, fprm in ((read, fprm_r), (built, fprm_b)):
        ix = blocks.BlockIndex(eng, arrays)
        try:
            out.append(blocks.finds(ix, fprm, queries)[0])
        finally:
            ix.free()
    assert np.array_equal(out[0], out[1])
    assert sum(1 for r in out[1] if blocks.split_finds_record(r).get("cands")) > len(queries) // 3


@pytest.mark.parametrize("run", ("default", "M4_pw"))
def test_the_hit_lists_on_the_built_index_are_the_programs(eng, tmp_path, run):
    from tests import test_gpu_aa_search as gas
    max_out, local, qck, all_out = gas.RUNS[run]
    s = gas.Setup(eng, str(tmp_path), "a", max_out, local, qck)
    try:
        s.dix.free()
        arrays, s.fprm, _ = blocks.build_index_a(eng, s.db_codes, s.db_off, blocks.build_params_default_a(eng.lib, len(s.db_codes)), max_out=max_out, local=local)
        s.dix = blocks.BlockIndex(eng, arrays)
        got, _ = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries, all_out=bool(all_out))
    finally:
        s.free()
    want = s.doc["runs"][run]["o4"]
    n_hits = 0
    for q, hits in zip(s.doc["queries"], got):
        w = want.get(q["name"], [])
        assert gas.printed_form(s, hits) == [dict(b=r["b"], val=r["val"], corners=r["corners"]) for r in w], (run, q["name"], q["cls"])
        n_hits += len(hits)
    assert n_hits == sum(len(v) for v in want.values()) and n_hits > 0


# ---- 3. beyond what the program can be made to write: against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_other_parameters_equal_the_restatement(eng, tmp_path, name):
    seqs, prm, want = cases.restated(name)
    codes, offs = air.encode_db(seqs)
    path = str(tmp_path / "built.bka")
    built, fprm, _ = blocks.build_index_a(eng, codes, offs, params_of(eng, prm), write_to=path)
    got = air.parse(open(path, "rb").read())
    assert air.differences(got, want) == [] and got["maxblk"] == want["maxblk"] == built["maxblk"], name
    same_arrays(built, want)
    # one sequence: ln(segn) = 0, no word scores above the cut-off, every list is lost and there is no average score to search with
    assert (want["wordno"] == 0 and want["avrscr"] == 0 and fprm is None) if name == "single" else (want["wordno"] > 0 and fprm is not None)


# ---- 4. the refusals, each by its message -----------------------------------------------------------------------------------------------
def test_refusals_by_name(eng):
    good_codes, good_offs = air.encode_db(["MKWARNDCQEG", "ARNDCQEGHILK"])

    def refused(codes=good_codes, offs=good_offs, **over):
        p = blocks.build_params_default_a(eng.lib, 1000)
        for k, v in over.items():
            setattr(p if k in ("nalpha", "convts") else p.b, k, v)
        with pytest.raises(RuntimeError) as e:
            blocks.build_index_a(eng, codes, offs, p)
        return str(e.value)
    assert "more than 65 535" in refused(*air.encode_db(["AAA"] * 65536))
    assert "no counted residue" in refused(good_codes, np.array([0, 11, 11, 23], dtype=np.int64))
    assert "no counted residue" in refused(*air.encode_db(["MKWARND", "BBBB", "ARNDCQ"]))
    assert "one bit pattern" in refused(nbitpat=3)
    assert "3 .. 7 amino acids" in refused(ktuple=2, bitpat=3) and "3 .. 7 amino acids" in refused(ktuple=8, bitpat=255)
    assert "6 .. 20 classes" in refused(nalpha=21) and "6 .. 20 classes" in refused(nalpha=5)
    assert "weight is not k" in refused(bitpat=0b1111) and "weight is not k" in refused(bitpat=0b1110)
    assert "nshift out of range" in refused(nshift=0) and "nshift out of range" in refused(nshift=33)
    assert "at or beyond convts" in refused(np.array([3, 4, 26, 5], dtype=np.uint8), np.array([0, 4], dtype=np.int64))
    assert "at or beyond convts" in refused(convts=20)
    assert "start at 0" in refused(good_codes, np.array([1, 11, 23], dtype=np.int64))
    assert "decreases" in refused(good_codes, np.array([0, 12, 11, 23], dtype=np.int64))
    lib = eng.lib
    lib.spdp_blk_index_build_a.restype = C.c_void_p
    lib.spdp_blk_index_build_a.argtypes = [C.c_void_p] * 5
    assert lib.spdp_blk_index_build_a(eng.ctx, None, None, None, None) is None and b"null argument" in lib.spdp_last_error(eng.ctx)
    lib.spdp_blk_build_params_default_a.argtypes = [C.c_int64, C.c_void_p]
    assert lib.spdp_blk_build_params_default_a(1000, None) == -1 and lib.spdp_blk_build_params_default_a(0, C.byref(blocks.BlkBuildParamsA())) == -1
    # ... and the context still builds
    built, _, _ = blocks.build_index_a(eng, good_codes, good_offs, blocks.build_params_default_a(eng.lib, 23))
    assert built["nseg"] == 3


# ---- 5. the program searches with the library's file ---------------------------------------------------------------------------------------
def test_the_program_searches_with_our_index(eng):
    ref = os.path.join(ROOT, "oracle", "_ref", "spaln")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/spaln is not built")
    env = dict(os.environ, ALN_TAB=os.path.join(ROOT, "oracle", "_ref", "table"))
    rng = np.random.default_rng(77)
    db = ["".join(air.AA[i] for i in rng.integers(0, 20, size=int(n))) for n in rng.integers(60, 500, size=300)]
    queries = []
    for i in range(60):
        s = list(db[int(rng.integers(0, len(db)))])
        for j in np.flatnonzero(rng.random(len(s)) < 0.15):
            s[j] = air.AA[int(rng.integers(0, 20))]
        queries.append("".join(s))
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "prot.faa"), "w") as f:
            f.write("".join(f">p{i}\n{s}\n" for i, s in enumerate(db)))
        with open(os.path.join(td, "q.faa"), "w") as f:
            f.write("".join(f">q{i}\n{s}\n" for i, s in enumerate(queries)))
        r = subprocess.run([ref, "-W", "-KA", "-t1", "prot.faa"], cwd=td, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and os.path.exists(os.path.join(td, "prot.bka")), r.stderr[-300:]
        run = lambda: subprocess.run([ref, "-Q7", "-A0", "-O4", "-t1", "-aprot", "q.faa"], cwd=td, env=env, capture_output=True, text=True)
        a = run()
        assert a.returncode == 0 and a.stdout.count("XYL:") > 40, a.stderr[-300:]
        theirs = open(os.path.join(td, "prot.bka"), "rb").read()
        codes, offs = air.encode_db(db)
        os.remove(os.path.join(td, "prot.bka"))
        blocks.build_index_a(eng, codes, offs, blocks.build_params_default_a(eng.lib, len(codes)), write_to=os.path.join(td, "prot.bka"))
        mine = open(os.path.join(td, "prot.bka"), "rb").read()
        assert air.masked(mine) == air.masked(theirs)
        b = run()
        assert b.returncode == 0, b.stderr[-300:]
        assert b.stdout == a.stdout
