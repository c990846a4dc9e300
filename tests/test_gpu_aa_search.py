"""Protein queries against a protein database in one call (spdp_map_align_b) against the program's own records: the fixtures
tests/golden/aa_search_<set>.json.gz hold what `spaln -Q4 .. -Q7 -A0 -O4 [-M4] [-pw] [-LS -M2 -pw] -a<db>` printed (and -O0 for the
default options).  Per query the ordered hit list must be the program's: names, the printed score, the corners as -O4 prints them,
mch / mmc / gap / unp where -O0 recorded them.  Reads only tests/golden/."""
import ctypes as C
import os

import numpy as np
import pytest

from spaln_amd import abi, blocks, defaults, engine
from tests import aa_fixture as af

pytestmark = pytest.mark.gpu

# run of the fixture -> (MaxOut, local, qck, all_out)
RUNS = {"default": (1, 0, 3, 0), "M4": (4, 0, 3, 0), "M4_pw": (4, 0, 3, 1), "LS_M2_pw": (2, 1, 3, 1), "Q4": (1, 0, 0, 0), "Q5": (1, 0, 1, 0),
        "Q6": (1, 0, 2, 0), "H160": (1, 0, 3, 0), "H270": (1, 0, 3, 0)}
# -H<thr>: Vthr = thr x alprm.scale.  Set b holds a pair of engine score 1667 and fstat.val 1565 and one of 2688 and 2722: the program holds
# Vthr against fstat.val (Gsinfo::scr after skl_rngB_ng, src/spaln.cc:684, 915), so the first is not printed at 1600, the second is at 2700
VTHR = {"H160": 1600, "H270": 2700}


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class Setup:
    """what a run of a set needs: the resident index, the database as the entry takes it, the bundles"""

    def __init__(self, eng, tmp, name, max_out, local, qck, vthr=None):
        self.doc = af.search(name)
        arrays, self.fprm = blocks.read_protein_db_index(eng.lib, af.bka_path(name, tmp), max_out=max_out, local=local)
        self.dix = blocks.BlockIndex(eng, arrays)
        seqs = [af.encode(d["seq"]) for d in self.doc["db"]]
        self.db_off = np.zeros(len(seqs) + 1, dtype=np.int64)
        self.db_off[1:] = np.cumsum([len(s) for s in seqs])
        self.db_codes = np.concatenate(seqs)
        self.lcl = 16 if local else 15
        self.sc = defaults.scoring_b(local=1 if local else 0)
        self.up = abi.UnsplicedParams(1.0, 0)
        self.model = defaults.wilip_model_b()
        self.sp = defaults.seed_params_b(qck, self.lcl)
        self.sp.wilip = C.addressof(self.model)
        if vthr is not None:
            self.sp.vthr = int(vthr)
        self.queries = [af.encode(q["seq"]) for q in self.doc["queries"]]

    def free(self):
        self.dix.free()


def segments(corners):
    """the (m, n, length) triples -O4 prints: the diagonal stretches between the corners, 1-based"""
    out = []
    for (m0, n0), (m1, n1) in zip(corners[:-1], corners[1:]):
        if m1 - m0 == n1 - n0 and m1 > m0:
            out += [int(m0) + 1, int(n0) + 1, int(m1 - m0)]
    return out


def printed_form(s: Setup, hits):
    return [dict(b=s.doc["db"][h["seq"]]["name"], val="%.1f" % (h["val"] / defaults.B_SCALE), corners=segments(h["corners"].tolist())) for h in hits]


@pytest.mark.parametrize("name,run", [("a", r) for r in RUNS if r not in VTHR] + [("b", r) for r in ("default", "M4", "M4_pw", "LS_M2_pw", "H160", "H270")])
def test_hit_lists_are_the_programs(eng, tmp_path, name, run):
    max_out, local, qck, all_out = RUNS[run]
    s = Setup(eng, str(tmp_path), name, max_out, local, qck, VTHR.get(run))
    try:
        got, sec = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries, all_out=bool(all_out))
        stats = blocks.finds_stats(eng)
    finally:
        s.free()
    want = s.doc["runs"][run]["o4"]
    lens = {d["name"]: len(d["seq"]) for d in s.doc["db"]}
    n_hits = 0
    for q, hits in zip(s.doc["queries"], got):
        w = want.get(q["name"], [])
        assert printed_form(s, hits) == [dict(b=r["b"], val=r["val"], corners=r["corners"]) for r in w], (name, run, q["name"], q["cls"])
        for r in w:                                     # the ranges the program prints are the sequences' own
            assert r["a_rng"] == [1, len(q["seq"])] and r["b_rng"] == [1, lens[r["b"]]]
        n_hits += len(hits)
    assert n_hits == sum(len(v) for v in want.values()) and n_hits > 0
    # the stats are arithmetic on the fixture
    assert stats["refused_short"] == len(s.doc["refused"]) and stats["searched"] == len(s.queries) - len(s.doc["refused"])
    ix = af.index(name, max_out, local)
    from tests import finds_restate as fr
    assert stats["candidates"] == sum(min(max_out, fr.finds(ix, q)["sigm"]) for q, d in zip(s.queries, s.doc["queries"]) if d["name"] not in s.doc["refused"])
    # -O0 of the same run: fstat of every printed record, and the ranges.  The program prints the sequences' own ranges (Seq::left + 1,
    # right: the whole query, the whole database sequence) in -O4 and -O0 alike; the entry returns the ALIGNED range, first corner to
    # last -- which in the program's output is where the first (m, n, length) triple of -O4 begins and the last one ends
    o0 = {(f[13], f[14]): f for f in s.doc["runs"][run]["o0"]}
    assert len(o0) == n_hits
    for q, hits in zip(s.doc["queries"], got):
        for h, r in zip(hits, want.get(q["name"], [])):
            f = o0[(q["name"], s.doc["db"][h["seq"]]["name"])]
            assert ("%.2f" % h["val"], "%.1f" % h["mch"], "%.1f" % h["mmc"], "%.1f" % h["gap"], "%.1f" % h["unp"]) == (f[1], f[2], f[3], f[4], f[5]), (q["name"], f)
            assert f[7:13] == ["1", str(len(q["seq"])), "+", "1", str(lens[r["b"]]), "+"]
            t = r["corners"]
            assert (h["a_rng"][0] + 1, h["b_rng"][0] + 1) == (t[0], t[1]), (q["name"], h["a_rng"], h["b_rng"], t[:3])
            assert (h["a_rng"][1], h["b_rng"][1]) == (t[-3] + t[-1] - 1, t[-2] + t[-1] - 1), (q["name"], h["a_rng"], h["b_rng"], t[-3:])
            assert 0 <= h["a_rng"][0] < h["a_rng"][1] <= len(q["seq"]) and 0 <= h["b_rng"][0] < h["b_rng"][1] <= lens[r["b"]]
    if run == "H160":
        assert not got[1] and s.doc["queries"][1]["name"] == "q1"
    if run == "H270":
        assert got[8] and s.doc["queries"][8]["name"] == "q8"


def test_one_call_equals_its_steps_and_the_thin_sweep_changes_nothing(eng, tmp_path):
    """spdp_blk_finds, spdp_align_b_seeded and spdp_skl_rng_b called one by one give the hits of the one call; SPDP_B_THIN=0 too"""
    max_out, local, qck, all_out = RUNS["M4"]
    s = Setup(eng, str(tmp_path), "a", max_out, local, qck)
    try:
        got, _ = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries)
        os.environ["SPDP_B_THIN"] = "0"
        try:
            tiled, _ = blocks.map_align_b(s.dix, s.db_codes, s.db_off, s.sc, s.up, s.sp, s.fprm, s.queries)
        finally:
            del os.environ["SPDP_B_THIN"]
        searched = [i for i, q in enumerate(s.queries) if len(q) >= 9]
        recs, _ = blocks.finds(s.dix, s.fprm, [s.queries[i] for i in searched])
        ps, owner = abi.ProblemSet(), []
        from tools import b_pairs
        for k, i in enumerate(searched):
            for c in blocks.split_finds_record(recs[k]).get("cands", []):
                ps.add(s.queries[i], s.db_codes[s.db_off[c]:s.db_off[c + 1]], None, None, exg=b_pairs.exg_of(s.lcl))
                owner.append((i, c))
        alns = eng.align_b_seeded(s.sc, s.up, s.sp, ps, model=s.model)
        st = eng.skl_rng_b(s.sc, s.up, ps, [a for _, a in alns])
    finally:
        s.free()
    steps = [[] for _ in s.queries]
    for (i, c), (score, skl), t in zip(owner, alns, st):
        steps[i].append((c, score, skl, t))
    for i, hits in enumerate(got):
        cand = steps[i]
        odr = []
        for n, x in enumerate(cand):
            v = x[3]["val"] if x[2].shape[0] >= 3 else 0
            m = len(odr)
            while m > 0 and v > (cand[odr[m - 1]][3]["val"] if cand[odr[m - 1]][2].shape[0] >= 3 else 0):
                m -= 1
            odr.insert(m, n)
        n_out = min(max_out, sum(1 for x in cand if x[2].shape[0] >= 3 and x[3]["val"] > s.sp.vthr))      # (Gsinfo::scr = fstat.val by then)
        mine = [(cand[k][0], cand[k][1], cand[k][3]["val"], cand[k][2][cand[k][3]["first"]:cand[k][3]["first"] + cand[k][3]["n_trim"]].tolist())
                for k in odr[:n_out] if cand[k][2].shape[0] >= 3]
        assert [(h["seq"], h["score"], h["val"], h["corners"].tolist()) for h in hits] == mine, i
        for h in hits:                                  # the ranges: first corner to last
            assert (h["a_rng"][0], h["b_rng"][0]) == tuple(h["corners"][0]) and (h["a_rng"][1], h["b_rng"][1]) == tuple(h["corners"][-1])
        assert [(h["seq"], h["val"], h["corners"].tolist()) for h in tiled[i]] == [(h["seq"], h["val"], h["corners"].tolist()) for h in hits]


def test_refusals_by_name(eng, tmp_path):
    s = Setup(eng, str(tmp_path), "b", 1, 0, 3)
    try:
        def refused(**kw):
            a = dict(index=s.dix, db_codes=s.db_codes, seq_off=s.db_off, sc=s.sc, up=s.up, sp=s.sp, fprm=s.fprm, queries=s.queries[:2])
            a.update(kw)
            with pytest.raises(RuntimeError) as e:
                blocks.map_align_b(**a)
            return str(e.value)
        assert "sequence count differs" in refused(seq_off=s.db_off[:-1])
        assert "longer than 65535" in refused(queries=[s.queries[0], np.full(65536, 3, dtype=np.uint8)])
        other = abi.BlkFindsParams.from_buffer_copy(s.fprm)
        other.max_out = 4
        assert "Ncand != MaxOut + 10" in refused(fprm=other)
        bad = defaults.scoring_b()
        bad.spj = 1
        assert "spj" in refused(sc=bad)
        nix = blocks.BlockIndex(eng, blocks.read_index_file(eng.lib, os.path.join(af.GOLDEN, "blk_k3.bkn")))
        try:
            assert "nucleotide index" in refused(index=nix)
        finally:
            nix.free()
        lib = eng.lib
        assert lib.spdp_map_align_b(eng.ctx, s.dix.h, None, None, None, None, None, None, None, None, 1, 0, None, None, None, None) == -1
        assert b"null argument" in lib.spdp_last_error(eng.ctx)
    finally:
        s.free()


def test_live_against_the_program():
    """tools/aa_search.py: a fresh database formatted by the program, 300 queries, the program's run against one spdp_map_align_b
    call (the fixtures above are the pin that never skips)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "oracle", "_ref", "spaln")):
        pytest.skip("oracle/_ref/spaln is not built")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "aa_search.py"), "--queries", "300", "--repeat", "1"], capture_output=True, text=True, timeout=600)
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert r.returncode == 0 and d["identical"] == 300 and d["of"] == 300, (d, r.stderr[-600:])
    assert d["library_aligned"] == d["reference_aligned"] > 100
