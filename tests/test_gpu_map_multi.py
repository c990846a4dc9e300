"""Map + align with every locus `spaln -M N` prints (spdp_map_align_s_multi / _h_multi and their group forms): the printed
locus lists of the compiled reference recorded by tests/golden/make_map_multi_goldens.py -- a cDNA genome with every gene twice
(-S1 and both orientations) and a protein one, -M4 with a raised output threshold -H, with and without -pw -- against the
library's, on genomes regenerated from their seeds and indexes made by the library's own builders."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spaln_amd import abi, blocks, engine, synth
from tests import spdg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_blk_goldens as mb  # noqa: E402

CODE_OF = np.zeros(256, dtype=np.uint8)                  # 1 + the set of bases a letter stands for (A = 1, C = 2, G = 4, T = 8); N = 16
for _ch, _code in zip(b"ACMGRSVTWYHKDBN", range(2, 17)):
    CODE_OF[_ch] = _code


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class Case:
    """one fixture's genome, queries, index (made for max_out) and the parameters the recorded program held"""

    def __init__(self, eng, name, max_out=4):
        fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
        self.setup, self.runs, self.z_scores = fx["setup"], fx["runs"], fx["scores"]
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.z = {k: z[k] for k in z.files}
        st = self.setup
        self.protein = st["protein"]
        chroms, queries = (mb.protein_genome_and_queries if self.protein else mb.paralog_genome_and_queries)(st["n_genes"], st["n_chr"], st["seed"])
        self.gen = np.concatenate([CODE_OF[c] for c in chroms]).astype(np.uint8)
        self.off = np.array([0] + list(np.cumsum([len(c) for c in chroms])), dtype=np.int64)
        self.names = [f"q{i}" for i in range(len(queries))]
        self.chr_names = st["chr_names"]
        ext = int(self.z["blk_prm"][blocks._PRM["extblock"]])
        if self.protein:
            bp = blocks.build_params_default_p(eng.lib, st["fasta_bytes"], threaded=st["threaded"])
            self.fx, _ = blocks.build_index_p(eng, self.gen, self.off, bp, ext_block=ext, max_out=max_out)
            self.queries = [synth.encode_protein(np.asarray(q, dtype=np.uint8)) for q in queries]
        else:
            bp = blocks.build_params_default(eng.lib, st["fasta_bytes"], 1, threaded=st["threaded"])
            self.fx, _ = blocks.build_index(eng, self.gen, self.off, bp, ext_block=ext, max_out=max_out)
            self.queries = [CODE_OF[np.asarray(q, dtype=np.uint8)] for q in queries]
        self.fx["blk_convtab"][:2] = 255
        self.ix = blocks.BlockIndex(eng, self.fx)
        self.model = abi.wilip_model_from_fixture(self.z)
        ip = np.ascontiguousarray(self.z["find_intpen"], dtype=np.int16)
        llmt, minl, _rlmt, maxl = (int(x) for x in self.z["cli_intron_prm"][:4])
        if self.protein:
            fq = spdg.load(os.path.join(GOLDEN, "live_h_q7555.spdg" if self.model.crs else "qh_0013.spdg"))
            fsig = fq if "pm5_f32" in fq else spdg.load(os.path.join(GOLDEN, "h1_basic.spdg"))
            self.sc = spdg.scoring_h(fq, intpen=ip, llmt=llmt, minl=minl)
            self.sc.scalar_engines = 1
            self.sp = abi.seed_params_from_fixture(fq)
            self.sp.qck = 3
            self.sigmodel = abi.signal_model_h_from_fixture(fsig)
            rp = [int(x) for x in fq["rparams"]]
            hp = dict(zip(spdg.HPARAM_NAMES, (int(x) for x in fq["hparams"])))
            self.rescore = abi.RescoreParamsH(minl, rp[4], hp["lcl"], rp[1])
        else:
            fq = spdg.load(os.path.join(GOLDEN, "q_c2_seed0.spdg"))
            self.sc = spdg.scoring(fq, intpen=ip, scalar_engines=1, llmt=llmt, minl=minl)
            self.sp = abi.seed_params_from_fixture(fq)
            self.sigmodel = abi.signal_model_from_fixture(fq)
            fs = fq["rng_fstat_A0"] if "rng_fstat_A0" in fq else [0, 0, 0, 0, 0, 0, 3, 1]
            self.rescore = (fq["prm"]["codonk1"], minl, int(fs[6]), int(fs[7]))
        self.sp.minl, self.sp.ip_maxl = minl, maxl
        # PwdB::Vthr = thr x Vab; the block search's vthr = scale x 2 x thr (src/blksrc.cc:2210), Vab = scale for both query kinds
        self.sp.vthr = int(self.z["find_prm"][0]) // 2
        self.sp.wilip = C.addressof(self.model)
        self.prm = blocks.find_params_from_fixture(self.z)
        self.prm.phase1t = int(self.ix.desc.rbscons)
        self.prm.max_out, self.prm.max_out2 = max_out, max(max_out, st["max_out2"])

    def multi(self, all_out, ori=1, prm=None):
        if self.protein:
            return blocks.map_align_h_multi(self.ix, self.gen, self.off, self.sc, self.sp, self.sigmodel, prm or self.prm, self.rescore,
                                            self.queries, all_out=all_out)
        return blocks.map_align_multi(self.ix, self.gen, self.off, self.sc, self.sp, self.sigmodel, prm or self.prm, self.rescore,
                                      self.queries, ori=ori, all_out=all_out)

    def best(self, ori=1):
        if self.protein:
            return blocks.map_align_h(self.ix, self.gen, self.off, self.sc, self.sp, self.sigmodel, self.prm, self.rescore, self.queries)
        return blocks.map_align(self.ix, self.gen, self.off, self.sc, self.sp, self.sigmodel, self.prm, self.rescore, self.queries, ori=ori)

    def as_printed(self, lists):
        return {self.names[i]: [[self.chr_names[g["chr"]], "-" if g["rvs"] else "+", [list(e) for e in g["exons"]]] for g in lst]
                for i, lst in enumerate(lists) if lst}

    def free(self):
        self.ix.free()


RUNS = [("map_multi_par", "S1", 1), ("map_multi_par", "S3", 3), ("map_multi_p1", "P", 1)]


@pytest.mark.parametrize("all_out", [False, True], ids=["threshold", "pw"])
@pytest.mark.parametrize("name,run,ori", RUNS, ids=[r[1] for r in RUNS])
def test_locus_lists_equal_the_recorded_program(eng, name, run, ori, all_out):
    """every query's ordered list of loci (chromosome, strand, exon table) = what `spaln -Q7 -O4 -M4 -H..` printed.  Both orientations
    (S3): a query whose printed first locus is the reverse-complemented query is held to that first locus only -- the program leaves
    the query reverse-complemented after such a locus (alignS_ng, src/fwd2s1.cc:2766-2777) and aligns its further loci in that state
    with the HSPs of the other one, where the library aligns every locus on its own (include/spdp.h, spdp_map_align_s_multi)"""
    c = Case(eng, name)
    try:
        want = c.runs[run + ("_pw" if all_out else "")]
        # the fixtures hold loci the threshold drops: -pw prints more for some queries (else this test could not tell)
        plain, pw = c.runs[run], c.runs[run + "_pw"]
        assert sum(1 for q in pw if len(pw[q]) > len(plain.get(q, []))) >= 3
        lists, _, rc = c.multi(all_out, ori)
        assert rc == 0
        got = c.as_printed(lists)
        carried = {q for q, v in want.items() if ori == 3 and v[0][2][0][0] > v[0][2][0][1]}     # (first locus: descending query positions)
        diff = [q for q in set(want) | set(got) if want.get(q) != got.get(q) and q not in carried]
        assert not diff, [(q, want.get(q), got.get(q)) for q in sorted(diff)[:3]]
        assert all(want[q][0] == got.get(q, [None])[0] and len(got[q]) <= c.prm.max_out for q in carried)
        assert len(carried) < len(want) // 2
        assert sum(len(v) for v in got.values()) > len(got)          # (several loci per query)
    finally:
        c.free()


def test_a_dropped_locus_takes_a_slot(eng):
    """blkaln orders ALL loci by fstat.val and prints the first n_out positions, n_out = the loci the threshold kept: a locus whose
    score is <= Vthr keeps its place and is printed, and a kept one behind it is not (src/spaln.cc:913-976).  The protein fixture
    (-H395) holds such a query: the program printed a record whose score is NEVSEL; the library reports the same list, that locus
    with SPDP_NEVSEL at the same place"""
    c = Case(eng, "map_multi_p1")
    try:
        thr = c.setup["H"]
        printed = {q: v for q, v in c.runs["P"].items() if min(c.z_scores["P"][q]) <= thr}
        assert printed                                                  # (the fixture holds the case, else this test could not tell)
        lists, _, rc = c.multi(False)
        assert rc == 0
        got = c.as_printed(lists)
        for q, want in printed.items():
            assert got.get(q) == want, (q, want, got.get(q))
            genes = lists[c.names.index(q)]
            assert [g["score"] == abi.NEVSEL for g in genes] == [s <= thr for s in c.z_scores["P"][q]], (q, genes)
            pw = c.runs["P_pw"][q]
            assert len(pw) > len(want) and any(x not in want for x in pw)   # (a kept locus the dropped one displaced)
    finally:
        c.free()


@pytest.mark.parametrize("name,run,ori", RUNS, ids=[r[1] for r in RUNS])
def test_one_locus_equals_the_best_only_entry(eng, name, run, ori):
    """-M1 (an index made for MaxOut 1: Ncand 11) with -pw: the locus the multi entry reports is the old entries' best one, for every
    query whose loci all aligned"""
    c = Case(eng, name, max_out=1)
    try:
        loci, _ = blocks.find(c.ix, c.gen, c.off, c.model, c.sc if not c.protein else _chain_costs(c.sc), c.prm, c.queries)
        lists, _, rc = c.multi(True, ori)
        best, _, rc2 = c.best(ori)
        assert rc == 0 and rc2 == 0
        n_same = 0
        for i, (lst, b) in enumerate(zip(lists, best)):
            if b is None:
                assert lst == [], i
                continue
            if b["n_loci"] != len(loci[i]):
                continue
            assert lst == [b], (i, lst, b)
            n_same += 1
        assert n_same >= len(c.queries) // 2
        assert any(len(v) > 1 for v in loci)                            # (MaxOut2 4: a choice to make)
    finally:
        c.free()


def _chunk_lines(stderr):
    return [ln for ln in stderr.splitlines() if ln.startswith("[map] chunk of ")]


@pytest.mark.parametrize("name,run,ori", RUNS, ids=[r[1] for r in RUNS])
def test_several_chunks_equal_one_chunk(eng, name, run, ori, monkeypatch, capfd):
    """the chunk loop of the map + align chain: a call cut into at least three chunks of loci (SPDP_MAP_CHUNK_MPOS=1: 2^20 positions
    each) reports what the same call in one chunk reports -- every locus (-pw), scores, val, n_loci and exon rows.  What can go
    wrong only beyond one chunk: slot m + k of the other strand under ori = 3, the at[] offsets, the range rng[2 (c0 + k)].  The
    `[map] chunk of` lines of SPDP_MAP_VERBOSE say how many chunks a call made.  A fixture whose loci fill fewer than three chunks
    has its queries repeated k times, k the smallest number that gives three by the positions the one-chunk call printed (queries
    are independent: every copy's lists must equal the first one's).  On these fixtures: S1 two copies, five chunks; S3 one copy,
    five chunks; P four copies, three chunks"""
    c = Case(eng, name)
    try:
        monkeypatch.setenv("SPDP_MAP_VERBOSE", "1")
        for v in ("SPDP_MAP_CHUNK_MPOS", "SPDP_MAP_CHUNK_MB"):
            monkeypatch.delenv(v, raising=False)

        def call():
            capfd.readouterr()
            lists, _, rc = c.multi(True, ori)
            assert rc == 0
            return lists, _chunk_lines(capfd.readouterr().err)

        one, lines = call()
        assert len(lines) == 1, lines
        # "... loci, %.1f M positions": at least this many (the figure is rounded to 10^5); three chunks are planned from 2 x 2^20 + 1 on
        positions = float(re.search(r"([0-9.]+) M positions", lines[0]).group(1)) * 1e6 - 5e4
        assert positions > 0, lines
        k = int((2 << 20) // positions) + 1
        n = len(c.queries)
        if k > 1:
            c.queries = c.queries * k
            one, lines = call()
            assert len(lines) == 1, lines
        monkeypatch.setenv("SPDP_MAP_CHUNK_MPOS", "1")
        cut, lines = call()
        print("copies of the queries", k, "loci per chunk", [int(ln.split()[3]) for ln in lines])
        assert len(lines) >= 3, (k, lines)
        assert cut == one, [(i, a, b) for i, (a, b) in enumerate(zip(one, cut)) if a != b][:2]
        assert sum(len(lst) for lst in one[:n]) > n                     # (several loci per query)
        for j in range(1, k):
            assert one[j * n:(j + 1) * n] == one[:n], j
    finally:
        c.free()


def _chain_costs(sch):
    """the gap and intron prices the HSP chaining of a protein search reads (as spdp_map_align_h hands them to spdp_blk_find)"""
    s = abi.Scoring()
    s.gop, s.gep, s.lgop, s.lgep, s.codonk1 = sch.gop, sch.gep, sch.lgop, sch.lgep, sch.codonk1
    s.intpen, s.intpen_len = sch.intpen, sch.intpen_len
    return s


class _Member:                                   # what blocks.BlockIndex needs of an engine
    def __init__(self, lib, ctx):
        self.lib, self.ctx = lib, ctx

    def _check(self, rc, what):
        assert rc == 0, what


def _group_call(grp, c, fn, extra, multi):
    lib = grp.lib
    lib.spdp_group_context.restype = C.c_void_p
    lib.spdp_group_context.argtypes = [C.c_void_p, C.c_int]
    n_mem = lib.spdp_group_size(grp.h)
    midx = [blocks.BlockIndex(_Member(lib, lib.spdp_group_context(grp.h, r)), c.fx) for r in range(n_mem)]
    try:
        handles = (C.c_void_p * n_mem)(*[i.h for i in midx])
        nq = len(c.queries)
        offs = np.zeros(nq + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(q) for q in c.queries])
        codes = np.ascontiguousarray(np.concatenate(c.queries))
        g = blocks.Genome()
        g.codes, g.chr_off, g.n_chr = c.gen.ctypes.data, c.off.ctypes.data, len(c.off) - 1
        rp = c.rescore if c.protein else abi.RescoreParams(*(int(x) for x in c.rescore))
        f = getattr(lib, fn)
        f.restype = C.c_int
        exons = C.POINTER(blocks.MapExon)()
        head = [grp.h, handles, C.byref(midx[0].desc), C.byref(g), C.byref(c.sc), C.byref(c.sp), C.addressof(c.sigmodel), C.byref(c.prm),
                C.byref(rp), codes.ctypes.data, offs.ctypes.data]
        f.argtypes = [C.c_void_p] * 11 + [C.c_int32] * (1 + len(extra)) + [C.c_void_p] * (3 if multi else 2)
        if multi:
            gene_off = np.zeros(nq + 1, dtype=np.int64)
            genes = C.POINTER(blocks.MapGene)()
            rc = f(*head, nq, *extra, gene_off.ctypes.data, C.byref(genes), C.byref(exons))
            assert rc == 0, lib.spdp_group_last_error(grp.h)
            idx = [list(range(int(gene_off[i]), int(gene_off[i + 1]))) for i in range(nq)]
        else:
            genes = (blocks.MapGene * nq)()
            rc = f(*head, nq, *extra, genes, C.byref(exons))
            assert rc == 0, lib.spdp_group_last_error(grp.h)
            idx = [[i] if genes[i].chr >= 0 else [] for i in range(nq)]
        out = [[dict(chr=genes[k].chr, rvs=genes[k].rvs, q_rev=genes[k].q_rev, score=genes[k].score, val=genes[k].val, n_loci=genes[k].n_loci,
                     exons=[(exons[genes[k].exon_off + j].q_left, exons[genes[k].exon_off + j].q_right, exons[genes[k].exon_off + j].g_left,
                             exons[genes[k].exon_off + j].g_right) for j in range(genes[k].n_exons)]) for k in ks] for ks in idx]
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        if multi:
            libc.free(genes)
        libc.free(exons)
        return out
    finally:
        for i in midx:
            i.free()


@pytest.mark.parametrize("members", [2, 3])
def test_group_forms_equal_one_context(eng, members):
    """groups of 2 and 3 members on one card: spdp_group_map_align_s_multi (both orientations, -pw and not),
    spdp_group_map_align_h_multi and spdp_group_map_align_h = one context's calls, in the caller's query order"""
    grp = engine.Group([0] * members)
    try:
        c = Case(eng, "map_multi_par")
        try:
            for ori, all_out in ((1, 0), (3, 1)):
                want, _, rc = c.multi(bool(all_out), ori)
                assert rc == 0
                assert _group_call(grp, c, "spdp_group_map_align_s_multi", (ori, all_out), True) == want
        finally:
            c.free()
        c = Case(eng, "map_multi_p1")
        try:
            want, _, rc = c.multi(False)
            assert rc == 0
            assert _group_call(grp, c, "spdp_group_map_align_h_multi", (0,), True) == want
            best, _, rc = c.best()
            assert rc == 0
            assert _group_call(grp, c, "spdp_group_map_align_h", (), False) == [[b] if b is not None else [] for b in best]
        finally:
            c.free()
    finally:
        grp.close()


def test_refusals(eng):
    """an index made for another MaxOut (its ncand != max_out + 10), max_out < 1 and max_out2 < max_out: an error with a message"""
    c = Case(eng, "map_multi_par")
    try:
        bad = blocks.BlkFindParams.from_buffer_copy(c.prm)
        bad.max_out = bad.max_out2 = 1
        with pytest.raises(RuntimeError, match="another MaxOut"):
            c.multi(False, prm=bad)
        bad.max_out = 0
        with pytest.raises(RuntimeError, match="max_out must be"):
            c.multi(False, prm=bad)
        bad.max_out, bad.max_out2 = 4, 3
        with pytest.raises(RuntimeError, match="max_out must be"):
            c.multi(False, prm=bad)
        with pytest.raises(RuntimeError, match="max_out must be"):       # (the protein entry checks the same before anything else)
            blocks.map_align_h_multi(c.ix, c.gen, c.off, abi.ScoringH(), c.sp, abi.SignalModelH(), bad, abi.RescoreParamsH(), c.queries[:2])
    finally:
        c.free()


N8 = [("cdna", ["--ori", "1"]), ("cdna_ori3", ["--ori", "3"]), ("protein", ["--protein"])]


@pytest.mark.parametrize("kind,flags", N8, ids=[k for k, _ in N8])
def test_tool_against_the_live_program(kind, flags):
    """tools/e2e_q7.py --paralogs --max-out 4 at 300-400 queries: every query's ordered locus list and exon tables = `spaln -M4`'s"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "spaln")):
        pytest.skip("oracle/_ref/spaln is not built")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e_q7.py"), "--paralogs", "--max-out", "4", "--queries", "320",
                        "--genes", "60"] + flags, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-600:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["max_out"] == 4 and d["reference_loci"] > d["reference_aligned"]
    assert d["reference_aligned"] == d["library_aligned"] == d["identical_first_loci"], (d, r.stderr[-600:])
    if kind == "cdna_ori3":                 # (see test_locus_lists_equal_the_recorded_program)
        assert d["identical_lists_of_the_others"] == d["reference_aligned"] - d["reversed_first"] and d["reversed_first"] < d["reference_aligned"], d
    else:
        assert d["identical_locus_lists"] == d["reference_aligned"], (d, r.stderr[-600:])


def test_vote_index_for_max_out_8(eng):
    """-M8: the index's queues sized for Ncand 18 fit the vote's LDS; the lists hold up to 8 loci"""
    c = Case(eng, "map_multi_par", max_out=8)
    try:
        assert int(c.ix.desc.ncand) == 18
        lists, _, rc = c.multi(True)
        assert rc == 0 and max(len(v) for v in lists) <= 8 and sum(len(v) for v in lists) >= len(c.queries)
    finally:
        c.free()
