"""Default scoring bundle of the cDNA x genome path, as the reference CLI sets it up
(setdefparam, src/spaln.cc:1471-1494; PwdB, src/aln2.cc:99-137; IntronPenalty,
src/codepot.cc:126-233 with the generic table/ parameter set).  These are DATA
read back from a reference run (the same values every tests/golden/*.spdg
fixture carries in its `params`, `mtx`, `qm_*` records), not code.
"""
import numpy as np

from . import abi

# residue codes of the reference's nucleotide alphabet (src/cmn.h:114): A=2 C=3 G=5 T=9, N=16
CODE_OF = {ord("A"): 2, ord("C"): 3, ord("G"): 5, ord("T"): 9, ord("N"): 16}
NSIMD = 17

# Simmtx::Nmtx for setNpam(4, -6), alprm.scale = 10: match +20, mismatch -60, gap column -20
NMTX = np.array([
    [   0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0],
    [   0,    0,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20,  -20],
    [   0,  -20,   20,  -60,    0,  -60,    0,  -60,  -30,  -60,    0,  -60,  -30,  -60,  -30,  -60,  -30],
    [   0,  -20,  -60,   20,    0,  -60,  -60,    0,  -30,  -60,  -60,    0,  -30,  -60,  -60,  -30,  -30],
    [   0,  -20,    0,    0,    0,  -60,  -30,  -30,  -30,  -60,  -30,  -30,  -30,  -60,  -60,  -60,  -30],
    [   0,  -20,  -60,  -60,  -60,   20,    0,    0,  -30,  -60,  -60,  -60,  -60,    0,  -30,  -30,  -30],
    [   0,  -20,    0,  -60,  -30,    0,    0,  -30,  -30,  -60,  -30,  -60,  -60,  -30,  -30,  -60,  -30],
    [   0,  -20,  -60,    0,  -30,    0,  -30,    0,  -30,  -60,  -60,  -30,  -60,  -30,  -60,  -30,  -30],
    [   0,  -20,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -60,  -60,  -60,  -30,  -60,  -30,  -30,  -30],
    [   0,  -20,  -60,  -60,  -60,  -60,  -60,  -60,  -60,   20,    0,    0,  -30,    0,  -30,  -30,  -30],
    [   0,  -20,    0,  -60,  -30,  -60,  -30,  -60,  -60,    0,    0,  -30,  -30,  -30,  -30,  -60,  -30],
    [   0,  -20,  -60,    0,  -30,  -60,  -60,  -30,  -60,    0,  -30,    0,  -30,  -30,  -60,  -30,  -30],
    [   0,  -20,  -30,  -30,  -30,  -60,  -60,  -60,  -30,  -30,  -30,  -30,  -30,  -60,  -30,  -30,  -30],
    [   0,  -20,  -60,  -60,  -60,    0,  -30,  -30,  -60,    0,  -30,  -30,  -60,    0,  -30,  -30,  -30],
    [   0,  -20,  -30,  -60,  -60,  -30,  -30,  -60,  -30,  -30,  -30,  -60,  -30,  -30,  -30,  -30,  -30],
    [   0,  -20,  -60,  -30,  -60,  -30,  -60,  -30,  -30,  -30,  -60,  -30,  -30,  -30,  -30,  -30,  -30],
    [   0,  -20,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30,  -30]
], dtype=np.int32)

GOP, GEP = -60, -20              # PwdB::BasicGOP / BasicGEP  (v = 6, u = 2, Vab = 10)
LGOP, LGEP = -158, -6
LLMT = 20                       # IntronPrm.llmt
IPEN = -245                     # IntronPenalty::Penalty() = GapWI
QM_LEN = [73, 136, 317, 959, 1523]    # IntronPenalty::qm[].len (5 equi-probable quantiles)
QM_PEN = [-230, -229, -251, -273, -323]
SH = 100                        # alprm.sh band shoulder
MAX_VMF_SPACE = 32 * 1024 * 1024


def exact_tables():
    """IntPen(length) of the default intron-length distribution, materialised up to 29 450 nt (longer introns
    price like the last entry), and the junction table behind Exinon::sig53(.., IE53): both read back from a
    reference run (the c5_6kb fixture).  What SpdpScoring.intpen / t53 carry for the -A0 / -A1 engines."""
    import os
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "exact_tables.npz"))
    return t["intpen"], t["t53"]


def scoring(nquant=None, **over) -> abi.Scoring:
    kw = dict(mtx=NMTX, mtx_dim=NSIMD, gop=GOP, gep=GEP, lgop=LGOP, lgep=LGEP, noll=2, spj=1,
              llmt=LLMT, ipen=IPEN, qm_len=QM_LEN, qm_pen=QM_PEN, nquant=nquant, local=0, sh=SH,
              max_vmf_space=MAX_VMF_SPACE, ubh=0)
    kw.update(over)
    return abi.make_scoring(**kw)


def encode(seq_ascii: np.ndarray) -> np.ndarray:
    """ASCII nucleotides -> reference residue codes."""
    lut = np.full(256, 16, dtype=np.uint8)
    for k, v in CODE_OF.items():
        lut[k] = v
        lut[k + 32] = v
    return lut[np.asarray(seq_ascii, dtype=np.uint8)]


# ---- aa x genome path (protein query vs genomic DNA): PwdB set-up for DvsP = 1 -------------------
# values read back from a reference run (tests/golden/h1_*.spdg carry the same numbers); the
# 23 x 26 amino-acid x tron matrix (Simmtx of mdm_mtx, PAM level 150) is data/aa_tron_mtx.npy
H_GOP, H_GEP, H_LGEP = -90, -20, -6
H_CODONK1 = 1610612733                      # effectively "never": GapExtPen3 = BasicGEP
H_GAPW1, H_GAPW2, H_GAPW3 = -410, -430, -110
H_IPEN = -401
H_QM_PEN = [-367, -370, -413, -456, -557]


def scoring_h(nquant=None, **over) -> abi.ScoringH:
    import os
    mtx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "aa_tron_mtx.npy"))
    kw = dict(mtx=mtx.astype(np.int32), mtx_rows=mtx.shape[0], mtx_cols=mtx.shape[1], gop=H_GOP, gep=H_GEP,
              lgep=H_LGEP, codonk1=H_CODONK1, gapw1=H_GAPW1, gapw2=H_GAPW2, gapw3=H_GAPW3, spj=1,
              llmt=LLMT, ipen=H_IPEN, qm_len=QM_LEN, qm_pen=H_QM_PEN, nquant=nquant, local=0,
              term_codon=1, sh=SH, max_vmf_space=MAX_VMF_SPACE, ubh=0)
    kw.update(over)
    return abi.make_scoring_h(**kw)


# ---- protein x protein (the unspliced aligner, Aln2b1): PwdB set-up for DvsP = 3 ------------------------------------
# What `spaln -Q0` applies to two protein files by default: u = 2, v = 9, u1 = 0.6, k1 = 7 (-yl3 only), thr = 35, scores
# scaled by 10, band shoulder 100.  The substitution matrix and the gap terms were read off the program's printed scores
# (tests/golden/make_b_goldens.py: all 1 x 1 pairs; pairs that differ by one block) and are kept with the other recorded
# outputs, in tests/golden/b_aa_params.json; tests/test_unspliced_ref.py proves them with the rescoring identity.
B_GOP, B_GEP, B_LGOP, B_LGEP, B_K1 = -90, -20, -188, -6, 7
B_THR, B_SCALE, B_DIM = 350, 10, 23


def matrix_b() -> np.ndarray:
    """23 x 23 by the reference's amino-acid codes (A = 3 .. V = 22, synth.encode_protein); other codes score 0"""
    import json
    import os
    from . import synth
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "b_aa_params.json")
    with open(path) as f:
        doc = json.load(f)
    assert (doc["gop"], doc["gep"], doc["lgop"], doc["lgep"], doc["k1"], doc["scale"]) == (B_GOP, B_GEP, B_LGOP, B_LGEP, B_K1, B_SCALE)
    code = synth.encode_protein(np.frombuffer(doc["alphabet"].encode(), dtype=np.uint8))
    mtx = np.zeros((B_DIM, B_DIM), dtype=np.int32)
    mtx[np.ix_(code, code)] = np.asarray(doc["mtx"], dtype=np.int32)
    return mtx


def scoring_b(noll=2, local=0, sh=SH, **over) -> abi.Scoring:
    """the bundle of spdp_align_b / spdp_homscore_b for protein pairs (noll = 3: -yl3; local = 1: -LS)"""
    kw = dict(mtx=matrix_b(), mtx_dim=B_DIM, gop=B_GOP, gep=B_GEP, lgop=B_LGOP, lgep=B_LGEP, noll=noll, spj=0, local=local, sh=sh,
              scalar_engines=1, codonk1=B_K1)
    kw.update(over)
    return abi.make_scoring(**kw)


def _wilip_doc_b() -> dict:
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "b_aa_wilip.json")
    with open(path) as f:
        return json.load(f)


def wilip_model_b() -> abi.WilipModel:
    """the HSP-search model of protein pairs (DvsP = 3: the aaprm word parameters, getSimmtx(WlnPamNo) by amino-acid code,
    EndBonus, crs / lsg / mlt) as the program sets it up for two protein files, recorded in tests/golden/b_aa_wilip.json"""
    doc = _wilip_doc_b()
    m = abi.WilipModel()
    for i, lv in enumerate(doc["levels"]):
        L = m.level[i]
        for k in ("elem", "tpl", "mask", "width", "gain", "gain1", "thr", "xdrp", "cutoff", "vthr"):
            setattr(L, k, int(lv[k]))
        L.bitpat_len = len(lv["bitpat"])
        for k, v in enumerate(lv["bitpat"]):
            L.bitpat[k] = int(v)
        for c in range(32):
            L.convtab[c] = min(255, int(lv["convtab"][c])) if c < len(lv["convtab"]) else 127
    m.mtx_rows, m.mtx_cols = int(doc["mtx_rows"]), int(doc["mtx_cols"])
    for k, v in enumerate(np.asarray(doc["mtx"], dtype=np.int32).ravel()):
        m.mtx[k] = int(v)
    for k in ("dvsp", "end_bonus", "crs", "lsg", "mlt", "shortquery", "min_hit", "met", "ser", "ser2"):
        setattr(m, k, int(doc[k]))
    return m


def seed_params_b(qck: int, lcl: int = 15) -> abi.SeedParams:
    """SpdpSeedParams of spdp_align_b_seeded for `spaln -Q<qck> -L<lcl>` on protein pairs: what the entry reads (qck, the levels'
    word widths, PwdB::Vthr, algmode.lcl); the model goes in with the call (Engine.align_b_seeded)"""
    doc = _wilip_doc_b()
    sp = abi.SeedParams()
    sp.qck = int(qck)
    for k in range(4):
        sp.wl_width[k] = int(doc["wl_width"][k])
    sp.vthr = int(doc["vthr"])
    sp.lcl = int(lcl)
    sp.crs = int(doc["crs"])
    return sp


# MakeBlk::prepacomp's per-class terms of the translated block index's word scores (src/blksrc.cc:844-877) for the reference's defaults
# (twenty classes, -Xp20, -Xq1, its mdm tables) -- recorded from the compiled reference (`spaln_idxtap -W -KP`, oracle/ref_build/idx_tap.cc:
# the "[idx_tap] acomp" line, exact hex floats); spdp_blk_index_build_p's acomp
BLOCK_ACOMP_20 = [float.fromhex(x) for x in (
    "-0x1.905a039bd2496p+2 -0x1.20cd81c8d9c8p+1 -0x1.ea713dcbdeac6p+2 -0x1.d7828e58105d8p+0 0x1.018bdf0832daep+3 "
    "0x1.9dac9b7222838p+0 -0x1.2fef0207cbap+1 0x1.44fd3d196c1cfp+3 -0x1.4611967298f91p+2 -0x1.7045848bd36fcp+2 "
    "0x1.157df2a1998dep+2 0x1.b29309c2da184p-3 -0x1.9e5b95c02c5ccp+1 0x1.aeb2e0dfc9daep+2 0x1.8ffa6b1bb2d76p+1 "
    "-0x1.785b7311540c6p+3 -0x1.f7373e897ef4ap+2 0x1.7b75b1ad70547p+3 0x1.3672571d50d5bp+3 -0x1.ae4b8287ac8dp+0").split()]


# ---- the block search of a protein database (`spaln -Q7 -a<db>`: SrchBlk::finds) ------------------------------------------------
# SrchBlk::initialize with gnmdb = false (src/blksrc.cc:2179-2226): Randbs takes its square-root form, and -- algmode.crs being set
# unless -yX0 -- the cross-species constants RbsFactSqrX = 0 and RbsBaseX = 0.5 (:65-67, 2053-2057); with -yX0 RbsFactSqr =
# 0.303 x 2 and RbsBase = 3
def search_opts_protein_db(max_out: int = 1, local: int = 0, cross_species: bool = True) -> dict:
    """the fields of SpdpBlkSearchOpts to read a <db>.bka with (blocks.read_index_file(lib, path, **opts))"""
    return dict(max_out=int(max_out), local=int(local), genomic_db=0, max_mmc=15,
                rbs_fact=0.0 if cross_species else float(np.float32(0.303 * 2)), rbs_base=0.5 if cross_species else 3.0)
