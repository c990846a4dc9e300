"""The seeded entry of the unspliced aligner without a GPU: its symbols are declared, exported and bound, the structs it reads
have the layouts the bindings say, the protein-pair HSP model is the recorded one, and every bundle it does not serve is refused
with a message that names the field (spdp_align_b_seeded_refusal: the check the entry makes before it touches the device)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from spaln_amd import abi, defaults, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spdp_align_b_seeded", "spdp_seeded_stats_b", "spdp_align_b_seeded_refusal"]


def test_symbols_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "spdp.h")).read()
    declared = set(re.findall(r"\b(spdp_[a-z_0-9]+)\s*\(", txt))
    lib = C.CDLL(engine.LIB_PATH)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in engine.EXPORTS and s in exported, s
    assert hasattr(engine.Engine, "align_b_seeded") and hasattr(engine.Engine, "seeded_stats_b")


def test_struct_sizes_match_the_bindings(tmp_path):
    names = [("SpdpSeedParams", abi.SeedParams), ("SpdpWilipModel", abi.WilipModel), ("SpdpWilipLevel", abi.WilipLevel),
             ("SpdpScoring", abi.Scoring), ("SpdpProblem", abi.Problem), ("SpdpUnsplicedParams", abi.UnsplicedParams),
             ("SpdpJuxt", abi.Juxt), ("SpdpHspSource", abi.HspSource), ("SpdpAlignment", abi.Alignment)]
    offs = [("SpdpSeedParams", "wilip", abi.SeedParams.wilip.offset), ("SpdpSeedParams", "lcl", abi.SeedParams.lcl.offset),
            ("SpdpSeedParams", "vthr", abi.SeedParams.vthr.offset), ("SpdpWilipModel", "dvsp", abi.WilipModel.dvsp.offset),
            ("SpdpWilipModel", "lsg", abi.WilipModel.lsg.offset), ("SpdpWilipModel", "ser2", abi.WilipModel.ser2.offset)]
    body = "".join(f'printf("%zu\\n", sizeof({n}));' for n, _ in names) + "".join(f'printf("%zu\\n", offsetof({n}, {f}));' for n, f, _ in offs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spdp.h"\nint main(){' + body + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(t) for _, t in names] + [o for _, _, o in offs]


def test_wilip_model_b_is_the_recorded_one():
    with open(os.path.join(ROOT, "tests", "golden", "b_aa_wilip.json")) as f:
        doc = json.load(f)
    assert "source" in doc and "src/wln.cc" in doc["source"]
    m = defaults.wilip_model_b()
    assert (m.dvsp, m.lsg) == (3, 0) == (doc["dvsp"], doc["lsg"])
    for k in ("end_bonus", "crs", "mlt", "shortquery", "min_hit", "met", "ser", "ser2", "mtx_rows", "mtx_cols"):
        assert getattr(m, k) == doc[k], k
    for i, lv in enumerate(doc["levels"]):
        L = m.level[i]
        for k in ("elem", "tpl", "mask", "width", "gain", "gain1", "thr", "xdrp", "cutoff", "vthr"):
            assert getattr(L, k) == lv[k], (i, k)
        assert L.bitpat_len == len(lv["bitpat"]) and list(L.bitpat)[:L.bitpat_len] == lv["bitpat"]
        assert list(L.convtab)[:len(lv["convtab"])] == [min(255, c) for c in lv["convtab"]]
        assert L.mask == L.elem ** L.tpl and sum(lv["bitpat"]) == L.tpl and len(lv["bitpat"]) == L.width
    assert np.array_equal(np.asarray([m.mtx[k] for k in range(m.mtx_rows * m.mtx_cols)]).reshape(m.mtx_rows, m.mtx_cols), np.asarray(doc["mtx"]))
    # the search matrix is symmetric over the twenty residues, and a residue scores best against itself
    code = np.asarray([c for c in range(m.mtx_rows) if c in set(defaults.matrix_b().nonzero()[0])])
    sub = np.asarray(doc["mtx"])[np.ix_(code, code)]
    assert code.size == 20 and np.array_equal(sub, sub.T) and np.all(sub.argmax(axis=1) == np.arange(20))
    sp = defaults.seed_params_b(3, 15)
    assert (sp.qck, sp.vthr, sp.lcl, list(sp.wl_width)) == (3, doc["vthr"], 15, doc["wl_width"]) and doc["vthr"] == defaults.B_THR


def _refusal(lib, sc, up, sp, model, hsps_for_all=0, has_src=0):
    sp.wilip = C.addressof(model) if model is not None else None
    r = lib.spdp_align_b_seeded_refusal(C.byref(sc), C.byref(up), C.byref(sp), hsps_for_all, has_src)
    sp.wilip = None
    return r.decode() if r else None


def test_what_is_not_served_is_refused_by_name():
    lib = engine.load_library()
    sc, up, model = defaults.scoring_b(), abi.UnsplicedParams(1.0, 0), defaults.wilip_model_b()
    assert _refusal(lib, sc, up, defaults.seed_params_b(3), model) is None
    assert _refusal(lib, sc, up, defaults.seed_params_b(1), None, hsps_for_all=1) is None
    assert _refusal(lib, sc, up, defaults.seed_params_b(1), None, has_src=1) is None
    assert _refusal(lib, defaults.scoring_b(local=1), up, defaults.seed_params_b(3, 16), model) is None

    def named(field, why):
        assert why is not None and field in why, (field, why)

    for q in (0, 4, -1):
        named("SpdpSeedParams.qck", _refusal(lib, sc, up, defaults.seed_params_b(q), model))
    named("SpdpSeedParams.wilip", _refusal(lib, sc, up, defaults.seed_params_b(3), None, hsps_for_all=1))      # the levels' tuple sizes
    named("SpdpSeedParams.wilip", _refusal(lib, sc, up, defaults.seed_params_b(1), None))                      # nobody to search
    sp = defaults.seed_params_b(3)
    sp.vthr = -1
    named("SpdpSeedParams.vthr", _refusal(lib, sc, up, sp, model))
    sp = defaults.seed_params_b(3)
    sp.wl_width[1] = -2
    named("SpdpSeedParams.wl_width", _refusal(lib, sc, up, sp, model))
    named("SpdpSeedParams.lcl", _refusal(lib, sc, up, defaults.seed_params_b(3, 15 | 32), model))            # LocalC: not part of Aln2b1
    named("SpdpSeedParams.lcl", _refusal(lib, sc, up, defaults.seed_params_b(3, 16), model))                 # local here, global there
    named("SpdpSeedParams.lcl", _refusal(lib, defaults.scoring_b(local=1), up, defaults.seed_params_b(3, 15), model))
    for field, value in (("dvsp", 1), ("dvsp", 0), ("lsg", 1), ("mtx_rows", 40), ("mtx_cols", 0)):
        bad = defaults.wilip_model_b()
        setattr(bad, field, value)
        named("wilip->" + field, _refusal(lib, sc, up, defaults.seed_params_b(3), bad))
    bad = defaults.wilip_model_b()
    bad.level[2].tpl = 0
    named("wilip->level", _refusal(lib, sc, up, defaults.seed_params_b(3), bad))
    bad = defaults.wilip_model_b()
    bad.level[0].bitpat_len = 33
    named("bitpat_len", _refusal(lib, sc, up, defaults.seed_params_b(3), bad))
    # the scoring bundle and the unspliced parameters: as spdp_align_b refuses them
    named("SpdpScoring.spj", _refusal(lib, defaults.scoring_b(spj=1), up, defaults.seed_params_b(3), model))
    named("SpdpScoring.scalar_engines", _refusal(lib, defaults.scoring_b(scalar_engines=0), up, defaults.seed_params_b(3), model))
    named("SpdpUnsplicedParams.max_trace_bytes", _refusal(lib, sc, abi.UnsplicedParams(1.0, -1), defaults.seed_params_b(3), model))
