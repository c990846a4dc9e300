"""The unspliced aligner's C ABI without a GPU: the symbols are exported and declared, the bindings match the C layouts, and
the host-side entries refuse what the header says they refuse (and serve what they can: rescoring needs no device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spaln_amd import abi, defaults, engine
from tests import unspliced_cases as uc
from tests import unspliced_ref as ubr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spdp_align_b", "spdp_homscore_b", "spdp_skl_rng_b", "spdp_skl_edits_b", "spdp_cells_b", "spdp_trace_bytes_b", "spdp_lsp_b"]


def test_symbols_are_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "spdp.h")).read()
    declared = set(re.findall(r"\b(spdp_[a-z_0-9]+)\s*\(", txt))
    lib = C.CDLL(engine.LIB_PATH)
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in engine.EXPORTS, s
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].endswith("_b")}
    assert set(NEW) <= exported


def test_struct_sizes_match_the_bindings(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spdp.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(SpdpUnsplicedParams), offsetof(SpdpUnsplicedParams, max_trace_bytes),'
                   'sizeof(SpdpRescoredB), offsetof(SpdpRescoredB, span), sizeof(SpdpScoring));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.UnsplicedParams), abi.UnsplicedParams.max_trace_bytes.offset, C.sizeof(abi.RescoredB),
                   abi.RescoredB.span.offset, C.sizeof(abi.Scoring)]


def _one_alignment():
    sc, up, ps, recs = uc.problems("shapes1", 0)
    skls = [ubr.align(sc, up, p)[1] for p in ps.items]
    return sc, up, ps, recs, skls


def _rng(lib, sc, up, ps, skls):
    n = len(ps)
    keep = [np.ascontiguousarray(s, dtype=np.int32) for s in skls]
    arr = (abi.Alignment * n)()
    for i, s in enumerate(keep):
        arr[i].n_skl = s.shape[0]
        arr[i].skl = C.cast(s.ctypes.data, C.POINTER(abi.Skl))
    out = (abi.RescoredB * n)()
    return lib.spdp_skl_rng_b(C.byref(sc), C.byref(up), ps.array(), n, arr, out), out


def test_spj_and_engine_flavour_are_refused():
    lib = engine.load_library()
    sc, up, ps, recs, skls = _one_alignment()
    assert _rng(lib, sc, up, ps, skls)[0] == 0
    for field, value in (("spj", 1), ("scalar_engines", 0), ("scalar_engines", 2), ("noll", 4)):
        bad = defaults.scoring_b(**{field: value}) if field != "noll" else defaults.scoring_b()
        if field == "noll":
            bad.noll = value
        assert _rng(lib, bad, up, ps, skls)[0] == -1, field
    assert _rng(lib, sc, abi.UnsplicedParams(1.0, -1), ps, skls)[0] == -1


def test_host_rescoring_gives_the_programs_statistics():
    """spdp_skl_rng_b / spdp_skl_edits_b need no device: on the restatement's corner lists they print what the program printed"""
    lib = engine.load_library()
    for name, k in (("shapes1", 0), ("shapes2", 5), ("mid", 3), ("tgapf", 0), ("local", 1)):
        sc, up, ps, recs = uc.problems(name, k)
        skls = [ubr.align(sc, up, p)[1] for p in ps.items]
        rc, out = _rng(lib, sc, up, ps, skls)
        assert rc == 0
        for i, rec in enumerate(recs):
            st = {f: getattr(out[i], f) for f, _ in abi.RescoredB._fields_}
            uc.check_record(st, skls[i][st["first"]:st["first"] + st["n_trim"]], rec, (name, k, i))
            want = ubr.rescore(sc, up, ps.items[i], skls[i])[0]
            assert {f: st[f] for f in want} == want


def test_cells_and_trace_bytes():
    lib = engine.load_library()
    sc, up, ps, _ = uc.problems("mid", 0)
    for p in ps.items:
        w = ubr.stripe(p, sc.sh)
        assert int(lib.spdp_cells_b(C.byref(p), C.byref(w))) == ubr.cells(p, sc.sh)
        rows, cols = p.a_right - p.a_left, p.b_right - p.b_left
        tb = int(lib.spdp_trace_bytes_b(C.byref(p), C.byref(w)))
        assert ubr.cells(p, sc.sh) <= tb <= (rows + 64) * (cols + 67)      # one byte per cell and the fill of whole tiles


def test_host_edit_records_give_the_programs_cigar():
    lib = engine.load_library()
    for name, k in (("shapes1", 1), ("mid", 0), ("local", 0)):
        sc, up, ps, recs = uc.problems(name, k)
        n = len(ps)
        keep = [np.ascontiguousarray(ubr.align(sc, up, p)[1], dtype=np.int32) for p in ps.items]
        arr = (abi.Alignment * n)()
        for i, s in enumerate(keep):
            arr[i].n_skl = s.shape[0]
            arr[i].skl = C.cast(s.ctypes.data, C.POINTER(abi.Skl))
        for fmt in (abi.FMT_CIGAR, abi.FMT_VULGAR, abi.FMT_SAM):
            out = (abi.Edits * n)()
            assert lib.spdp_skl_edits_b(C.byref(sc), C.byref(up), ps.array(), n, arr, fmt, out) == 0
            for i, rec in enumerate(recs):
                got = [[out[i].rec[j].op, out[i].rec[j].alen, out[i].rec[j].blen] for j in range(out[i].n)]
                _, _, want, sam = ubr.rescore(sc, up, ps.items[i], keep[i], fmt)
                assert got == want.tolist(), (name, k, i, fmt)
                if fmt == abi.FMT_CIGAR:
                    assert [[chr(o), l] for o, l, _ in got] == (rec["cigar"] or [])      # (no Cigar line for an alignment without a leg)
                if fmt == abi.FMT_SAM:
                    assert [out[i].sam_flag, out[i].sam_pos, out[i].sam_mapq, out[i].sam_left, out[i].sam_right] == sam
            lib.spdp_free_edits(out, n)
        assert lib.spdp_skl_edits_b(C.byref(sc), C.byref(up), ps.array(), n, arr, 7, (abi.Edits * n)()) == -1


def test_lsp_b_without_a_context_is_refused():
    """spdp_lsp_b takes spdp_align_b's arguments and a counter array; without a context (no device) it refuses like
    spdp_align_b, before it reads anything else or writes the counters"""
    lib = engine.load_library()
    sc, up, ps, _ = uc.problems("shapes1", 0)
    n = len(ps)
    out = (abi.Alignment * n)()
    stats = (C.c_int64 * 8)(*([7] * 8))
    assert lib.spdp_lsp_b(None, C.byref(sc), C.byref(up), ps.array(), n, out, stats) == -1
    assert lib.spdp_align_b(None, C.byref(sc), C.byref(up), ps.array(), n, out) == -1
    assert list(stats) == [7] * 8 and all(out[i].n_skl == 0 and not out[i].skl for i in range(n))
    assert lib.spdp_lsp_b(None, None, None, None, 0, None, None) == -1
    # the refusals that carry a message name the fields spdp_align_b names (tests/test_gpu_thin_sweep.py reads them on a device);
    # both go through the same two functions
    src = open(os.path.join(ROOT, "spaln_amd", "csrc", "spdp_b_api.cpp")).read()
    body = src[src.index('extern "C" int spdp_lsp_b('):src.index('extern "C" int spdp_homscore_b(')]
    assert "refused(sc, up)" in body and "bad_problem(*sc, probs[i])" in body
