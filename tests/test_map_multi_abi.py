"""CPU checks of the map + align entries that report several loci per query (`spaln -M N`): the five new entries are exported by
the library and declared in include/spdp.h with the argument lists the Python side passes, and the layouts those lists hand back
(SpdpMapGene, SpdpMapExon) match the header."""
import ctypes as C
import os
import re
import subprocess

from spaln_amd import blocks, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("spdp_map_align_s_multi", "spdp_map_align_h_multi", "spdp_group_map_align_s_multi", "spdp_group_map_align_h_multi",
       "spdp_group_map_align_h")


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "spdp.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", txt)
    assert m, name
    return [a.strip() for a in " ".join(m.group(1).split()).split(",")]


def test_new_entries_are_exported_and_declared():
    lib = C.CDLL(engine.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        _declaration(name)


def test_multi_argument_lists():
    """the inputs of today's entries, then all_out, then gene_off[n + 1] and the two malloc'ed arrays (+ seconds on one context)"""
    for name, base, group in (("spdp_map_align_s_multi", "spdp_map_align_s", False), ("spdp_map_align_h_multi", "spdp_map_align_h", False),
                              ("spdp_group_map_align_s_multi", "spdp_group_map_align_s", True),
                              ("spdp_group_map_align_h_multi", "spdp_group_map_align_h", True)):
        new, old = _declaration(name), _declaration(base)
        n_in = len(old) - (2 if group else 3)                            # (genes, exons[, seconds])
        assert new[:n_in] == old[:n_in], name
        assert new[n_in] == "int32_t all_out", name
        assert new[n_in + 1:n_in + 4] == ["int64_t* gene_off", "SpdpMapGene** genes", "SpdpMapExon** exons"], name
        assert new[n_in + 4:] == ([] if group else ["double* seconds"]), name
    h, s = _declaration("spdp_group_map_align_h"), _declaration("spdp_group_map_align_s")
    assert h[0] == s[0] and h[-2:] == s[-2:] and "int32_t ori" not in h


def test_map_records_match_the_header(tmp_path):
    """the new entries add no record of their own: they hand back the existing SpdpMapGene / SpdpMapExon and read SpdpBlkFindParams;
    their ctypes mirrors, which the multi wrappers index by offset, still match the header"""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spdp.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(SpdpMapGene), sizeof(SpdpMapExon), offsetof(SpdpMapGene, val),'
                   'offsetof(SpdpMapGene, n_exons), offsetof(SpdpMapGene, exon_off), offsetof(SpdpMapExon, g_right), sizeof(SpdpBlkFindParams));'
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(blocks.MapGene), C.sizeof(blocks.MapExon), blocks.MapGene.val.offset, blocks.MapGene.n_exons.offset,
                   blocks.MapGene.exon_off.offset, blocks.MapExon.g_right.offset, C.sizeof(blocks.BlkFindParams)]


def test_python_entries_exist():
    assert callable(blocks.map_align_multi) and callable(blocks.map_align_h_multi)
