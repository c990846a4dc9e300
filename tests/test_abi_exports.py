"""CPU-side checks of the drop-in boundary: the shared library loads and exports
every symbol include/spdp.h declares; the ctypes mirrors match the C layouts."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from spaln_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "spdp.h")).read()
    return sorted(set(re.findall(r"\b(spdp_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_all_declared_symbols():
    lib = C.CDLL(engine.LIB_PATH)
    missing = [s for s in _declared() if not hasattr(lib, s)]
    assert not missing, missing
    assert set(engine.EXPORTS) <= set(_declared())
    # the read-back of the column records (tests/test_gpu_signal_cases.py): declared, exported, wrapped
    for name in ("spdp_signal_records_s", "spdp_signal_records_h"):
        assert name in _declared() and name in engine.EXPORTS and hasattr(lib, name)
    assert hasattr(engine.Engine, "signal_records_s") and hasattr(engine.Engine, "signal_records_h")
    # the HSP search's request path and the block search's counters (tests/test_hsp_cases.py, tests/test_gpu_hsp_cases.py)
    from spaln_amd import blocks
    for name, wrapper in (("spdp_hsp_plan", "hsp_plan"), ("spdp_hsp_tasks", "hsp_tasks"), ("spdp_hsp_tasks_host", "hsp_tasks_host"), ("spdp_blk_find_stats", "find_stats"),
                          ("spdp_blk_vote_stats", "vote_stats")):
        assert name in _declared() and name in engine.EXPORTS and hasattr(lib, name) and hasattr(blocks, wrapper)


def test_hsp_entries_refuse_null_arguments():
    """without a device: the device entry and the counters can only refuse, the host entries say why"""
    lib = engine.load_library()
    assert lib.spdp_hsp_tasks(None, None, None, None, None, None, None) == -1
    assert lib.spdp_blk_find_stats(None, None, 0) == -1
    assert lib.spdp_blk_vote_stats(None, None, None, 0) == -1
    # the binding names as many fields as the header declares
    n = int(re.search(r"#define SPDP_BLK_VOTE_STATS_N (\d+)", open(os.path.join(ROOT, "include", "spdp.h")).read()).group(1))
    assert len(abi.BLK_VOTE_STATS) == n == len(set(abi.BLK_VOTE_STATS))
    err = C.create_string_buffer(128)
    assert lib.spdp_hsp_tasks_host(None, None, None, None, err, 128) == -1 and b"null argument" in err.value
    assert lib.spdp_hsp_plan(None, 1, 17, 17, 1, 1, None, err, 128) == -1 and b"null argument" in err.value


def test_signal_records_refuse_a_null_context():
    """without a device the two entries can only refuse: -1, nothing touched"""
    lib = engine.load_library()
    assert lib.spdp_signal_records_s(None, None, None, 0, None, 0, None, None, None) == -1
    assert lib.spdp_signal_records_h(None, None, None, 0, None, 0, None, None) == -1


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spdp.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(SpdpScoring), sizeof(SpdpProblem),'
                   'offsetof(SpdpScoring, gop), offsetof(SpdpScoring, qm_len), offsetof(SpdpProblem, a_left),'
                   'sizeof(SpdpAlignment));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.Scoring), C.sizeof(abi.Problem), abi.Scoring.gop.offset,
            abi.Scoring.qm_len.offset, abi.Problem.a_left.offset, C.sizeof(abi.Alignment)]
    assert got == want


def test_no_gpu_means_loud_failure():
    # torch is asked in a child process: its wheel carries a HIP runtime of its own, and loaded here after the library it
    # would start a second runtime in this process, which takes the device from the library's for every later test
    probe = subprocess.run([sys.executable, "-c", "import torch; print(int(torch.cuda.is_available()))"],
                           capture_output=True, text=True, check=True)
    if probe.stdout.split()[-1] == "1":
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        engine.Engine(0)
