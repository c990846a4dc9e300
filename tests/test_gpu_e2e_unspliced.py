"""Protein pairs end to end against the live program: tools/b_pairs.py as a child process (its own context, its own timing)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "spaln")


def test_300_pairs_equal_the_programs_records():
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/spaln is not built (the reference's source tree is not on this machine)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "b_pairs.py"), "--pairs", "300", "--threads", "16"],
                       capture_output=True, text=True, cwd=ROOT, timeout=240)
    assert r.stdout.strip(), r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    print(line)
    assert line["pairs"] == 300 and line["identical"] == 300, line
    assert r.returncode == 0
