"""Every request of tests/thin_cases.py through the host emulation of the two sweeps: tests/b_thin_host_check.cpp (a program with
its own main: lsp_without_cells, forward_terms, the thin or the tiled emulation of tests/b_sweep_host.h with the product's
thin_step_b / thin_geo_b / thin_top_b / trace_index_b, finish_forward_b and close_records) is built with
-fsanitize=address,undefined and run on a text dump of the cases; the score and the corner list of every request must be the
restatement's, in the thin layout and in the tiled one, and the sanitizers must have nothing to say.  No GPU; nothing is loaded
into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import host_logic
from spaln_amd import abi
from tests import thin_cases as tc
from tests import unspliced_ref as ubr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(names, thin_allowed):
    """the text b_thin_host_check reads, and [(recipe, index)] by case id"""
    lines, ids = [], []
    for name in names:
        sc, up, ps, _ = tc.build(name)
        mtx = [sc.mtx[k] for k in range(sc.mtx_dim * sc.mtx_dim)]
        lines.append("S " + " ".join(str(int(x)) for x in [sc.mtx_dim] + mtx + [sc.gop, sc.gep, sc.lgop, sc.lgep, sc.codonk1, sc.noll, sc.local, sc.sh]) +
                     f" {up.tgapf!r}")
        for i, p in enumerate(ps.items):
            a = np.frombuffer((C.c_uint8 * p.a_len).from_address(p.a), dtype=np.uint8) if p.a_len else np.zeros(0, dtype=np.uint8)
            b = np.frombuffer((C.c_uint8 * p.b_len).from_address(p.b), dtype=np.uint8) if p.b_len else np.zeros(0, dtype=np.uint8)
            lines.append("P " + " ".join(str(int(x)) for x in [p.a_len, p.b_len] + a.tolist() + b.tolist()))
            lines.append("C " + " ".join(str(int(x)) for x in [len(ids), p.a_left, p.a_right, p.b_left, p.b_right, p.a_exgl, p.a_exgr, p.b_exgl, p.b_exgr,
                                                                 int(thin_allowed)]))
            ids.append((name, i))
    return "\n".join(lines) + "\n", ids


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("b_thin_host") / "b_thin_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", out, os.path.join(ROOT, "tests", "b_thin_host_check.cpp")])
    return out


@pytest.fixture(scope="module")
def wanted():
    """the restatement's (score, skl) of every case, computed once"""
    return {name: [ubr.align(sc, up, p) for p in ps.items] for name in tc.names() for sc, up, ps, _ in [tc.build(name)]}


def run(exe, tmp_path, thin_allowed):
    text, ids = dump(tc.names(), thin_allowed)
    path = tmp_path / "cases.txt"
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])      # a clean sanitizer exit
    got = {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        assert f[1] != "FAILED", (ln, ids[int(f[0])])
        v = [int(x) for x in f]
        assert len(v) == 4 + 2 * v[3], ln
        got[ids[v[0]]] = (v[1], v[2], [tuple(v[k:k + 2]) for k in range(4, len(v), 2)])
    assert len(got) == len(ids)
    return got


def as_skl(score, recs):
    """globalB_ng's tail: header + stdskl of the records, nothing where there is no alignment"""
    if not recs or score <= abi.NEVSEL:
        return []
    corners = host_logic.std_skl(list(recs))
    return [[1, len(corners)]] + [list(c) for c in corners]


@pytest.mark.parametrize("thin_allowed", [True, False], ids=["thin", "tiled"])
def test_every_case_equals_the_restatement(exe, wanted, tmp_path, thin_allowed):
    got = run(exe, tmp_path, thin_allowed)
    n_thin = 0
    for name in tc.names():
        sc, up, ps, tags = tc.build(name)
        for i, p in enumerate(ps.items):
            score, served, recs = got[(name, i)]
            wscore, wskl = wanted[name][i]
            g = tc.geometry(p, sc.sh)
            assert served == (0 if g["host"] else (1 if thin_allowed and g["rows"] <= 16 else 2)), (name, i, tags[i])
            n_thin += served == 1
            assert score == wscore and as_skl(score, recs) == wskl.tolist(), (name, i, tags[i], score, wscore, recs, wskl.tolist())
    assert n_thin == (sum(tc.predict(*tc.build(name)[:3])["thin_requests"] for name in tc.names() if "tight" not in name) +
                      sum(tc.predict(*tc.build(name)[:3])["requests_le16_rows"] for name in tc.names() if "tight" in name) if thin_allowed else 0)
