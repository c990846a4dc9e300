"""The seeded walk of the unspliced aligner on the CPU against every recorded fixture: tests/b_seeded_host_check.cpp (a program
with its own main: the walk header, the HSP search, lastB_ng and the record walk of the product, and a host emulation of the
two sweeps -- the thin one lane by lane with the shared step function) is built with -fsanitize=address,undefined, run on a
text dump of the fixtures, and every record it prints must be the program's.  No GPU; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from oracle import host_logic
from spaln_amd import abi, defaults
from tests import unspliced_ref as ubr
from tests import unspliced_seeded_cases as usc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_words(m: abi.WilipModel):
    out = []
    for i in range(3):
        L = m.level[i]
        out += [L.elem, L.tpl, L.mask, L.width, L.gain, L.gain1, L.thr, L.xdrp, L.cutoff, L.vthr, L.bitpat_len]
        out += list(L.bitpat) + list(L.convtab)
    out += [m.mtx_rows, m.mtx_cols] + [m.mtx[k] for k in range(m.mtx_rows * m.mtx_cols)]
    out += [m.dvsp, m.end_bonus, m.crs, m.lsg, m.mlt, m.shortquery, m.min_hit, m.met, m.ser, m.ser2]
    return out


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    """builds the program, runs it once over every fixture record; {case id: (score, records)} and the case list"""
    tmp = tmp_path_factory.mktemp("b_seeded_host")
    exe = str(tmp / "b_seeded_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "b_seeded_host_check.cpp")])
    sc0 = defaults.scoring_b()
    words = _model_words(defaults.wilip_model_b())
    words += [sc0.mtx_dim] + [sc0.mtx[k] for k in range(sc0.mtx_dim * sc0.mtx_dim)]
    words += [sc0.gop, sc0.gep, sc0.lgop, sc0.lgep, sc0.codonk1, sc0.sh]
    cases = []
    lines = []
    keep = []                                        # (the problem sets own the buffers the problems point into)
    for name, k in usc.runs():
        sc, up, sp, ps, recs, opts = usc.problems(name, k)
        assert (sc.gop, sc.gep, sc.lgop, sc.lgep, sc.codonk1, sc.sh) == (sc0.gop, sc0.gep, sc0.lgop, sc0.lgep, sc0.codonk1, sc0.sh)
        doc = usc.load(name)
        keep.append(ps)
        for i, p in enumerate(ps.items):
            a, b = usc.uc.encode(doc["pairs"][i]["a"]), usc.uc.encode(doc["pairs"][i]["b"])
            cid = len(cases)
            cases.append((name, k, i, sc, up, p, recs[i], opts))
            lines.append(" ".join(str(int(x)) for x in [cid, a.size, b.size] + a.tolist() + b.tolist() + [sc.noll, sc.local]) +
                         f" {up.tgapf!r} {sp.qck} {sp.vthr} {p.a_exgl} {p.a_exgr} {p.b_exgl} {p.b_exgr} " + " ".join(str(sp.wl_width[j]) for j in range(4)))
    path = tmp / "cases.txt"
    path.write_text(" ".join(str(int(x)) for x in words) + f"\n{len(cases)}\n" + "\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])      # a clean sanitizer exit
    got = {}
    tail = ""
    for ln in r.stdout.splitlines():
        if ln.startswith("#"):
            tail = ln
            continue
        f = ln.split()
        assert f[1] != "FAILED", ln
        v = [int(x) for x in f]
        got[v[0]] = (v[1], np.asarray(v[3:], dtype=np.int32).reshape(-1, 2))
        assert got[v[0]][1].shape[0] == v[2]
    return cases, got, tail, keep


def test_every_fixture_record_matches(checked):
    cases, got, _, _keep = checked
    assert len(got) == len(cases) and len(cases) > 1500
    for cid, (name, k, i, sc, up, p, rec, opts) in enumerate(cases):
        score, recs = got[cid]
        what = (name, opts, i)
        if rec is None:
            assert recs.shape[0] == 0, what
            continue
        assert recs.shape[0] >= 1, what
        corners = host_logic.std_skl([list(r) for r in recs.tolist()])
        skl = np.asarray([[1, len(corners)]] + [list(c) for c in corners], dtype=np.int32)
        stat, trimmed, ed, _ = ubr.rescore(sc, up, p, skl, abi.FMT_CIGAR)
        usc.uc.check_record(stat, trimmed, rec, what)
        assert [[chr(o), l] for o, l, _ in ed.tolist()] == (rec["cigar"] or []), what


def test_both_sweep_forms_were_exercised(checked):
    """the walk ran: every pair searched its HSPs at least once (no pair brings any), and the requests between them came in
    both sizes -- at most 16 rows (the thin form: the `gaps` set plants blocks of 1 .. 16 residues) and more (the tiled layout)"""
    cases, _, tail, _keep = checked
    f = tail.replace(",", "").replace(";", "").split()
    thin, wide, searches = int(f[2]), int(f[4]), int(f[10])
    assert thin > 0 and wide > 0 and searches >= len(cases), tail
