"""The splice-signal kernels (spdp_signals.hip: spdp_signals; spdp_signals_h.hip: spdh_signals, spdh_signal_phases,
spdh_signal_pack) on the device against the oracle, case by case and as batches: every recipe of tests/signal_cases.py through
spdp_splice_signals / spdp_splice_signals_h; the column records of whole batches (spdp_signal_records_s / _h) made from codes
against the records the host packs from the oracle's arrays, byte for byte; a batch of 65 537 windows (two launches); alignments
from codes against alignments from the oracle's arrays; the refusals by name.  Integer arrays, compared exactly, every cell."""
import ctypes as C

import numpy as np
import pytest

from oracle import signals, signals_h
from tests import signal_cases as sc
from tests import spdg
from tests.conftest import golden_files

pytestmark = pytest.mark.gpu
KEYS_S = ("sig5", "sig3", "cano5", "cano3", "dinc")
KEYS_H = ("sig5", "sig3", "sigS", "sigT", "sigE", "phs5", "phs3", "dinc")


@pytest.fixture(scope="module")
def eng():
    from spaln_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


_MODELS = {}


def _model(c):
    from spaln_amd import abi
    key = (c["kind"], c["model_name"])
    if key not in _MODELS:
        _MODELS[key] = (abi.signal_model_from_fixture if c["kind"] == "s" else abi.signal_model_h_from_fixture)(c["model"])
    return _MODELS[key]


# ---- one window per call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sc.GROUPS[:5] + ("order",))
def test_cdna_windows_equal_oracle(eng, group):
    n = 0
    for c in sc.cases("s"):
        if c["group"] != group:
            continue
        want = sc.expected(c)
        got = eng.splice_signals(_model(c), c["codes"], c["left"], c["right"])
        for k in KEYS_S:
            m = want["mask"] if k in ("sig5", "sig3") else slice(None)         # (long windows: the spans the oracle evaluated)
            assert np.array_equal(got[k][m], want[k][m]), (c["name"], k, np.flatnonzero(got[k] != want[k])[:8])
        outside = np.ones(c["codes"].size + 1, dtype=bool); outside[c["left"]:c["right"]] = False
        assert not got["sig5"][outside].any() and not got["sig3"][outside].any(), c["name"]
        n += 1
    assert n >= 2


@pytest.mark.parametrize("group", sc.GROUPS)
def test_protein_windows_equal_oracle(eng, group):
    n = 0
    for c in sc.cases("h"):
        if c["group"] != group:
            continue
        want = sc.expected(c)
        got = eng.splice_signals_h(_model(c), c["codes"], c["left"], c["right"])
        for k in KEYS_H:                                                       # b_len + 3 cells each, the tail included
            assert got[k].size == c["codes"].size + 2
            assert np.array_equal(got[k], want[k]), (c["name"], k, np.flatnonzero(got[k] != want[k])[:8])
        n += 1
    assert n >= 6


# ---- batches: the column records from codes against the host's packing of the oracle's arrays ------------------------------------------
def _batches(kind):
    """the cases by model, shuffled so that the longest window is neither first nor last"""
    by = {}
    for c in sc.cases(kind):
        by.setdefault(c["model_name"], []).append(c)
    for name, cs in sorted(by.items()):
        order = np.random.default_rng(len(name) + len(cs)).permutation(len(cs)).tolist()
        cs = [cs[i] for i in order]
        if len(cs) > 2:
            k = max(range(len(cs)), key=lambda i: cs[i]["codes"].size)
            cs.insert(len(cs) // 2, cs.pop(k))
        yield name, cs


def _inner(c, i):
    """an engine sub-range inside the case's range (what a call between two HSPs passes; the signals follow exin_left / exin_right)"""
    lf, rt = c["left"], c["right"]
    return (lf, rt) if i % 3 == 0 or rt - lf < 8 else (lf + 1 + i % 3, rt - 2 - i % 2)


def _sets_s(cs):
    from spaln_amd import abi
    arrays, codes = abi.ProblemSet(), abi.ProblemSet()
    q = np.array([2, 3, 5, 9, 2, 5, 9, 3, 2, 2], dtype=np.uint8)
    for i, c in enumerate(cs):
        e = sc.expected(c, full=True)
        bl, br = _inner(c, i)
        for ps, full in ((arrays, True), (codes, False)):
            p = ps.add(q, c["codes"], e["sig5"] if full else None, e["sig3"] if full else None, 0, q.size, bl, br,
                       **(dict(cano5=e["cano5"], cano3=e["cano3"], dinc=e["dinc"]) if full else {}))
            p.exin_left, p.exin_right = c["left"], c["right"]
    return arrays, codes


def _sets_h(cs):
    from spaln_amd import abi
    arrays, codes = abi.ProblemSetH(), abi.ProblemSetH()
    q = np.arange(3, 15, dtype=np.uint8)
    for i, c in enumerate(cs):
        e = sc.expected(c)
        bl, br = _inner(c, i)
        arrays.add(q, c["codes"], *(e[k] for k in KEYS_H[:7]), 0, q.size, bl, br, exin=(c["left"], c["right"]), dinc=e["dinc"])
        codes.add(q, c["codes"], *([None] * 7), 0, q.size, bl, br, exin=(c["left"], c["right"]))
    return arrays, codes


@pytest.mark.parametrize("spj,ipen", [(1, -245), (0, -245), (1, 0)], ids=["spj1", "spj0", "ipen0"])
def test_cdna_records_from_codes_equal_records_from_oracle_arrays(eng, spj, ipen):
    from spaln_amd import defaults
    intpen, t53 = defaults.exact_tables()
    n = 0
    for name, cs in _batches("s"):
        pa, pc = _sets_s(cs)
        ra = eng.signal_records_s(defaults.scoring(spj=spj, ipen=ipen, intpen=intpen, t53=t53), pa)
        rc = eng.signal_records_s(defaults.scoring(spj=spj, ipen=ipen, intpen=intpen, t53=t53, sigmodel=_model(cs[0])), pc)
        assert np.array_equal(ra["col_off"], rc["col_off"]) and ra["aux"] is not None and rc["aux"] is not None
        for i, c in enumerate(cs):                                             # (by problem, for the message; then the whole buffers)
            lo, hi = int(ra["col_off"][i]), int(ra["col_off"][i + 1])
            assert hi - lo >= c["codes"].size + 1
            assert np.array_equal(ra["cols"][lo:hi], rc["cols"][lo:hi]), (name, c["name"], np.flatnonzero((ra["cols"][lo:hi] != rc["cols"][lo:hi]).any(axis=1))[:8])
            assert np.array_equal(ra["aux"][lo:hi], rc["aux"][lo:hi]), (name, c["name"])
        assert ra["cols"].tobytes() == rc["cols"].tobytes() and ra["aux"].tobytes() == rc["aux"].tobytes()
        assert (ra["max_s5"], ra["max_s3"]) == (rc["max_s5"], rc["max_s3"]), name
        n += len(cs)
    assert n == len(sc.cases("s"))


@pytest.mark.parametrize("spj,ipen", [(1, -401), (0, -401), (1, 0)], ids=["spj1", "spj0", "ipen0"])
def test_protein_records_from_codes_equal_records_from_oracle_arrays(eng, spj, ipen):
    from spaln_amd import defaults
    n = 0
    for name, cs in _batches("h"):
        pa, pc = _sets_h(cs)
        ra = eng.signal_records_h(defaults.scoring_h(spj=spj, ipen=ipen), pa)
        rc = eng.signal_records_h(defaults.scoring_h(spj=spj, ipen=ipen, sigmodel=_model(cs[0])), pc)
        assert np.array_equal(ra["col_off"], rc["col_off"])
        for i, c in enumerate(cs):
            lo, hi = int(ra["col_off"][i]), int(ra["col_off"][i + 1])
            assert hi - lo >= c["codes"].size + 2
            assert np.array_equal(ra["cols"][lo:hi], rc["cols"][lo:hi]), (name, c["name"], np.flatnonzero((ra["cols"][lo:hi] != rc["cols"][lo:hi]).any(axis=1))[:8])
            assert np.array_equal(ra["aux"][lo:hi], rc["aux"][lo:hi]), (name, c["name"])
        assert ra["cols"].tobytes() == rc["cols"].tobytes() and ra["aux"].tobytes() == rc["aux"].tobytes()
        n += len(cs)
    assert n == len(sc.cases("h"))


@pytest.mark.parametrize("kind", ["s", "h"])
def test_second_launch_of_a_large_batch(eng, kind):
    """65 537 windows, 16 distinct ones of 5 .. 40 bases in turn: the kernels take at most 65 535 jobs per launch, so the last two
    windows belong to a second launch, whose job pointer and offsets must continue the first's"""
    from spaln_amd import abi, defaults
    n_jobs, rng = 65537, np.random.default_rng(11)
    src = sc.case(f"{kind}/length/{256}")
    model = _model(src)
    wins = []
    for k in range(16):
        n = 5 + (k * 7) % 36
        at = 3 * k
        w = src["codes"][at:at + n].copy()
        wins.append(w if kind == "s" else np.concatenate([w, [0]]).astype(np.uint8))
    q = np.arange(3, 13, dtype=np.uint8)
    ps = abi.ProblemSet() if kind == "s" else abi.ProblemSetH()
    for j in range(n_jobs):
        w = wins[j % 16]
        if kind == "s":
            ps.add(q, w, None, None)
        else:
            ps.add(q, w, *([None] * 7))
    if kind == "s":
        intpen, t53 = defaults.exact_tables()
        rec = eng.signal_records_s(defaults.scoring(intpen=intpen, t53=t53, sigmodel=model), ps)
    else:
        rec = eng.signal_records_h(defaults.scoring_h(sigmodel=model), ps)
    off = rec["col_off"]
    assert off.size == n_jobs + 1 and np.all(np.diff(off) > 0)
    for j in list(range(16)) + list(range(65535 - 16, n_jobs)):
        k = j % 16
        for key in ("cols", "aux"):
            a = rec[key][off[j]:off[j + 1]]
            b = rec[key][off[k]:off[k + 1]]
            assert np.array_equal(a, b), (j, key)
    # and the first 16 are what one window per call gives
    for k in range(16):
        if kind == "s":
            one = eng.splice_signals(model, wins[k])
            s5 = (rec["cols"][off[k]:off[k] + wins[k].size + 1, 0] & 0xffff).astype(np.uint16).view(np.int16)
            assert np.array_equal(s5, (one["sig5"] + np.int16(defaults.IPEN)).astype(np.int16))
        else:
            one = eng.splice_signals_h(model, wins[k])
            assert np.array_equal(rec["aux"][off[k]:off[k] + wins[k].size + 2, 3], one["sig5"])


# ---- alignments from codes against alignments from the oracle's arrays ------------------------------------------------------------------
_GENES = {}


def _genes_s():
    """24 planted genes with a few Ns in their introns, sub-ranges, and the oracle's arrays under the fixtures' model"""
    if "s" not in _GENES:
        from spaln_amd import synth
        fx = spdg.load(golden_files("s1_basic")[0])
        md = signals.model_of(fx)
        out = []
        for i, (w, q, _s5, _s3, exons) in enumerate(synth.make_batch(24, seed=4242, mrna_len=400, n_exons=3, flank=120, intron_hi=300)):
            w = w.copy()
            for k, (lo, hi) in enumerate(exons[:-1]):
                w[hi + 20 + k] = sc.N_CODE                                     # inside an intron, off the site's context
            lf, rt = (0, w.size) if i % 4 == 0 else (1 + i % 5, w.size - 2 - i % 3)
            s5, s3 = signals.splice_signals(md, w, lf, rt)
            d5, d3, c5, c3 = signals.classes(w, lf, rt, md["any"], md["both_ori"])
            out.append(dict(w=w, q=q, lf=lf, rt=rt, sig5=s5, sig3=s3, cano5=c5, cano3=c3, dinc=((d5 << 4) | d3).astype(np.uint8)))
        _GENES["s"] = (fx, out)
    return _GENES["s"]


def _genes_h():
    if "h" not in _GENES:
        from spaln_amd import synth
        fx = spdg.load([f for f in golden_files("h1_") if f.endswith("h1_basic.spdg")][0])
        md = signals_h.model_of(fx)
        out = []
        for i, (g, sg) in enumerate(synth.make_protein_batch(24, seed=4343, aa_len=90, n_exons=3, flank=150, intron_hi=300)):
            b = sg["b"].copy()
            for k, (lo, hi) in enumerate(g.exons[:-1]):
                b[hi + 25 + k] = 2                                             # an unknown codon inside an intron
            b_len = b.size - 1
            lf, rt = (0, b_len) if i % 4 == 0 else (1 + i % 5, b_len - 2 - i % 3)
            e = signals_h.splice_signals_h(md, b, b_len, lf, rt)
            d5, d3, _, _ = signals_h.classes(b[:b_len], lf, rt, md["any"])
            e["dinc"] = ((d5 << 4) | d3).astype(np.uint8)
            out.append(dict(b=b, q=synth.encode_protein(g.query), lf=lf, rt=rt, e=e))
        _GENES["h"] = (fx, out)
    return _GENES["h"]


@pytest.mark.parametrize("engines", [0, 1, 2])
def test_cdna_alignments_from_codes_equal_alignments_from_oracle_arrays(eng, engines):
    from spaln_amd import abi
    fx, genes = _genes_s()
    model = abi.signal_model_from_fixture(fx)
    pa, pc = abi.ProblemSet(), abi.ProblemSet()
    for g in genes:
        pa.add(g["q"], g["w"], g["sig5"], g["sig3"], 0, None, g["lf"], g["rt"], cano5=g["cano5"], cano3=g["cano3"], dinc=g["dinc"])
        p = pc.add(g["q"], g["w"], None, None, 0, None, g["lf"], g["rt"])
        p.exin_left, p.exin_right = g["lf"], g["rt"]
    ra = [(s, skl.tolist()) for s, skl in eng.align_s(spdg.scoring(fx, scalar_engines=engines), pa)]
    rc = [(s, skl.tolist()) for s, skl in eng.align_s(spdg.scoring(fx, scalar_engines=engines, sigmodel=model), pc)]
    assert ra == rc
    assert sum(1 for s, skl in rc if len(skl) > 3) >= len(genes) - 2


@pytest.mark.parametrize("engines", [0, 1])
def test_protein_alignments_from_codes_equal_alignments_from_oracle_arrays(eng, engines):
    from spaln_amd import abi
    fx, genes = _genes_h()
    model = abi.signal_model_h_from_fixture(fx)
    pa, pc = abi.ProblemSetH(), abi.ProblemSetH()
    for g in genes:
        e = g["e"]
        pa.add(g["q"], g["b"], *(e[k] for k in KEYS_H[:7]), 0, None, g["lf"], g["rt"], exin=(g["lf"], g["rt"]), dinc=e["dinc"])
        pc.add(g["q"], g["b"], *([None] * 7), 0, None, g["lf"], g["rt"], exin=(g["lf"], g["rt"]))
    ra = [(s, skl.tolist(), f) for s, skl, f in eng.align_h(spdg.scoring_h(fx, scalar_engines=engines), pa)]
    rc = [(s, skl.tolist(), f) for s, skl, f in eng.align_h(spdg.scoring_h(fx, scalar_engines=engines, sigmodel=model), pc)]
    assert ra == rc
    assert sum(1 for s, skl, f in rc if len(skl) > 3) >= len(genes) - 2


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _with_shape(fx, tag, **hdr):
    """the model dict with one matrix header changed (rows / cols / offset / order) and a matrix of the size it then claims"""
    out = dict(fx)
    h = np.array(fx[tag + "_hdr"]).copy()
    for k, v in hdr.items():
        h[("rows", "cols", "offset", "order").index(k)] = v
    out[tag + "_hdr"] = h
    out[tag + "_f32"] = np.concatenate([fx[tag + "_f32"][:2], np.zeros(int(h[0]) * int(h[1]), dtype=np.int32)])
    return out


def test_refusals_by_name(eng):
    from spaln_amd import abi, defaults
    cs, ch = sc.case("s/bad/none"), sc.case("h/bad/none")
    b, bh = cs["codes"], ch["codes"]
    # shapes the launcher's LDS windows do not hold.  (cols - offset + 2 > 60 would need cols > 48, refused before it: the bound
    # cannot bind on its own)
    for bad in (dict(cols=49), dict(offset=61), dict(offset=-1)):
        with pytest.raises(RuntimeError, match="matrix shape out of range"):
            eng.splice_signals(abi.signal_model_from_fixture(_with_shape(cs["model"], "pm3", **bad)), b)
        with pytest.raises(RuntimeError, match="matrix shape out of range"):
            eng.splice_signals_h(abi.signal_model_h_from_fixture(_with_shape(ch["model"], "pmI", **bad)), bh)
    with pytest.raises(RuntimeError, match="84 rows"):
        eng.splice_signals(abi.signal_model_from_fixture(_with_shape(_with_shape(cs["model"], "pm5", rows=20), "pm3", rows=20)), b)
    for tag, bad in (("pm5", dict(rows=20)), ("pmI", dict(rows=84)), ("pmT", dict(order=0)), ("pm3", dict(order=3, rows=340))):
        with pytest.raises(RuntimeError, match="rows do not match its Markov order"):
            eng.splice_signals_h(abi.signal_model_h_from_fixture(_with_shape(ch["model"], tag, **bad)), bh)
    pot = dict(ch["model"], potC_hdr=np.array([1024, 3], dtype=np.int32), potC_f32=ch["model"]["potC_f32"][:3 * 1024])
    with pytest.raises(RuntimeError, match="5th-order table"):
        eng.splice_signals_h(abi.signal_model_h_from_fixture(pot), bh)
    # windows
    ms, mh = _model(cs), _model(ch)
    for lf, rt in ((0, b.size + 1), (-1, b.size), (9, 8)):
        with pytest.raises(RuntimeError, match="spdp_splice_signals: bad window"):
            eng.splice_signals(ms, b, lf, rt)
    for lf, rt in ((0, bh.size), (-1, bh.size - 1), (9, 8)):
        with pytest.raises(RuntimeError, match="spdp_splice_signals_h: bad window"):
            eng.splice_signals_h(mh, bh, lf, rt)
    # the Exinon range of a problem: inside the sequence, around the active range
    q = np.arange(3, 13, dtype=np.uint8)
    b_len = bh.size - 1
    for exin, why in (((-1, b_len), "Exinon range outside the sequence"), ((0, b_len + 1), "Exinon range outside the sequence"),
                      ((0, b_len + 3), "Exinon range outside the sequence"), ((5, b_len), "active range outside the Exinon range")):
        ps = abi.ProblemSetH()
        ps.add(q, bh, *([None] * 7), 0, None, 0, b_len, exin=exin)
        with pytest.raises(RuntimeError, match="problem 0: " + why):
            eng.signal_records_h(defaults.scoring_h(sigmodel=mh), ps)
    for exin in ((-1, b.size), (0, b.size + 1), (3, b.size)):
        ps = abi.ProblemSet()
        p = ps.add(q, b, None, None, 0, None, 1, b.size)
        p.exin_left, p.exin_right = exin
        with pytest.raises(RuntimeError, match="exin_left / exin_right must enclose"):
            eng.signal_records_s(defaults.scoring(sigmodel=ms), ps)
    # the records entries themselves
    ps = abi.ProblemSet()
    ps.add(q, b, None, None)
    with pytest.raises(RuntimeError, match="sigmodel"):
        eng.signal_records_s(defaults.scoring(), ps)
    with pytest.raises(RuntimeError, match="spdp_signal_records_s: null argument or empty batch"):
        eng.signal_records_s(defaults.scoring(sigmodel=ms), abi.ProblemSet())
    with pytest.raises(RuntimeError, match="spdp_signal_records_h: null argument or empty batch"):
        eng.signal_records_h(defaults.scoring_h(sigmodel=mh), abi.ProblemSetH())
    off = np.zeros(2, dtype=np.int64)
    small = np.zeros(8, dtype=np.int32)
    assert eng.lib.spdp_signal_records_s(eng.ctx, C.byref(defaults.scoring(sigmodel=ms)), ps.array(), 1, off.ctypes.data, 1,
                                         small.ctypes.data, None, None) == -1
    assert b"capacity below col_off[n]" in eng.lib.spdp_last_error(eng.ctx)
    assert eng.lib.spdp_signal_records_s(None, None, None, 0, None, 0, None, None, None) == -1
    assert eng.lib.spdp_signal_records_h(None, None, None, 0, None, 0, None, None) == -1
