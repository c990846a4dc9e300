"""Windows, ranges and signal models for the splice-signal kernels (spdp_signals.hip, spdp_signals_h.hip), built by named
recipe; shared by tests/test_signal_cases.py (the generator against the oracle, CPU) and tests/test_gpu_signal_cases.py
(spdp_splice_signals / _h and the column records on the device).

A case is a dict: name, kind ("s": cDNA side, "h": protein side), group, codes (kind h: b_len + 1 tron codes, the last a
terminator), left, right, model (a fixture-shaped dict that oracle.signals*.model_of and abi.signal_model*_from_fixture read),
model_name (cases with the same one share a batch), spans (kind s, long windows: the stretches the oracle evaluates, or None).
expected(case) gives the oracle's arrays, cached.  Everything is a function of the case's name.

The models are random: matrix entries +-u * 2^k, k = -6 .. 6, so that the order of the float additions decides some results
(tests/test_signal_cases.py counts them), scaled so that no signal leaves the int16 range (the reference's cast would be
undefined there).  Groups (GROUPS): length, range, bad, mode, shape, phase, stop, branch; kind s alone: order."""
import functools
import zlib

import numpy as np

from oracle import signals, signals_h

GROUPS = ("length", "range", "bad", "mode", "shape", "phase", "stop", "branch")      # kind s: the first five and "order"
NT = np.array([2, 3, 5, 9], dtype=np.uint8)                 # A C G T in the nucleotide code
N_CODE = 15
TRON_OF = ([5, 6, 8, 9, 11, 14, 21], [3, 17, 18, 19], [4, 7, 10, 20, 23], [12, 13, 15, 16, 22])   # tron codes by middle base, stops apart
TRM, TRM2 = 25, 24                                          # TAA / TAG, TGA: middle bases A, G
BAD_TRON = [0, 1, 2, 26, 27, 28, 29, 30, 31]                # tnredctab says "none" (26 .. 31: beyond the reference's table)
LEN_S = (0, 1, 2, 3, 5, 23, 24, 25, 255, 256, 257, 4095, 4096, 4097, 4096 + 256, 8192)
LEN_H = (0, 1, 2, 3, 5, 8, 252, 253, 254, 256, 509, 510)
SHAPES = (((1, 0), (2, 1)), ((48, 0), (48, 47)), ((24, 60), (48, 10)))      # (cols, offset) of the donor and the acceptor matrix
# (cols - offset + 2 is at most 50 with cols <= 48: the launcher's bound of 60 on it cannot bind; (48, 0) is the widest reach)
SIGMA = 15.6                                                # rms of one matrix entry as drawn below


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _bits(*f):
    return np.array(f, dtype=np.float32).view(np.int32)


# ---- models -----------------------------------------------------------------------------------------------------------------------
def _matrix(rng, cols, offset, order, tonic=0.0):
    """entries over many binades; min_elem (what a window with a bad base scores per column) is a free field of the model"""
    rows = (4, 20, 84)[order]
    k = rng.integers(-6, 7, size=rows * cols)
    m = (rng.uniform(0.5, 1.0, size=rows * cols) * np.exp2(k) * rng.choice([-1.0, 1.0], size=rows * cols)).astype(np.float32)
    return np.array([rows, cols, offset, order, 4], dtype=np.int32), np.concatenate([_bits(tonic, -4.0), m.view(np.int32)])


def _scale(cols, order):
    """fs such that the scaled scan stays inside +-32000 (checked on every evaluated position by tests/test_signal_cases.py)"""
    return float(np.float32(30000.0 / (6.0 * SIGMA * np.sqrt(cols + order))))


@functools.lru_cache(maxsize=None)
def model_s(name="m0", shape5=(24, 3), shape3=(24, 23), any_=0, both_ori=0):
    rng = _rng("model_s/" + name)
    h5, f5 = _matrix(rng, *shape5, 2)
    h3, f3 = _matrix(rng, *shape3, 2)
    fs = min(_scale(shape5[0], 2), _scale(shape3[0], 2))
    tab = rng.integers(-60, 30, size=32).astype(np.int32)
    return {"pm5_hdr": h5, "pm5_f32": f5, "pm3_hdr": h3, "pm3_f32": f3, "sig53tab01": tab,
            "sigmodel": np.array([_bits(fs)[0], any_, 1, both_ori], dtype=np.int32)}


NO_PM = (np.zeros(5, dtype=np.int32), np.zeros(0, dtype=np.int32))


@functools.lru_cache(maxsize=None)
def model_h(name="m0", pm5=(24, 3, 2), pm3=(24, 23, 2), pmI=(20, 11, 1), pmT=(3, 2, 2), pmB=None, any_=0, dvsp=1, pot=4096,
            maxb3d=20):
    """pm*: (cols, offset, order) or None.  The phase thresholds sit half a standard deviation below the mean signal (under any = 2 most
    cells the sites around them leave unmarked are threshold sites), the branch threshold 0.8 above: every fifth position"""
    rng = _rng("model_h/" + name)
    fx = {}
    for tag, shp in (("pm5", pm5), ("pm3", pm3), ("pmI", pmI), ("pmT", pmT), ("pmB", pmB)):
        fx[tag + "_hdr"], fx[tag + "_f32"] = _matrix(rng, *shp) if shp else NO_PM
    fs = min(_scale(pm5[0], pm5[2]), _scale(pm3[0], pm3[2]))
    fT = min(_scale(s[0], s[2]) for s in (pmI, pmT) if s) if (pmI or pmT) else 1.0
    fB = _scale(pmB[0], pmB[2]) / 4 if pmB else 0.0        # (added to sig3: a quarter of the range)
    sd = lambda s: SIGMA * float(np.sqrt(s[0] + s[2]))
    f = [20.0, 0.0, fT, fB, -475.0, fs, fs * 0.75, -0.5 * sd(pm3), -0.5 * sd(pm5), 0.8 * sd(pmB) if pmB else 0.0]
    fx["sigmodel_f32"] = _bits(*f)                           # fE fI fT fB fO fS fs tonic3 tonic5 tonicB
    fx["sigmodel_i32"] = np.array([any_, 1 if dvsp else 3, maxb3d, 1, 4, TRM, TRM2], dtype=np.int32)
    fx["sig53tab01"] = rng.integers(-60, 30, size=32).astype(np.int32)
    fx["potC_hdr"] = np.array([pot, 3], dtype=np.int32)
    fx["potC_f32"] = (rng.normal(0.0, 2.0, size=3 * pot).astype(np.float32) * np.exp2(rng.integers(-3, 3, size=3 * pot)).astype(np.float32)
                      ).astype(np.float32).view(np.int32) if pot else np.zeros(0, dtype=np.int32)
    return fx


# ---- sequences ----------------------------------------------------------------------------------------------------------------------
def _bases(rng, n):
    return rng.integers(0, 4, size=n)


def _put(b, at, word):
    """ACGT letters (N or any other letter: bad) into the base array, clipped to it"""
    for i, ch in enumerate(word):
        if 0 <= at + i < b.size:
            b[at + i] = "ACGT".find(ch) if ch in "ACGT" else 4


def _codes(kind, rng, b, bad_codes=None, stops=()):
    """bases 0 .. 3 / 4 = bad -> nucleotide codes, or tron codes + terminator (a stop code where `stops` says so: its middle base
    must be A for TRM, G for TRM2)"""
    b = np.asarray(b)
    if kind == "s":
        out = np.where(b < 4, NT[np.minimum(b, 3)], N_CODE).astype(np.uint8)
        if bad_codes is not None:
            out[b > 3] = rng.choice(bad_codes, size=int((b > 3).sum()))
        return out
    out = np.zeros(b.size + 1, dtype=np.uint8)
    for i, v in enumerate(b):
        out[i] = rng.choice(TRON_OF[v]) if v < 4 else rng.choice(BAD_TRON if bad_codes is None else bad_codes)
    for i in stops:
        if 0 <= i < b.size:
            out[i] = TRM if i % 2 else TRM2
    return out


def _case(kind, group, name, codes, left, right, model, model_name, spans=None):
    return dict(kind=kind, group=group, name=f"{kind}/{group}/{name}", codes=codes, left=int(left), right=int(right), model=model,
                model_name=model_name, spans=spans)


def _spans(n):
    """long cDNA windows: within 70 positions of every multiple of 256 and of both ends"""
    out, lo = [], None
    marks = sorted(set(list(range(0, n + 1, 256)) + [n]))
    for m in marks:
        a, b = max(0, m - 70), min(n, m + 70)
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


# ---- the recipes ----------------------------------------------------------------------------------------------------------------------
def _length(kind):
    out = []
    md, mn = (model_s(), "m0") if kind == "s" else (model_h(), "m0")
    for n in (LEN_S if kind == "s" else LEN_H):
        rng = _rng(f"{kind}/length/{n}")
        b = _bases(rng, n)
        if n >= 23:
            b[rng.integers(0, n, size=max(1, n // 400))] = 4       # a few bad bases
        for at in range(256, n + 1, 256):                          # a site across every chunk edge
            _put(b, at - 1, "GTGT" if (at // 256) % 2 else "AGAG")
        out.append(_case(kind, "length", str(n), _codes(kind, rng, b), 0, n, md, mn, _spans(n) if kind == "s" and n > 3000 else None))
    return out


def _range(kind):
    out = []
    md, mn = (model_s(), "m0") if kind == "s" else (model_h(), "m0")
    n = 300
    rng = _rng(f"{kind}/range")
    b = _bases(rng, n)
    _put(b, 0, "GTAGGT"); _put(b, n - 6, "AGGTAG")                # sites at both ends of the sequence
    codes = _codes(kind, rng, b)
    offs = (3, 23) if kind == "s" else (3, 11, 23)
    lefts = sorted({0, 1, 2, 3} | {o + d for o in offs for d in (-1, 0, 1)})
    rights = sorted({n, n - 1, n - 2, n - 3} | {n - c + d for c in ((24,) if kind == "s" else (3, 20, 24)) for d in (-1, 1)})
    for lf in lefts:
        out.append(_case(kind, "range", f"left{lf}", codes, lf, n, md, mn))
    for rt in rights:
        out.append(_case(kind, "range", f"right{rt}", codes, 0, rt, md, mn))
    for lf, rt in ((0, 0), (150, 150), (n, n), (0, 1), (149, 150), (n - 1, n), (3, n - 3), (24, n - 25)):
        out.append(_case(kind, "range", f"{lf}_{rt}", codes, lf, rt, md, mn))
    return out


def _bad(kind):
    out = []
    md, mn = (model_s(), "m0") if kind == "s" else (model_h(), "m0")
    n = 420
    rng = _rng(f"{kind}/bad")
    clean = _bases(rng, n)
    for at in (255, 256, 257):                                     # one bad base either side of the chunk edge: every distance
        b = clean.copy()                                           # -(cols + 2) .. cols + 2 from a checked position, across it
        b[at] = 4
        out.append(_case(kind, "bad", f"single{at}", _codes(kind, rng, b), 0, n, md, mn))
    out.append(_case(kind, "bad", "none", _codes(kind, rng, clean), 0, n, md, mn))
    b = clean.copy()
    for k in range(1, 10):                                         # pairs at spacing 1 .. 9, 40 apart
        b[40 * k] = b[40 * k + k] = 4
    out.append(_case(kind, "bad", "pairs", _codes(kind, rng, b), 0, n, md, mn))
    out.append(_case(kind, "bad", "all", _codes(kind, rng, np.full(100, 4)), 0, 100, md, mn))
    # the whole code range the kernels index: every nucleotide code 0 .. 16 and some above; every tron code 0 .. 31 and some
    # above (the pack maps those to the zero row of the matrix)
    rng2 = _rng(f"{kind}/bad/codes")
    top = 17 if kind == "s" else 32
    every = np.concatenate([np.arange(top), [top, top + 1, 63, 64, 100, 200, 255], rng2.integers(top, 256, size=30),
                            rng2.integers(0, top, size=300)]).astype(np.uint8)
    rng2.shuffle(every)
    out.append(_case(kind, "bad", "codes", every if kind == "s" else np.concatenate([every, [0]]).astype(np.uint8), 0, every.size, md, mn))
    if kind == "s":                                                # the block edge (SIG_TPB * SIG_CHUNKS = 4096)
        for at in (4095, 4096):
            rng3 = _rng(f"s/bad/block{at}")
            b = _bases(rng3, 4352)
            b[at] = 4
            out.append(_case(kind, "bad", f"block{at}", _codes(kind, rng3, b), 0, 4352, md, mn, _spans(4352)))
    return out


def _mode(kind):
    out = []
    n = 400
    rng = _rng(f"{kind}/mode")
    b = _bases(rng, n)
    b[[77, 200]] = 4
    codes = _codes(kind, rng, b)
    if kind == "s":
        for a in range(4):
            for o in (0, 1):
                out.append(_case(kind, "mode", f"any{a}_ori{o}", codes, 1, n - 1, model_s("m0", any_=a, both_ori=o), f"m0/any{a}_ori{o}"))
        return out
    for a in range(4):
        out.append(_case(kind, "mode", f"any{a}", codes, 1, n - 1, model_h("m0", any_=a), f"m0/any{a}"))
    # any = 3 gives every cell the class loop assigns a level, so the threshold rule (any == 2 only) would show at the two cells
    # it does not assign -- the donor cell right - 1 and the acceptor cell left: many ranges, so that some of those cells are
    # above the threshold and unmarked by a neighbouring site
    for k in range(70):
        out.append(_case(kind, "mode", f"any3_edge{k}", codes, 20 + 5 * k, 50 + 5 * k, model_h("m0", any_=3), "m0/any3"))
    out.append(_case(kind, "mode", "dvsp_off", codes, 1, n - 1, model_h("m0", dvsp=0), "m0/dvsp_off"))
    out.append(_case(kind, "mode", "no_pmI_pmT", codes, 1, n - 1, model_h("m0", pmI=None, pmT=None), "m0/no_pmI_pmT"))
    out.append(_case(kind, "mode", "pmB", codes, 1, n - 1, model_h("m0", pmB=(12, 8, 1)), "m0/pmB"))
    out.append(_case(kind, "mode", "no_pot", codes, 1, n - 1, model_h("m0", pot=0), "m0/no_pot"))
    return out


def _shape(kind):
    out = []
    n = 300
    rng = _rng(f"{kind}/shape")
    b = _bases(rng, n)
    b[[5, 150, n - 7]] = 4
    codes = _codes(kind, rng, b)
    for (s5, s3) in SHAPES:
        tag = f"{s5[0]}_{s5[1]}__{s3[0]}_{s3[1]}"
        if kind == "s":
            out.append(_case(kind, "shape", tag, codes, 0, n, model_s("sh" + tag, s5, s3), "sh" + tag))
            out.append(_case(kind, "shape", tag + "_sub", codes, 2, n - 2, model_s("sh" + tag, s5, s3), "sh" + tag))
            continue
        for order in (0, 1, 2):                                    # the same shapes at every Markov order, all five matrices
            md = model_h(f"sh{tag}_o{order}", s5 + (order,), s3 + (order,), s3 + (order,), s5 + (order,), s5 + ((order + 1) % 3,))
            out.append(_case(kind, "shape", f"{tag}_o{order}", codes, 1, n - 1, md, f"sh{tag}_o{order}"))
    return out


def _phase():
    """protein side: the sequential phase rule.  m0/any0: canonical sites only; m0/any2: threshold sites between them"""
    out = []
    n = 260
    rng = _rng("h/phase")
    b = _bases(rng, n)
    words = ["GTGT", "AGAG", "GTGTGT", "AGGT", "AGGTGT", "GTAG", "AGAGAG", "CAGGTA", "ATAC", "GCAG"]
    for k in range(24):
        _put(b, 10 + 10 * k, words[k % len(words)])
    codes = _codes("h", rng, b)
    for a in (0, 2):
        md = model_h("m0", any_=a)
        out.append(_case("h", "phase", f"words_any{a}", codes, 0, n, md, f"m0/any{a}"))
        for lf, word in ((10, "gt_at_left"), (9, "gt_at_left1"), (11, "gt_cut")):
            out.append(_case("h", "phase", f"{word}_any{a}", codes, lf, n, md, f"m0/any{a}"))
        for rt in (12, 13, 14):                                    # GT at right - 2, right - 3, right - 4: its marks reach `right`
            out.append(_case("h", "phase", f"gt_right{rt}_any{a}", codes, 0, rt, md, f"m0/any{a}"))
    return out


def _stop():
    """protein side: the stop-codon rules of sigE against `right` and the sequence end (pos + 3 < right && pos + 3 < len): one
    termination code at right + k, k = -4 .. 3, for ranges that end at, near and well inside the end of the sequence"""
    out = []
    md = model_h()
    n = 120
    for right in (n, n - 1, n - 2, n - 25, n - 30, n - 40, n - 50, n - 60, n - 70):
        rng = _rng(f"h/stop/{right}")
        b = _bases(rng, n)
        for k in range(-4, 4):
            at = [20, right + k]                                   # (and one well inside: both rules in every case)
            bb = b.copy()
            for i in at:
                if 0 <= i < n:
                    bb[i] = 0 if i % 2 else 2                      # middle base of TRM / TRM2
            out.append(_case("h", "stop", f"right{right}_stop{k}", _codes("h", _rng(f"h/stop/{right}"), bb, stops=at), 1, right, md, "m0"))
    for k in (0, 1, 2):                                            # six good bases between two bad ones, ending at right + k
        rng = _rng(f"h/stop/six/{k}")
        b = _bases(rng, n)
        right = n - 25
        b[right + k - 6] = 4
        b[right + k + 1] = 4
        out.append(_case("h", "stop", f"six{k}", _codes("h", rng, b), 1, right, md, "m0"))
    return out


def _order():
    """cDNA side: a model under which the order of the float additions decides the truncated result often.  Every other
    column of the trinucleotide part is raised by 2^13 and the ones between lowered by it: the partial sums swing between ~0 and
    ~8192 (rounding at 2^-10 there) while the whole sum keeps its size.  Offset 0, so that no window loses columns at the
    start of the sequence, and a range that ends 30 bases before the sequence does, so that none loses its last column either"""
    base = model_s("ord", (24, 0), (24, 0))
    md = dict(base)
    for tag in ("pm5", "pm3"):
        f = base[tag + "_f32"].copy()
        m = f[2:].view(np.float32).reshape(24, 84)
        m[:, 20:] += (np.float32(8192.0) * np.where(np.arange(24) % 2 == 0, 1, -1).astype(np.float32))[:, None]
        md[tag + "_f32"] = f
    out = []
    for k in range(2):
        rng = _rng(f"s/order/{k}")
        out.append(_case("s", "order", f"w{k}", _codes("s", rng, _bases(rng, 1500)), 0, 1470, md, "ord"))
    return out


def _branch():
    out = []
    n = 400
    rng = _rng("h/branch")
    b = _bases(rng, n)
    b[[100, 101, 250]] = 4
    codes = _codes("h", rng, b)
    for reach in (0, 1, 20):
        md = model_h("m0", pmB=(12, 8, 1), maxb3d=reach)
        out.append(_case("h", "branch", f"reach{reach}", codes, 0, n, md, f"m0/pmB{reach}" if reach != 20 else "m0/pmB"))
        out.append(_case("h", "branch", f"reach{reach}_sub", codes, 30, n - 30, md, f"m0/pmB{reach}" if reach != 20 else "m0/pmB"))
    return out


@functools.lru_cache(maxsize=None)
def cases(kind):
    out = _length(kind) + _range(kind) + _bad(kind) + _mode(kind) + _shape(kind)
    out += _phase() + _stop() + _branch() if kind == "h" else _order()
    assert len({c["name"] for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases(name[0]) if c["name"] == name)


# pairs of recipes one step apart: their outputs must differ (tests/test_signal_cases.py)
NEIGHBOURS = [("s/bad/single255", "s/bad/single256"), ("s/bad/single256", "s/bad/single257"), ("s/bad/none", "s/bad/single256"),
              ("s/bad/block4095", "s/bad/block4096"), ("s/range/left0", "s/range/left1"), ("s/range/left22", "s/range/left23"),
              ("s/range/left23", "s/range/left24"), ("s/range/right299", "s/range/right300"), ("s/range/right298", "s/range/right299"),
              ("s/range/right275", "s/range/right277"), ("s/mode/any0_ori0", "s/mode/any1_ori0"), ("s/mode/any1_ori0", "s/mode/any2_ori0"),
              ("s/mode/any2_ori0", "s/mode/any3_ori0"), ("s/mode/any0_ori0", "s/mode/any0_ori1"), ("s/mode/any2_ori0", "s/mode/any2_ori1"),
              ("h/bad/single255", "h/bad/single256"), ("h/bad/single256", "h/bad/single257"), ("h/range/left0", "h/range/left1"),
              ("h/range/left10", "h/range/left11"), ("h/range/left11", "h/range/left12"), ("h/range/right299", "h/range/right300"),
              ("h/range/right279", "h/range/right281"), ("h/mode/any0", "h/mode/any1"), ("h/mode/any1", "h/mode/any2"),
              ("h/mode/any2", "h/mode/any3"), ("h/mode/any0", "h/mode/dvsp_off"), ("h/mode/any0", "h/mode/no_pmI_pmT"),
              ("h/mode/any0", "h/mode/pmB"), ("h/mode/any0", "h/mode/no_pot"), ("h/phase/gt_at_left_any0", "h/phase/gt_at_left1_any0"),
              ("h/phase/gt_at_left_any0", "h/phase/gt_cut_any0"), ("h/phase/gt_right12_any0", "h/phase/gt_right13_any0"),
              ("h/phase/gt_right13_any0", "h/phase/gt_right14_any0"), ("h/phase/words_any0", "h/phase/words_any2"),
              ("h/stop/right95_stop-1", "h/stop/right95_stop0"), ("h/stop/right95_stop2", "h/stop/right95_stop3"),
              ("h/stop/right119_stop-1", "h/stop/right119_stop0"), ("h/stop/right118_stop0", "h/stop/right118_stop1"), ("h/stop/six0", "h/stop/six1"),
              ("h/stop/six1", "h/stop/six2"), ("h/branch/reach0", "h/branch/reach1"), ("h/branch/reach1", "h/branch/reach20")]


# ---- the oracle's arrays ----------------------------------------------------------------------------------------------------------------
_CACHE = {}


def expected(c, full=False):
    """kind s: sig5, sig3, cano5, cano3, dinc (b_len + 1 cells) and `mask`, the cells whose signals were evaluated (all of them
    unless the case has spans and full is False).  kind h: the seven SGPT6 arrays and dinc (b_len + 3 cells)"""
    key = (c["name"], bool(full and c["spans"]))
    if key in _CACHE:
        return _CACHE[key]
    if c["kind"] == "s":
        md = signals.model_of(c["model"])
        b, lf, rt = c["codes"], c["left"], c["right"]
        d5, d3, c5, c3 = signals.classes(b, lf, rt, md["any"], md["both_ori"])
        mask = np.ones(b.size + 1, dtype=bool)
        if c["spans"] and not full:
            s5 = np.zeros(b.size + 1, dtype=np.int16); s3 = np.zeros(b.size + 1, dtype=np.int16)
            mask[lf:rt] = False
            for lo, hi in c["spans"]:
                a5, a3 = signals.splice_signals(md, b, lf, rt, lo, hi)
                s5[lo:hi] = a5[lo:hi]; s3[lo:hi] = a3[lo:hi]
                mask[max(lo, lf):min(hi, rt)] = True
        else:
            s5, s3 = signals.splice_signals(md, b, lf, rt)
        out = dict(sig5=s5, sig3=s3, cano5=c5, cano3=c3, dinc=((d5 << 4) | d3).astype(np.uint8), mask=mask)
    else:
        md = signals_h.model_of(c["model"])
        b_len = c["codes"].size - 1
        out = signals_h.splice_signals_h(md, c["codes"], b_len, c["left"], c["right"])
        d5, d3, _, _ = signals_h.classes(c["codes"][:b_len], c["left"], c["right"], md["any"])
        out["dinc"] = ((d5 << 4) | d3).astype(np.uint8)
    _CACHE[key] = out
    return out


# ---- the scan once more, term by term: what a different order of the additions gives ---------------------------------------------------
def scan_terms(pm, x, pos):
    """the addends of oracle.signals.scan (order 2) in the order it adds them, or None where it returns the floor"""
    ln = x.size
    n = pos - pm.offset
    c0 = 0
    if n < 0:
        c0, n = -n, 0
    q = 1 if (pos - pm.offset) + pm.cols >= ln else 0
    last = min(n + (pm.cols - c0), ln - 2)
    terms, first, col = [], True, c0
    for s in range(n, last):
        row = pm.mtx[col * pm.rows:(col + 1) * pm.rows]
        i0, i1, i2 = int(x[s]), int(x[s + 1]), int(x[s + 2])
        if max(i0, i1, i2) > 3:
            return None
        if first:
            terms += [row[i0], row[4 * i0 + i1 + 4]]
        terms.append(row[16 * i0 + 4 * i1 + i2 + 20])
        first = False
        col += 1
    return None if q else terms


def sig5_with_order(c, reverse):
    """sig5 of a kind-s case with the columns summed first to last (the oracle's own values) or last to first"""
    md = signals.model_of(c["model"])
    x = signals.RED_STRICT[c["codes"]]
    want = expected(c)
    out = want["sig5"].copy()
    d5 = want["dinc"] >> 4
    for pos in np.flatnonzero(want["mask"]):
        if not c["left"] <= pos < c["right"]:
            continue
        t = scan_terms(md["pm5"], x, int(pos))
        if t is None:
            continue
        fit = np.float32(0)
        for v in (t[::-1] if reverse else t):
            fit = np.float32(fit + v)
        out[pos] = int(np.float32(md["fs"] * np.float32(fit + md["pm5"].tonic))) + int(md["tab"][d5[pos]])
    return out
