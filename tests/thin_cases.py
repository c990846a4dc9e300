"""Single lspB_ng requests for the thin form of the unspliced sweep (spdp_b_sweep_thin), built by named recipe; shared by
tests/test_thin_cases.py (the generator against the restatement, CPU), tests/test_b_thin_host.py (the host emulation of the
sweeps, CPU) and tests/test_gpu_thin_sweep.py (spdp_lsp_b on the device).

A recipe is one call: build(name) -> (Scoring, UnsplicedParams, ProblemSet, tags), tags[i] a dict about problem i.  Every request
is a sub-range of a longer pair with 5 .. 40 residues of unrelated sequence on each side of the range (none on a side a recipe
wants at the very end of its sequence), so that a wrong offset or a column read one too far changes the result.  Everything is
a function of the recipe's name.

Two alphabets: the twenty amino acids under the program's matrix (defaults.scoring_b), and four letters (codes 1 .. 4) under
match 4 / mismatch -2 with gop -4, gep -2, lgep -1: few distinct values, all even but the long extension, so that h, f and e1
tie in many cells.  The local recipes put diagonal 40 / off-diagonal -30 on either alphabet.

Groups (GROUPS): grid, ends, band, long, local, waves, rounds.  ends/*/steep_top is the recipe a surviving variant of the
kernel asked for (lane 0 taking its own F for the row above): see _steep_top.  Only the recipes whose name holds "without_cells" contain
requests that lspB_ng serves without a DP cell."""
import functools
import itertools
import zlib

import numpy as np

from spaln_amd import abi, defaults

EXGS = list(itertools.product((0, 1), repeat=4))        # (a_exgl, a_exgr, b_exgl, b_exgr)
GRID_ROWS = (1, 2, 3, 15, 16, 17)
GRID_COLS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 49, 64)
BAND_SH = (100, 5, 2, 1, -10)
BAND_SHAPES = ((16, 60), (16, 2), (3, 40))
WAVE_SIZES = (1, 2, 3, 4, 5, 7, 8, 9)
UNLIKE = ((1, 1), (16, 60), (3, 17), (16, 1), (7, 33))  # the members of the waves of 4 and 5


# ---- bundles ----------------------------------------------------------------------------------------------------------------------
def lgop_at(gop, gep, lgep, k1):
    """the long-gap opening price that makes both gap prices meet at length k1"""
    return gop + k1 * (gep - lgep)


def bundle(alpha, noll=2, local=0, sh=100, k1=None):
    """alpha "aa": the protein bundle; "nt": four letters with few distinct values.  local: the 40 / -30 matrix"""
    if alpha == "aa":
        k1 = defaults.B_K1 if k1 is None else k1
        kw = dict(noll=noll, local=local, sh=sh, codonk1=k1, lgop=lgop_at(defaults.B_GOP, defaults.B_GEP, defaults.B_LGEP, k1))
        if local:
            m = np.full((23, 23), -30, dtype=np.int32)
            m[np.arange(23), np.arange(23)] = 40
            kw["mtx"] = m
        return defaults.scoring_b(**kw)
    k1 = 3 if k1 is None else k1
    m = np.zeros((5, 5), dtype=np.int32)
    m[1:, 1:] = -30 if local else -2
    m[np.arange(1, 5), np.arange(1, 5)] = 40 if local else 4
    gop, gep, lgep = (-40, -20, -10) if local else (-4, -2, -1)
    return abi.make_scoring(mtx=m, mtx_dim=5, gop=gop, gep=gep, lgop=lgop_at(gop, gep, lgep, k1), lgep=lgep, noll=noll, spj=0, local=local,
                            sh=sh, scalar_engines=1, codonk1=k1)


def letters(alpha):
    return (3, 20) if alpha == "aa" else (1, 4)          # first code, number of codes


# ---- arithmetic on a problem (tests/test_thin_cases.py holds it to the restatement's stripe) ---------------------------------------
def window(p, sh):
    """(lw, up) of stripe() on the problem's ranges"""
    rows, cols = p.a_right - p.a_left, p.b_right - p.b_left
    if sh < 0:
        sh = -sh * min(rows, cols) // 100
    up, lw = p.b_right - p.a_right, p.b_left - p.a_left
    if up < lw:
        up, lw = lw, up
    return max(lw - sh, p.b_left - p.a_right), min(up + sh, p.b_right - p.a_left)


def geometry(p, sh):
    """what the thin sweep derives from a request: rows, cols, steps (anti-diagonals of its one tile), top_hi (the last column
    offset the top boundary reaches), host (lspB_ng serves it without a DP cell)"""
    lw, up = window(p, sh)
    rows, cols = p.a_right - p.a_left, p.b_right - p.b_left
    nlo = max(p.a_left + lw, p.b_left) + 1
    nhi = min(p.a_right + up, p.b_right)
    steps = 0 if nhi < nlo else (nhi - nlo + 1) + rows - 1
    return dict(rows=rows, cols=cols, lw=lw, up=up, steps=steps, top_hi=min(cols, up - (p.b_left - p.a_left)),
                host=(rows == 0 or cols == 0 or lw == up))


def tiled_need(p, sh):
    """bytes of the tiled sweep's trace store for the request (spdp_trace_bytes_b)"""
    g = geometry(p, sh)
    if g["host"]:
        return 0
    stride = (min(g["cols"], g["up"] - g["lw"] + 64) + 63 + 3) & ~3
    return (g["rows"] + 63) // 64 * stride * 64


def thin_need(p, sh):
    return ((geometry(p, sh)["steps"] + 3) & ~3) * 16


def predict(sc, up, ps, thin_on=True):
    """the counters spdp_lsp_b reports for the call, from arithmetic on the requests alone"""
    out = dict(thin_requests=0, wide_requests=0, host_requests=0, requests_not_computed=0, requests_le16_rows=0)
    budget = up.max_trace_bytes or (4 << 30)
    for p in ps.items:
        g = geometry(p, sc.sh)
        if g["host"]:
            out["host_requests"] += 1
            continue
        thin = thin_on and g["rows"] <= 16
        out["requests_le16_rows"] += g["rows"] <= 16
        if (thin_need(p, sc.sh) if thin else tiled_need(p, sc.sh)) > budget:
            out["requests_not_computed"] += 1
        else:
            out["thin_requests" if thin else "wide_requests"] += 1
    return out


# ---- sequences --------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _random(rng, alpha, n):
    lo, k = letters(alpha)
    return rng.integers(lo, lo + k, size=int(n)).astype(np.uint8)


def _mutate(rng, alpha, s, rate):
    s = s.copy()
    hit = rng.random(s.size) < rate
    s[hit] = _random(rng, alpha, int(hit.sum()))
    return s


def _cores(rng, alpha, rows, cols, kind):
    """two cores of the given lengths.  "rel": b is a with substitutions, cut or continued at a random place to its length;
    "rnd": unrelated"""
    a = _random(rng, alpha, rows)
    if kind == "rnd" or rows == 0 or cols == 0:
        return a, _random(rng, alpha, cols)
    b = _mutate(rng, alpha, a, 0.15)
    if cols < rows:
        at = int(rng.integers(0, cols + 1))
        b = np.concatenate([b[:at], b[at + rows - cols:]])
    elif cols > rows:
        at = int(rng.integers(0, rows + 1))
        b = np.concatenate([b[:at], _random(rng, alpha, cols - rows), b[at:]])
    return a, b


class Builder:
    def __init__(self, name, alpha):
        self.name, self.alpha, self.rng = name, alpha, _rng(name)
        self.ps, self.tags = abi.ProblemSet(), []

    def add(self, ca, cb, exg, at_end=(0, 0, 0, 0), **tag):
        """the cores as a sub-range of a longer pair; at_end = (a left, a right, b left, b right): 1 puts the range at that
        very end of its sequence, else 5 .. 40 unrelated residues lie beyond it"""
        fl = [0 if e else int(self.rng.integers(5, 41)) for e in at_end]
        a = np.concatenate([_random(self.rng, self.alpha, fl[0]), ca, _random(self.rng, self.alpha, fl[1])])
        b = np.concatenate([_random(self.rng, self.alpha, fl[2]), cb, _random(self.rng, self.alpha, fl[3])])
        self.ps.add(a, b, None, None, a_left=fl[0], a_right=fl[0] + ca.size, b_left=fl[2], b_right=fl[2] + cb.size, exg=exg)
        self.tags.append(dict(rows=int(ca.size), cols=int(cb.size), exg=tuple(exg), at_end=tuple(int(bool(e)) for e in at_end), **tag))

    def pair(self, rows, cols, kind, exg, at_end=(0, 0, 0, 0), **tag):
        ca, cb = _cores(self.rng, self.alpha, rows, cols, kind)
        self.add(ca, cb, exg, at_end, kind=kind, **tag)


# ---- recipes ----------------------------------------------------------------------------------------------------------------------
_RECIPES = {}


def _recipe(name):
    def deco(fn):
        _RECIPES[name] = fn
        return fn
    return deco


def _both_alphabets(group, noll_of=dict(aa=2, nt=3)):
    return [(f"{group}/{alpha}", alpha, noll_of[alpha]) for alpha in ("aa", "nt")]


def _grid(name, alpha, noll):
    def make():
        bd = Builder(name, alpha)
        shapes = [(r, c) for r in GRID_ROWS for c in GRID_COLS] + [(c, r) for r in GRID_ROWS for c in GRID_COLS if c <= 16]
        j = 0
        for r, c in shapes:
            for kind in ("rel", "rel", "rnd"):
                bd.pair(r, c, kind, EXGS[j % 16])
                j += 1
        return bundle(alpha, noll=noll), abi.UnsplicedParams(1.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def _ends(name, alpha, noll, tgapf):
    def make():
        bd = Builder(name, alpha)
        for exg in EXGS:
            for at_end in EXGS:
                rows = int(bd.rng.integers(1, 17))
                cols = int(bd.rng.choice([1, 2, 3, rows, rows + 1, int(bd.rng.integers(1, 41)), int(bd.rng.integers(1, 41))]))
                bd.pair(rows, cols, "rel" if bd.rng.random() < 0.8 else "rnd", exg, at_end)
        return bundle(alpha, noll=noll), abi.UnsplicedParams(tgapf, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def harsh(sc, mismatch):
    """the bundle with every mismatch at `mismatch`"""
    d = sc.mtx_dim
    for x in range(1, d):
        for y in range(1, d):
            if x != y:
                sc.mtx[x * d + y] = mismatch
    return sc


def _steep_top(name, alpha, noll):
    """tgapf = 2 at a_left == 0 without a_exgl: the top boundary falls by twice the gap extension per column, so F of the first
    row, continued from the left, would beat the one opened from the boundary -- lane 0 of the thin sweep must read the row above
    it as black, not as its own last cell.  Mismatches cost more than any gap and the pairs are unrelated, so that the
    vertical states decide"""
    def make():
        bd = Builder(name, alpha)
        for j in range(256):
            rows, cols = int(bd.rng.integers(1, 17)), int(bd.rng.integers(1, 41))
            x, y, z = j & 1, (j >> 1) & 1, (j >> 2) & 1
            bd.pair(rows, cols, "rnd", (0, x, 0, y), (1, x, 1 - z, y))
        return harsh(bundle(alpha, noll=noll), -400 if alpha == "aa" else -40), abi.UnsplicedParams(2.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def _band(name, alpha, noll, sh):
    def make():
        bd = Builder(name, alpha)
        for r, c in BAND_SHAPES:
            for j, exg in enumerate(EXGS):
                for kind in ("rel", "rnd"):
                    # half of them at the right ends of both sequences: the last-row / last-column passes run inside the band
                    bd.pair(r, c, kind, exg, (0, j & 1, 0, j & 1))
                # one or two rows / columns off the named shape: the band's corner falls elsewhere
                bd.pair(max(1, r - 1 - (j & 1)), c + 1 + (j >> 3), "rel", exg)
        return bundle(alpha, noll=noll, sh=sh), abi.UnsplicedParams(0.5 if alpha == "nt" else 1.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def _long(name, alpha, noll, k1):
    def make():
        bd = Builder(name, alpha)
        j = 0
        for d in range(1, 13):
            for where in ("start", "mid", "end"):
                for rows in (16, 13):
                    a = _random(bd.rng, alpha, rows)
                    m = _mutate(bd.rng, alpha, a, 0.1)
                    # a deletion: d residues of a face no column (the boundary column or F / F2 carries the gap)
                    if d < rows:
                        at = 0 if where == "start" else (rows - d if where == "end" else int(bd.rng.integers(1, max(2, rows - d))))
                        bd.add(a, np.concatenate([m[:at], m[at + d:]]), EXGS[j % 16] if j % 3 == 0 else (0, 0, 0, 0), indel=-d, where=where)
                        j += 1
                    # an insertion: d columns face no residue of a (the boundary row or e1 / e2 carries the gap)
                    rr = rows - 9
                    at = 0 if where == "start" else (rr if where == "end" else int(bd.rng.integers(1, rr)))
                    bd.add(a[:rr], np.concatenate([m[:at], _random(bd.rng, alpha, d), m[at:rr]]), EXGS[j % 16] if j % 3 == 0 else (0, 0, 0, 0),
                           indel=d, where=where)
                    j += 1
        return bundle(alpha, noll=noll, k1=k1), abi.UnsplicedParams(1.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def _disjoint(bd, rows, cols):
    """two cores without a letter in common: nothing scores above zero"""
    lo, k = letters(bd.alpha)
    half = k // 2
    return (bd.rng.integers(lo, lo + half, size=rows).astype(np.uint8), bd.rng.integers(lo + half, lo + k, size=cols).astype(np.uint8))


def _local(name, alpha, noll):
    def make():
        bd = Builder(name, alpha)
        lo, k = letters(alpha)
        other = lambda n: np.full(n, lo + k - 1, dtype=np.uint8)        # a letter the motifs below do not use
        for j in range(60):                                              # local at all four ends: the optimum lies inside
            rows = int(bd.rng.integers(2, 17))
            core = _random(bd.rng, alpha, int(bd.rng.integers(2, rows + 1)))
            a = np.concatenate([_random(bd.rng, alpha, rows - core.size), core]) if j & 1 else np.concatenate([core, _random(bd.rng, alpha, rows - core.size)])
            b = np.concatenate([_random(bd.rng, alpha, int(bd.rng.integers(0, 20))), _mutate(bd.rng, alpha, core, 0.1),
                                _random(bd.rng, alpha, int(bd.rng.integers(0, 20)))])
            bd.add(a, b, (1, 1, 1, 1), part="inside")
        for j, exg in enumerate(e for e in EXGS if e != (1, 1, 1, 1)):   # local on one side, on neither, free ends that are not local
            for rep in range(3):
                rows = int(bd.rng.integers(1, 17))
                bd.pair(rows, int(bd.rng.integers(1, 50)), "rel", exg, (0, rep == 1, 0, rep == 2), part="one_side")
        for j in range(15):                                              # nothing positive
            ca, cb = _disjoint(bd, int(bd.rng.integers(1, 17)), int(bd.rng.integers(1, 40)))
            bd.add(ca, cb, (1, 1, 1, 1), part="empty")
        for j in range(12):                                              # equal maxima
            L = int(bd.rng.integers(2, 8))
            motif = bd.rng.integers(lo, lo + k - 1, size=L).astype(np.uint8)
            gap = other(int(bd.rng.integers(1, 4)))
            twice = np.concatenate([motif, gap, motif])
            bd.add(motif, twice, (1, 1, 1, 1), part="same_row")          # the motif's last row, at two columns
            bd.add(twice, motif, (1, 1, 1, 1), part="two_rows")          # two rows, one column
            bd.add(twice, np.concatenate([motif, other(gap.size + 4), motif]), (1, 1, 1, 1), part="two_rows")    # two rows, two columns
        return bundle(alpha, noll=noll, local=1), abi.UnsplicedParams(1.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def _waves(name, alpha, n, v):
    def make():
        bd = Builder(name, alpha)
        if n in (4, 5):
            # very unlike members in one wave; local and global ones side by side, each with flags of its own
            flags = [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 0, 0)]
            order = np.roll(np.arange(n), v)
            for i in order:
                r, c = UNLIKE[i]
                bd.pair(r, c, "rel", flags[(i + v) % n])
        else:
            for i in range(n):
                bd.pair(int(bd.rng.integers(1, 17)), int(bd.rng.integers(1, 65)), "rel", EXGS[int(bd.rng.integers(0, 16))])
        return bundle(alpha, noll=3 if alpha == "nt" else 2, local=1), abi.UnsplicedParams(1.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


def _mixed(name, alpha, tight):
    def make():
        bd = Builder(name.replace("_tight", ""), alpha)                 # the tight form: the same requests
        for j in range(90):                                              # thin and tiled requests interleaved
            if j % 3 == 1:
                bd.pair(int(bd.rng.integers(17, 71)), int(bd.rng.integers(1, 65)), "rel", EXGS[j % 16])
            else:
                bd.pair(int(bd.rng.integers(1, 17)), int(bd.rng.integers(1, 65)), "rel", EXGS[j % 16])
        sc = bundle(alpha, noll=3 if alpha == "nt" else 2)
        budget = max(tiled_need(p, sc.sh) for p in bd.ps.items) if tight else 0
        return sc, abi.UnsplicedParams(1.0, budget), bd.ps, bd.tags
    _RECIPES[name] = make


@_recipe("rounds/big")
def _big():
    """a few tiled requests of 200 x 200: what a later thin-only call finds in the pool"""
    bd = Builder("rounds/big", "aa")
    for j in range(3):
        bd.pair(200, 200, "rel", (0, 0, 0, 0))
    return bundle("aa"), abi.UnsplicedParams(1.0, 0), bd.ps, bd.tags


@_recipe("rounds/after_big")
def _after_big():
    bd = Builder("rounds/after_big", "aa")
    for j in range(64):
        bd.pair(int(bd.rng.integers(1, 17)), int(bd.rng.integers(1, 65)), "rel", EXGS[j % 16], (0, j % 5 == 0, 0, j % 7 == 0))
    return bundle("aa", sh=5), abi.UnsplicedParams(0.5, 0), bd.ps, bd.tags


def _without_cells(name, alpha):
    def make():
        bd = Builder(name, alpha)
        for j, exg in enumerate(EXGS):
            n = int(bd.rng.integers(1, 17))
            bd.pair(0, n, "rnd", exg, branch="no_rows")
            bd.pair(n, 0, "rnd", exg, branch="no_cols")
            bd.pair(0, 0, "rnd", exg, branch="neither")
            bd.pair(n, n, "rel", exg, branch="diagonal")                 # sh = 0 and a square range: one diagonal
            bd.pair(n, n + 1 + j % 3, "rel", exg, branch="sweep")        # sh = 0 off the square: a band as wide as the difference
        return bundle(alpha, noll=3 if alpha == "nt" else 2, sh=0), abi.UnsplicedParams(1.0, 0), bd.ps, bd.tags
    _RECIPES[name] = make


for _name, _alpha, _noll in _both_alphabets("grid"):
    _grid(_name, _alpha, _noll)
for _alpha, _noll in (("aa", 2), ("nt", 3)):
    for _t in (1.0, 0.5, 0.0):
        _ends(f"ends/{_alpha}/tgapf{_t}", _alpha, _noll, _t)
    for _n2 in (2, 3):
        _steep_top(f"ends/{_alpha}/steep_top/noll{_n2}", _alpha, _n2)
    for _sh in BAND_SH:
        _band(f"band/{_alpha}/sh{_sh}", _alpha, _noll, _sh)
    for _n2 in (2, 3):
        for _k1 in (3, 7):
            _long(f"long/{_alpha}/noll{_n2}/k{_k1}", _alpha, _n2, _k1)
    _local(f"local/{_alpha}", _alpha, _noll)
    for _n in WAVE_SIZES:
        for _v in range(3):
            _waves(f"waves/{_alpha}/n{_n}/v{_v}", _alpha, _n, _v)
    _mixed(f"rounds/{_alpha}/mixed", _alpha, False)
    _mixed(f"rounds/{_alpha}/mixed_tight", _alpha, True)
    _without_cells(f"rounds/{_alpha}/without_cells", _alpha)

GROUPS = ("grid", "ends", "band", "long", "local", "waves", "rounds")


def names(group=None):
    return [n for n in _RECIPES if group is None or n.split("/")[0] == group]


@functools.lru_cache(maxsize=None)
def build(name):
    """(Scoring, UnsplicedParams, ProblemSet, tags) of the recipe; built once, to be left unchanged"""
    return _RECIPES[name]()
