"""spdp_ladder_plan / spdp_ladder_postwork (spaln_amd/csrc/spdp_ladder.h: the linear-space ladder, stated once for both
query kinds) against the oracle's two separate restatements of lspS_ng / lspH_ng and mimd_postwork / rcsv_postwork
(oracle/host_logic.py, oracle/host_logic_h.py), whose engine calls are replaced by recorders.  Host-only entries: runs
without a GPU."""
import ctypes as C
import itertools
import math
import types

import numpy as np
import pytest

from oracle import host_logic, host_logic_h, oracle
from spaln_amd import abi, defaults, engine

END = abi.END_OF_ULK
EMPTY, ONE_SEQ, DIAGONAL, TRACEBACK, LINEAR = range(5)
MODES = (1, 2, 0)                                   # SpdpScoring.scalar_engines: -A0, -A1, SIMD
SIMD_OF = {1: 0, 2: 1, 0: 2}                        # -> the oracle's simd = algmode.alg & 3
VMF = (64 << 10, 1 << 20, 4 << 20, defaults.MAX_VMF_SPACE)
_DUMMY = C.create_string_buffer(8)                  # non-null intpen / cano5 / dinc: never read, the engines are recorders


class LadderPlan(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("kind", "n_imd", "imd_intvl", "recursive")]


class LadderStep(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("kind", "a_left", "a_right", "b_left", "b_right", "b_exgl")] + [("w", abi.Window)]


def _side(unit):
    """the oracle module, its problem / scoring types and its band for a row unit"""
    if unit == 1:
        return host_logic, abi.Problem, abi.Scoring, oracle.stripe
    return host_logic_h, abi.ProblemH, abi.ScoringH, oracle.stripe31


def _problem(unit, rng4, a_len, b_len):
    p = _side(unit)[1]()
    p.a_left, p.a_right, p.b_left, p.b_right = rng4
    p.a_len, p.b_len = a_len, b_len
    p.cano5 = p.dinc = C.addressof(_DUMMY)
    return p


# ---- the plan ---------------------------------------------------------------------------------------------------
class _PlanOracle:
    """lsp / lsp_h with every engine call, both post-works and math.pow recorded instead of run"""

    def __init__(self, unit, monkeypatch):
        self.mod = mod = _side(unit)[0]
        self.ev = []
        sfx = "" if unit == 1 else "_h"
        note = self.ev.append
        monkeypatch.setattr(mod, "trcbk" + sfx, lambda *a, **k: note(("trcbk",)) or 0)
        monkeypatch.setattr(mod, "diagonal" + sfx, lambda *a, **k: note(("diagonal",)) or 0)
        monkeypatch.setattr(mod, "mimd" + sfx, lambda *a, **k: note(("mimd",)))
        monkeypatch.setattr(mod, "rcsv" + sfx, lambda *a, **k: note(("rcsv",)))
        monkeypatch.setattr(mod, "math", types.SimpleNamespace(pow=lambda x, y: note(("pow", math.pow(x, y))) or math.pow(x, y)))

        def udh(sc, p, n_im, *rest):                # a score above NEVSEL and a crossed row: the post-work is entered
            note(("udh", n_im, rest[0] if len(rest) == 2 else None))
            out = (1, [[0] * 10] * (n_im + 1), (p.a_left, p.a_right, p.b_left, p.b_right))
            return out + (0,) if len(rest) == 2 else out
        for f in ("wip_udh", "exact_udh", "scalar_udh"):
            monkeypatch.setattr(oracle, f + sfx, udh)

    def __call__(self, sc, p, w, simd):
        """(kind, n_imd, imd_intvl or None, recursive, pow value or None)"""
        del self.ev[:]
        rec = []
        (self.mod.lsp if self.mod is host_logic else self.mod.lsp_h)(sc, p, w, rec, simd)
        names = [e[0] for e in self.ev]
        pw = next((e[1] for e in self.ev if e[0] == "pow"), None)
        if "udh" in names:
            u = self.ev[names.index("udh")]
            return LINEAR, u[1], u[2], int("rcsv" in names), pw
        kind = TRACEBACK if "trcbk" in names else DIAGONAL if "diagonal" in names else ONE_SEQ if rec else EMPTY
        return kind, 0, None, 0, pw


def _plan_points(unit):
    """(m, n, left ends, sh, max_vmf_space, ubh, recursive, mode, noll)"""
    rng = np.random.default_rng(7100 + unit)
    ms = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 257, 1000, 2000, 5000)
    ds = (0, 1, 3, 7, 8, 15, 16, 17)
    far = (200, 1000, 2500, 3000, 5000, 20000, 40000, 45000, 60000)
    nolls = (2, 3) if unit == 1 else (2,)
    grid = []
    for m in ms:
        ns = sorted({x for d in ds for b in {m, unit * m} for x in (b - d, b + d) if x >= 0} | set(far))
        # the full cross of the rows below has 1 to 3 x 10^5 points per unit: every 5th of it, the scoring fields innermost, so
        # that each (m, n, sh, mode) keeps several settings of the others and these rotate from one to the next
        grid += itertools.product([m], ns, [(0, 0)], (-25, 0, 10, 100), MODES, VMF, (0, 1, 3, 7), (0, 1), nolls)
    for m, n, left, sh, mode, vmf, ubh, rcs, noll in grid[::5]:
        yield m, n, left, sh, vmf, ubh, rcs, mode, noll
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    for k in range(20000):
        fam = k % 10
        vmf, ubh, rcs, sh = pick(VMF), pick((0, 0, 1, 3, 7)), int(rng.integers(4) == 0), pick((-25, 0, 10, 100, int(rng.integers(0, 300))))
        if fam == 0:                                # ends of the ladder: nothing, one sequence only, one diagonal
            m = int(rng.integers(0, 40)) * int(rng.integers(3) > 0)
            n = pick((0, 0, unit * m, int(rng.integers(0, 200))))
            sh = pick((0, 0, sh))
        elif fam == 1:                              # automatic n_imd of 0: too few rows for an intermediate one
            m, vmf, ubh, rcs = int(rng.integers(11, 16)), pick(VMF[:2]), 0, 0
            n = int(rng.integers(vmf // (2 * m), vmf // m))
        elif fam == 2:                              # forced n_imd that divides m: one intermediate row fewer
            ubh, rcs, vmf = pick((3, 7, 7, 7)), 0, pick(VMF[:3])
            m = ubh * int(rng.integers(2, ubh + 1))
            n = int(rng.integers(vmf // (2 * m), vmf // m))
        else:
            m = int(math.exp(rng.uniform(0, math.log(6000))))
            n = pick((unit * m + int(rng.integers(-40, 41)), int(math.exp(rng.uniform(0, math.log(60000))))))
        left = (int(rng.integers(0, 3000)), int(rng.integers(0, 9000))) if rng.integers(2) else (0, 0)
        yield m, max(n, 0), left, sh, vmf, ubh, rcs, pick(MODES), pick((2, 3))


@pytest.mark.parametrize("unit", [1, 3])
def test_plan_equals_restatement(unit, monkeypatch):
    lib = engine.load_library()
    orc = _PlanOracle(unit, monkeypatch)
    _, _, Scoring, band = _side(unit)
    lib_band = lib.spdp_stripe if unit == 1 else lib.spdp_stripe31
    kinds = [0] * 5
    forced = reduced = none_left = 0
    out, w2 = LadderPlan(), abi.Window()
    for m, n, (al, bl), sh, vmf, ubh, rcs, mode, noll in _plan_points(unit):
        rng4 = (al, al + m, bl, bl + n)
        p = _problem(unit, rng4, al + m, bl + n)
        sc = Scoring()
        sc.sh, sc.max_vmf_space, sc.ubh, sc.recursive, sc.scalar_engines, sc.noll = sh, vmf, ubh, rcs, mode, noll
        sc.intpen = C.addressof(_DUMMY)
        w = band(p, sh)
        lib_band(C.byref(p), sh, C.byref(w2))
        assert (w2.lw, w2.up, w2.width) == (w.lw, w.up, w.width), (rng4, sh)
        kind, n_imd, intvl, recursive, pw = orc(sc, p, w, SIMD_OF[mode])
        assert lib.spdp_ladder_plan(unit, (C.c_int32 * 4)(*rng4), C.byref(w), mode, rcs, ubh, vmf, noll, C.byref(out)) == 0
        where = (rng4, sh, vmf, ubh, rcs, mode, noll)
        assert (out.kind, out.n_imd, out.recursive) == (kind, n_imd, recursive), where
        if intvl is not None:                       # (the oracle hands the interval to the -A0 engine only)
            assert out.imd_intvl == intvl, where
        # what the oracle's own answers covered
        kinds[kind] += 1
        asked = ubh if ubh else min(int(pw + 0.5) - 1, m // 16) if pw is not None else None
        forced += kind == LINEAR and recursive and not rcs and pw is not None
        reduced += kind == LINEAR and not recursive and pw is not None and n_imd < asked
        none_left += kind == TRACEBACK and pw is not None
    assert min(kinds) >= 200, kinds
    assert min(forced, reduced, none_left) >= 20, (forced, reduced, none_left)


# ---- the post-work -------------------------------------------------------------------------------------------------
def _block(rng, unit, recursive):
    """a written-back range inside its parent and (n_imd + 1) cpos rows as the engines leave them; what was tripped"""
    n_imd = 1 if recursive else int(rng.integers(1, 8))
    cpos = np.full((n_imd + 1, 10), END, dtype=np.int32)
    lo = 0 if recursive else int(rng.integers(0, n_imd))                # rows below lo and from hi on are unused
    hi = int(rng.integers(lo + 1, n_imd + 1))
    al, bl = int(rng.integers(0, 50)), int(rng.integers(0, 150))
    ms = np.sort(rng.choice(np.arange(al + 1, al + 400), hi - lo, replace=False))
    ar = int(ms[-1]) + int(rng.integers(1, 50))
    x = bl
    for i, m in zip(range(lo, hi), ms):
        x += int(rng.integers(0, 60)) * unit
        pos = x + np.sort(rng.integers(0, 30, int(rng.integers(0, 5))))  # 0 .. 4 positions behind the left n, then the terminator
        cpos[i, :3] = m, int(rng.integers(0, 3)), x
        cpos[i, 3:3 + len(pos)] = pos
        x = int(pos[-1]) if len(pos) else x
    br = x + int(rng.integers(0, 60))
    for i in range(n_imd + 1):                                          # diagonal bounds: every row, the extra one included
        cpos[i, 8] = int(rng.integers(-300, 100))
        cpos[i, 9] = cpos[i, 8] + int(rng.integers(0, 80))
    a_len, b_len = ar + int(rng.integers(0, 5)), br + int(rng.integers(0, 5))
    trip = (None, None, "gt", "neg", "beyond", "unused0")[int(rng.integers(6))]
    t = int(rng.integers(lo, hi))
    if trip == "gt": cpos[t, 2] = br + 1 + int(rng.integers(0, 9))
    elif trip == "neg": cpos[t, 2] = -1 - int(rng.integers(0, 9))
    elif trip == "beyond":
        if rng.integers(2): a_len = ar - 1
        else: b_len = br - 1
    elif trip == "unused0" and recursive: cpos[0, 0] = END            # crosses nothing (reached by a local call only)
    return (al, ar, bl, br), a_len, b_len, n_imd, cpos, trip, hi - lo


def _oracle_postwork(unit, monkeypatch):
    mod, _, Scoring, _ = _side(unit)
    sfx = "" if unit == 1 else "_h"
    calls = []

    def call(kind):
        def f(sc, p, w, rec, simd=2):
            assert (p.a_exgl, p.a_exgr, p.b_exgr) == (0, 0, 0)
            calls.append((kind, p.a_left, p.a_right, p.b_left, p.b_right, p.b_exgl, w.lw, w.up, w.width))
            return 0
        return f
    monkeypatch.setattr(mod, "trcbk" + sfx, call(1))
    monkeypatch.setattr(mod, "lsp" + sfx, call(2))

    def run(recursive, simd, local, sh, rng4, a_len, b_len, n_imd, cpos):
        del calls[:]
        rec = []
        sc = Scoring()
        sc.sh, sc.local = sh, local
        cur = _problem(unit, rng4, a_len, b_len)
        rows = cpos.tolist()
        if recursive: getattr(mod, "rcsv" + sfx)(sc, cur, rows, rec, simd)
        else: getattr(mod, "mimd" + sfx)(sc, cur, rows, n_imd, rec, simd)
        return rec, list(calls)
    return run


@pytest.mark.parametrize("unit", [1, 3])
def test_postwork_equals_restatement(unit, monkeypatch):
    lib = engine.load_library()
    orc = _oracle_postwork(unit, monkeypatch)
    rng = np.random.default_rng(7200 + unit)
    steps = (LadderStep * 64)()
    seen = dict(gt=0, neg=0, beyond=0, final=0)
    for recursive, a0 in itertools.product((0, 1), (1, 0)):
        for _ in range(5000):
            rng4, a_len, b_len, n_imd, cpos, trip, used = _block(rng, unit, recursive)
            sh = int(rng.choice((-25, 0, 10, 100)))
            local = int(rng.integers(2)) if unit == 1 else 0            # (protein: the ladder has no local branch here)
            rec, calls = orc(recursive, 0 if a0 else 2, local, sh, rng4, a_len, b_len, n_imd, cpos)
            n = lib.spdp_ladder_postwork(unit, recursive, a0, local, sh, (C.c_int32 * 4)(*rng4), a_len, b_len, n_imd,
                                         cpos.ctypes.data_as(C.c_void_p), steps, len(steps))
            assert 0 <= n <= len(steps)
            got = [steps[i] for i in range(n)]
            where = (recursive, a0, local, sh, rng4, a_len, b_len, n_imd, cpos.tolist())
            assert [(s.a_left, s.b_left) for s in got if s.kind == 0] == rec, where
            assert [(s.kind, s.a_left, s.a_right, s.b_left, s.b_right, s.b_exgl, s.w.lw, s.w.up, s.w.width)
                    for s in got if s.kind != 0] == calls, where
            if not recursive:                       # what the oracle's own walks covered
                final = bool(calls) and calls[-1][1] == rng4[0] and calls[-1][3] == rng4[2]
                seen["final"] += final
                if trip in seen and len(calls) - final < used:
                    seen[trip] += 1
    need = ("gt", "neg", "final") + (("beyond",) if unit == 3 else ())
    assert all(seen[k] >= 50 for k in need), seen
