"""Which statements of the oracle's two rescoring walks (oracle/host_logic.py::skl_rng_s, oracle/host_logic_h.py::skl_rng_h) the
fixtures written by the reference execute.  A statement no fixture reaches is held by nothing: the oracle could be wrong there,
and so could the kernel that is compared with it.  Every statement must execute, except the ones marked `# unpinned: <key>` in
the oracle's source, with the reason per key in UNPINNED; their number may only shrink (tests/rescore_cases.py keeps its corner lists away from what is on it)."""
import inspect
import sys

from tests import spdg
from tests.conftest import golden_files
from oracle import host_logic, host_logic_h

# a statement no fixture reaches carries the comment `# unpinned: <key>` in the oracle's source, where an edit of the oracle moves
# it along with the statement; the keys and why nothing reaches them
UNPINNED = {
    "shared-n": "no list the reference's aligner leaves has its first two corners on one genomic position under b_exgl (it trims that gap)",
    "stop-gap": "no fixture ends in a gap behind its last intron in front of a stop codon",
    "gtgt": "no fixture has a GTGT....AGAG junction (both phase marks 2) whose phase -1 reading is tried",
}
MAX_UNPINNED_LINES = 16                                  # only shrinks (22 before h1_local_inner took the two end bonuses off and h1_suptcodon four)


def _codes(fn):
    """the code objects of a function and of the functions and classes written inside it"""
    out, todo = [], [fn.__code__]
    while todo:
        c = todo.pop()
        out.append(c)
        todo += [k for k in c.co_consts if inspect.iscode(k)]
    return out


def _statement_lines(fn):
    lines = set()
    for c in _codes(fn):
        lines |= {ln for _, _, ln in c.co_lines() if ln is not None and ln > c.co_firstlineno}
    src, first = inspect.getsourcelines(fn)
    text = {ln: src[ln - first].strip() for ln in lines}
    # lines that only continue a statement, close a bracket or hold a docstring are not statements of their own
    return {ln: t for ln, t in text.items() if t and not t.startswith(('"""', "#", ")", "]"))}


class _Tracer:
    def __init__(self, fns):
        self.codes = {c for fn in fns for c in _codes(fn)}
        self.hit = set()

    def __call__(self, frame, event, arg):
        if frame.f_code not in self.codes:
            return None
        if event == "line":
            self.hit.add((frame.f_code.co_filename, frame.f_lineno))
        return self

    def __enter__(self):
        sys.settrace(self)
        return self

    def __exit__(self, *exc):
        sys.settrace(None)


def _run_all_fixtures():
    from tests.test_oracle_cip import cip_problem
    from tests.test_oracle_h_golden import _rescore_kw
    n = 0
    for prefix in ("s1_", "c2_", "c5_", "o3_", "cp_"):
        for f in golden_files(prefix):
            fx = spdg.load(f)
            for alg in (0, 1, 2, 3):
                if f"rng_eij_A{alg}" not in fx:
                    continue
                sc = spdg.scoring(fx, nquant=(1 if alg == 3 else None))
                _, p = cip_problem(fx) if prefix == "cp_" else spdg.problem(fx)
                fs = fx[f"rng_fstat_A{alg}"]
                host_logic.skl_rng_s(sc, p, [int(x) for x in fx[f"aln_skl_A{alg}"]], codonk1=fx["prm"]["codonk1"],
                                     minl=fx["prm"]["minl"], jneibr=int(fs[6]), lsg=int(fs[7]))
                n += 1
    for f in golden_files("h1_") + golden_files("c1_"):
        name = f.split("/")[-1][:-5]
        if name == "h1_cut_right":
            continue                                    # undefined in the reference (tests/test_oracle_h_golden.py)
        fx = spdg.load(f)
        for alg in (0, 2, 3):
            if f"rng_eij_A{alg}" not in fx or (name == "h1_local_udh" and alg in (2, 3)):
                continue
            sc = spdg.scoring_h(fx, nquant=None if alg != 3 else 1)
            _, p = spdg.problem_h(fx)
            host_logic_h.skl_rng_h(sc, p, [int(x) for x in fx[f"aln_skl_A{alg}"]], **_rescore_kw(fx))
            n += 1
    return n


def test_every_statement_of_the_rescoring_walks_runs_on_a_fixture():
    fns = (host_logic.skl_rng_s, host_logic_h.skl_rng_h)
    with _Tracer(fns) as tr:
        n = _run_all_fixtures()
    assert n >= 150
    import re
    missed, stale, marked = [], [], 0
    for fn in fns:
        file = fn.__code__.co_filename
        src, first = inspect.getsourcelines(fn)
        for ln, text in sorted(_statement_lines(fn).items()):
            m = re.search(r"# unpinned: (\S+)", src[ln - first])
            assert m is None or m.group(1) in UNPINNED, (fn.__name__, ln, text)
            hit = (file, ln) in tr.hit
            marked += m is not None
            if not hit and m is None:
                missed.append((fn.__name__, ln, text))
            if hit and m is not None:
                stale.append((fn.__name__, ln, text))
    assert not missed, missed                            # a statement no fixture reaches, and no reason given
    assert not stale, stale                              # a marked statement that a fixture reaches by now: take the mark off
    assert 0 < marked <= MAX_UNPINNED_LINES
