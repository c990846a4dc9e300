"""Fixtures of the protein database search from the program itself: runs where oracle/_ref/spaln is built (oracle/ref_build) and
writes DATA only --
    tests/golden/aa_db_<set>.bka.gz        the index `spaln -W -KA -t1` wrote of the set's database
    tests/golden/aa_search_<set>.json.gz   the database sequences, the queries with their class, and per option set the records
                                           `spaln -Q7 -A0 -O4 [-O0] -t1 <options> -a<db> q.faa` printed (-A0: the scalar
                                           engine of Aln2b1, the one the library's unspliced aligner reproduces)

    python tests/golden/make_aa_search_goldens.py [--sets a b]

The script stops with a message unless the reference alone shows what the fixtures are there to pin (see `require`)."""
import argparse
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "spaln")
ENV = dict(os.environ, ALN_TAB=os.path.join(ROOT, "oracle", "_ref", "table"))
AA = "ARNDCQEGHILKMFPSTWYV"

OPTION_SETS = {"default": [], "M4": ["-M4"], "M4_pw": ["-M4", "-pw"], "LS_M2_pw": ["-LS", "-M2", "-pw"]}
# -H<thr>: alprm.thr, Vthr = thr x 10 (src/aln2.cc:105).  Set b holds pairs whose engine score and fstat.val lie on different sides of these
# two (q1 x p30: 1667 / 1565; q8 x p31: 2688 / 2722): blkaln holds Vthr against Gsinfo::scr, which skl_rngB_ng has set to fstat.val by then
# (src/spaln.cc:684, 915)
H_SETS = {"H160": ["-H160"], "H270": ["-H270"]}
Q_SETS = {"Q4": ["-Q4"], "Q5": ["-Q5"], "Q6": ["-Q6"]}      # (-Q7 is the default of every other run)
SETS = {"a": dict(seed=11, n=300, q_per_class=8, q_levels=True), "b": dict(seed=23, n=220, q_per_class=6, q_levels=False, h_levels=True)}


def rand_protein(rng, n):
    return "".join(AA[i] for i in rng.integers(0, 20, size=n))


def mutate(rng, s, sub, indel=0.0):
    out = []
    for c in s:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(AA[rng.integers(0, 20)])
        out.append(AA[rng.integers(0, 20)] if rng.random() < sub else c)
    return "".join(out)


def make_set(seed, n, q_per_class, **_):
    rng = np.random.default_rng(seed)
    db = [rand_protein(rng, int(rng.integers(60, 701))) for _ in range(n)]
    for k in range(n // 8):                                     # paralogs of others
        db[n - 1 - k] = mutate(rng, db[k], 0.25, 0.04)
    db[n // 2] = db[5]                                          # one sequence under two names: equal fstat.val, equal rscr
    names = [f"p{i}" for i in range(n)]
    queries = []

    def add(cls, src, s):
        queries.append(dict(name=f"q{len(queries)}", cls=cls, src=src, seq=s))
    for i in range(q_per_class):
        s = 10 + i                                              # (sources that have no planted copy or paralog ... but 5 below)
        add("m15", s, mutate(rng, db[s], 0.15, 0.03))
        a = int(rng.integers(0, len(db[s + 20]) - 60))
        add("frag", s + 20, db[s + 20][a:a + int(rng.integers(12, 61))])
        add("xx", s + 40, "".join("X" if k % 10 == 9 else c for k, c in enumerate(mutate(rng, db[s + 40], 0.10))))
        add("m35", s + 60, mutate(rng, db[s + 60], 0.35))
        add("m50", s + 80, mutate(rng, db[s + 80], 0.50))
        add("unr", -1, rand_protein(rng, int(rng.integers(60, 400))))
        add("tiny", s + 100, db[s + 100][7:7 + 3 + i + (i % 3)])
    add("twin", 5, mutate(rng, db[5], 0.05))
    add("twin", 5, db[5][10:90])
    add("para", 3, mutate(rng, db[3], 0.10))
    return db, names, queries


def run(cwd, opts):
    r = subprocess.run([REF, "-Q7", "-A0", "-t1"] + opts + ["-aprot", "q.faa"], cwd=cwd, env=ENV, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"spaln {' '.join(opts)} ended with {r.returncode}: {r.stderr[-500:]}")
    return r.stdout, r.stderr


def parse_o4(txt):
    """XYL: <a> <l> <r> <strand> <b> <l> <r> <strand> <val> : <m n len> ...  -> per query the records in print order"""
    out = {}
    for ln in txt.splitlines():
        f = ln.split()
        if not f or f[0] != "XYL:":
            continue
        at = f.index(":", 1)
        out.setdefault(f[1], []).append(dict(b=f[5], a_rng=[int(f[2]), int(f[3])], b_rng=[int(f[6]), int(f[7])], val=f[9],
                                             corners=[int(x) for x in f[at + 1:]]))
    return out


def parse_o0(txt):
    """the -O0 lines (fstat, the two ranges, the two names), verbatim fields, in print order"""
    out = []
    for ln in txt.splitlines():
        f = ln.split()
        if len(f) == 15 and f[9] in "+-" and f[12] in "+-":
            out.append(f)
    return out


def require(cond, msg):
    if not cond:
        sys.exit("make_aa_search_goldens: the reference does not show what the fixtures are to pin: " + msg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="*", default=list(SETS))
    args = ap.parse_args()
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/spaln is not built (make -C oracle/ref_build)")
    for name in args.sets:
        cfg = SETS[name]
        db, names, queries = make_set(**cfg)
        td = tempfile.mkdtemp(prefix="aa_gold_")
        try:
            with open(os.path.join(td, "prot.faa"), "w") as f:
                for n_, s in zip(names, db):
                    f.write(f">{n_}\n{s}\n")
            with open(os.path.join(td, "q.faa"), "w") as f:
                for q in queries:
                    f.write(f">{q['name']}\n{q['seq']}\n")
            r = subprocess.run([REF, "-W", "-KA", "-t1", "prot.faa"], cwd=td, env=ENV, capture_output=True, text=True)
            if r.returncode or not os.path.exists(os.path.join(td, "prot.bka")):
                sys.exit("spaln -W -KA failed: " + r.stderr[-500:])
            runs = {}
            refused = set()
            sets = dict(OPTION_SETS)
            if cfg["q_levels"]:
                sets.update(Q_SETS)
            if cfg.get("h_levels"):
                sets.update(H_SETS)
            for key, opts in sets.items():
                txt, err = run(td, ["-O4"] + opts)
                again, _ = run(td, ["-O4"] + opts)
                require(txt == again, f"two runs of {key} print different records")
                txt0, _ = run(td, ["-O0"] + opts)
                runs[key] = dict(options=opts, o4=parse_o4(txt), o0=parse_o0(txt0))
                refused |= {m.group(1) for m in re.finditer(r"(\S+) \(\d+ - \d+\) \d+ is too short", err)}
            # ---- what the reference alone must show
            d = runs["default"]["o4"]
            planted = [q for q in queries if q["cls"] in ("m15", "frag", "xx")]
            first = sum(1 for q in planted if d.get(q["name"]) and d[q["name"]][0]["b"] == names[q["src"]])
            require(first >= 0.9 * len(planted), f"{first} of {len(planted)} planted sources printed first")
            require(any(q["name"] not in d for q in queries if q["cls"] in ("m35", "m50")), "every m35 / m50 query printed something")
            counts = {len(runs["M4"]["o4"].get(q["name"], [])) for q in queries if q["name"] not in refused}
            require(len(counts) >= 3, f"record counts under -M4: {sorted(counts)}")
            tie = any(len({r_["val"] for r_ in recs}) < len(recs) for recs in runs["M4_pw"]["o4"].values())
            require(tie, "no query with two candidates of equal fstat.val")
            require(refused, "no query refused as too short")
            if cfg.get("h_levels"):
                require("q1" not in runs["H160"]["o4"] and "q8" in runs["H270"]["o4"] and "q1" in d and "q8" in d,
                        "the pairs around -H160 / -H270 are not printed as fstat.val against Vthr says")
            searched_tiny = [q for q in queries if len(q["seq"]) < 12 and q["name"] not in refused and q["name"] in runs["M4_pw"]["o4"]]
            require(searched_tiny, "no query of fewer than 12 residues searched")
            doc = dict(set=name, db=[dict(name=n_, seq=s) for n_, s in zip(names, db)], queries=queries, refused=sorted(refused), runs=runs)
            with gzip.GzipFile(os.path.join(HERE, f"aa_search_{name}.json.gz"), "wb", mtime=0) as f:
                f.write(json.dumps(doc, separators=(",", ":")).encode())
            with open(os.path.join(td, "prot.bka"), "rb") as src, gzip.GzipFile(os.path.join(HERE, f"aa_db_{name}.bka.gz"), "wb", mtime=0) as f:
                f.write(src.read())
            print(name, "sequences", len(db), "queries", len(queries), "refused", len(refused), "planted first", first, "/", len(planted),
                  "-M4 record counts", sorted(counts))
        finally:
            shutil.rmtree(td, ignore_errors=True)


if __name__ == "__main__":
    main()
