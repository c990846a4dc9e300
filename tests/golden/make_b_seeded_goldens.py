#!/usr/bin/env python3
"""Writes the fixtures of the unspliced aligner's seeded path, tests/golden/b_aas_*.json.gz, from runs of the compiled reference
program (oracle/_ref/spaln -Q<n> -A0 -ip -pw, n = 1 .. 3; build it with __graft_entry__.build() where the reference's source
tree is present).

    python tests/golden/make_b_seeded_goldens.py

  b_aas_<set>_q<n>.json.gz  (gzip of one JSON document) sequences, option sets and the printed records of -Q<n> (-O1 corners and
                       score, -O0 statistics, -O8 Cigar).  A pair the program prints nothing for is recorded as null; the run
                       goes on.
Every file holds data only.  The HSP-search model of protein pairs (b_aa_wilip.json) is recorded separately: see its "source".

The script stops unless at least a fifth of the `mid`, `long` and `gaps` pairs have, under -Q3, a corner list different from
the -Q0 record of the same pair: otherwise the fixtures would not exercise the walk."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tools import b_pairs  # noqa: E402
import make_b_goldens  # noqa: E402

GAP_BLOCKS = [1, 2, 15, 16, 17, 40, 64, 65]
SUB_BLOCKS = ([1, 6, 8, 10, 40], [1, 8, 40])             # blocks that stand for two residues of the other copy: in a, in b


def opts_of(lcl, noll, tgapf, qck):
    # (the later -Q wins over the -Q0 run_spaln puts first)
    return (["-LS"] if lcl & 16 else [f"-L{lcl}"]) + (["-yl3"] if noll == 3 else []) + ([f"-yt{tgapf}"] if tgapf != 1.0 else []) + [f"-Q{qck}"]


def records(opts, pairs):
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    o1 = b_pairs.parse_o1(b_pairs.run_spaln(opts + ["-O1"], a, b)[0], len(pairs))
    o0 = b_pairs.parse_o0(b_pairs.run_spaln(opts + ["-O0"], a, b)[0], len(pairs))
    o8 = b_pairs.parse_o8(b_pairs.run_spaln(opts + ["-O8"], a, b)[0], len(pairs))
    out = []
    for i in range(len(pairs)):
        if o1[i] is None or o0[i] is None:
            assert o1[i] is None and o0[i] is None and o8[i] is None, (opts, i)
            out.append(None)
        else:
            out.append(dict(corners=o1[i][0], score=o1[i][1], cigar=o8[i], **o0[i]))
    return out


def write_set(name, pairs, runs, walk_check=False):
    doc = dict(pairs=[dict(a=a, b=b) for a, b in pairs], runs=[])
    for lcl, noll, tgapf, qck in runs:
        opts = opts_of(lcl, noll, tgapf, qck)
        recs = records(opts, pairs)
        doc["runs"].append(dict(opts=opts, lcl=lcl, noll=noll, tgapf=tgapf, qck=qck, records=recs))
    differ = total = 0
    if walk_check:
        for run in doc["runs"]:
            if run["qck"] != 3:
                continue
            q0 = b_pairs.parse_o1(b_pairs.run_spaln([o for o in run["opts"] if not o.startswith("-Q")] + ["-O1"],
                                                    [p[0] for p in pairs], [p[1] for p in pairs])[0], len(pairs))
            for r, z in zip(run["records"], q0):
                total += 1
                differ += (r["corners"] if r else None) != (z[0] if z else None)
    sizes = []
    for qck in sorted({r["qck"] for r in doc["runs"]}):                 # one file per recursion depth: each stays small
        part = dict(pairs=doc["pairs"], runs=[r for r in doc["runs"] if r["qck"] == qck])
        path = os.path.join(HERE, f"b_aas_{name}_q{qck}.json.gz")
        with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
            g.write(json.dumps(part, separators=(",", ":")).encode())    # (no name, no time stamp: the same bytes on every run)
        sizes.append(os.path.getsize(path))
    none = sum(r is None for run in doc["runs"] for r in run["records"])
    print(name, len(pairs), "pairs x", len(runs), "option sets ->", sizes, "bytes;", none, "without a record;",
          f"{differ} of {total} -Q3 records differ from -Q0" if walk_check else "")
    return differ, total


def gap_pairs(seed):
    """two copies of a random 120-residue protein that differ by one inserted block of k residues, in a and then in b; then the
    same with the block standing in for two residues of the other copy.  Between the two HSPs of a pure insertion the program
    runs no DP at all (one of the two gaps is empty: backforth joins them in closed form); with two residues opposite the
    block both gaps are open and lspB_ng gets a request of about k + 2 rows (block in a) or columns (block in b), plus the few
    residues creepback / creepfwrd hand back -- requests on both sides of the 16-row boundary between the thin and the tiled sweep."""
    rng = np.random.default_rng(seed)
    out = []
    for stands_for, blocks in ((0, (GAP_BLOCKS, GAP_BLOCKS)), (2, SUB_BLOCKS)):
        for side in (0, 1):
            for k in blocks[side]:
                p = b_pairs.random_protein(rng, 120)
                q = p[:60 - stands_for // 2] + b_pairs.random_protein(rng, k + stands_for) + p[60 + stands_for // 2:]
                out.append((q, p) if side == 0 else (p, q))
    return out


def main():
    if not os.path.exists(b_pairs.REF):
        raise SystemExit(f"{b_pairs.REF} is not built")
    ends = [(lcl, noll, 1.0, qck) for qck in (1, 3) for lcl in (15, 0, 5, 10) for noll in (2, 3)]
    local = [(16, noll, 1.0, qck) for qck in (1, 3) for noll in (2, 3)]
    extra = [(15, 2, 1.0, 2), (0, 2, 0.5, 3)]
    write_set("shapes", make_b_goldens.shape_pairs(1), ends + extra)
    write_set("local", make_b_goldens.local_pairs(5), ends + local + extra)
    rng = np.random.default_rng(3)
    mid = [b_pairs.make_pair(rng, ("mut", "del", "emb")[i % 3], int(rng.integers(300, 701))) for i in range(12)]
    long_ = [b_pairs.make_pair(rng, "mut", 1400), b_pairs.make_pair(rng, "del", 1500)]
    differ = total = 0
    for name, pairs in (("mid", mid), ("long", long_), ("gaps", gap_pairs(7))):
        d, t = write_set(name, pairs, ends + local + extra, walk_check=True)
        differ += d
        total += t
    if differ * 5 < total:
        raise SystemExit(f"only {differ} of {total} -Q3 records of mid / long / gaps differ from the -Q0 record: the fixtures do not exercise the walk")
    print(f"{differ} of {total} -Q3 records of mid / long / gaps differ from -Q0")


if __name__ == "__main__":
    main()
