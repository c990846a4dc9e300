#!/usr/bin/env python3
"""Writes the fixtures of the unspliced aligner, tests/golden/b_aa_params.json and b_aa_*.json.gz, from runs of the compiled reference program
(oracle/_ref/spaln -Q0 -A0 -ip -pw; build it with __graft_entry__.build() where the reference's source tree is present).

    python tests/golden/make_b_goldens.py

  b_aa_params.json   the protein-pair parameters as the program applies them, read off its printed scores: the substitution
                     matrix from all 1 x 1 pairs, the gap terms from pairs that differ by one block of 1, 2, 9 and 10 residues
  b_aa_<set>.json.gz (gzip of one JSON document) sequences, option sets and the printed records (-O1 corners and score, -O0 statistics, -O8 Cigar)
Every file holds data only.  A pair the program prints nothing for stops the script with the pair's name."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tools import b_pairs  # noqa: E402

LENGTHS = [1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 130, 300]
END_MODES = [15, 0, 3, 5, 10]


def records(opts, pairs, name):
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    o1 = b_pairs.parse_o1(b_pairs.run_spaln(opts + ["-O1"], a, b)[0], len(pairs))
    o0 = b_pairs.parse_o0(b_pairs.run_spaln(opts + ["-O0"], a, b)[0], len(pairs))
    o8 = b_pairs.parse_o8(b_pairs.run_spaln(opts + ["-O8"], a, b)[0], len(pairs))
    out = []
    for i in range(len(pairs)):
        if o1[i] is None or o0[i] is None:
            raise SystemExit(f"{name} {' '.join(opts)}: the program printed no record for pair {i} ({len(pairs[i][0])} x {len(pairs[i][1])})")
        out.append(dict(corners=o1[i][0], score=o1[i][1], cigar=o8[i], **o0[i]))
    return out


def write_set(name, pairs, runs):
    doc = dict(pairs=[dict(a=a, b=b) for a, b in pairs], runs=[])
    for lcl, noll, tgapf in runs:
        opts = (["-LS"] if lcl & 16 else [f"-L{lcl}"]) + (["-yl3"] if noll == 3 else []) + ([f"-yt{tgapf}"] if tgapf != 1.0 else [])
        doc["runs"].append(dict(opts=opts, lcl=lcl, noll=noll, tgapf=tgapf, records=records(opts, pairs, name)))
    path = os.path.join(HERE, f"b_aa_{name}.json.gz")
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
        g.write(json.dumps(doc, separators=(",", ":")).encode())         # (no name, no time stamp: the same bytes on every run)
    print(name, len(pairs), "pairs x", len(runs), "option sets ->", os.path.getsize(path), "bytes")


def shape_pairs(seed):
    rng = np.random.default_rng(seed)
    return [b_pairs.make_pair(rng, kind, n) for n in LENGTHS for kind in ("mut", "emb", "unr")]


def local_pairs(seed):
    """every sequence at least 5 long, every pair shares a planted segment of at least 12 residues"""
    rng = np.random.default_rng(seed)
    out = []
    for n in [5, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 130, 300]:
        for kind in ("mut", "emb"):
            core = b_pairs.random_protein(rng, 12 + int(rng.integers(0, 6)))
            a, b = b_pairs.make_pair(rng, kind, n)
            ka, kb = int(rng.integers(0, len(a) + 1)), int(rng.integers(0, len(b) + 1))
            out.append((a[:ka] + core + a[ka:], b[:kb] + core + b[kb:]))
    return out


def params():
    """the parameters behind the printed scores"""
    aa = b_pairs.AA
    pairs = [(x, y) for x in aa for y in aa]
    raw = b_pairs.parse_o0(b_pairs.run_spaln(["-L0", "-O0"], [p[0] for p in pairs], [p[1] for p in pairs])[0], len(pairs))
    o1 = b_pairs.parse_o1(b_pairs.run_spaln(["-L0", "-O1"], [p[0] for p in pairs], [p[1] for p in pairs])[0], len(pairs))
    mtx = [[0] * 20 for _ in range(20)]
    for k, (x, y) in enumerate(pairs):
        assert o1[k][0] == [[1, 1], [2, 2]], (x, y, o1[k])
        mtx[aa.index(x)][aa.index(y)] = int(round(raw[k]["val"]))
    scale = None
    for k in range(len(pairs)):
        if abs(o1[k][1]) >= 1:
            scale = round(raw[k]["val"] / o1[k][1])
            break
    rng = np.random.default_rng(99)
    left, right = b_pairs.random_protein(rng, 40), b_pairs.random_protein(rng, 40)

    def gap_cost(d, opts):
        ins = "".join("WCWC"[i % 4] for i in range(d))
        r = b_pairs.parse_o0(b_pairs.run_spaln(["-L0", "-O0"] + opts, [left + ins + right], [left + right])[0], 1)[0]
        base = sum(mtx[aa.index(c)][aa.index(c)] for c in left + right)
        assert r["mch"] == 80 and r["gap"] == 1 and r["unp"] == d, (d, r)
        return int(round(r["val"])) - base
    g1, g2 = gap_cost(1, []), gap_cost(2, [])
    gep = g2 - g1
    gop = g1 - gep
    l9, l10 = gap_cost(9, ["-yl3"]), gap_cost(10, ["-yl3"])
    lgep = l10 - l9
    lgop = l9 - 9 * lgep
    k1 = 7
    assert lgop == gop - (lgep - gep) * k1, (gop, gep, lgop, lgep)
    assert gap_cost(7, ["-yl3"]) == gop + 7 * gep and gap_cost(8, ["-yl3"]) == lgop + 8 * lgep
    doc = dict(alphabet=aa, mtx=mtx, gop=gop, gep=gep, lgop=lgop, lgep=lgep, k1=k1, scale=scale, sh=100,
               u=-gep / scale, v=-gop / scale, u1=-lgep / scale, thr=35.0)
    with open(os.path.join(HERE, "b_aa_params.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("params", {k: v for k, v in doc.items() if k != "mtx"})


def main():
    if not os.path.exists(b_pairs.REF):
        raise SystemExit(f"{b_pairs.REF} is not built")
    params()
    ends = [(lcl, noll, 1.0) for lcl in END_MODES for noll in (2, 3)]
    write_set("shapes1", shape_pairs(1), ends)
    write_set("shapes2", shape_pairs(2), ends)
    rng = np.random.default_rng(3)
    mid = [b_pairs.make_pair(rng, ("mut", "del", "emb")[i % 3], int(rng.integers(300, 701))) for i in range(12)]
    write_set("mid", mid, ends)
    long_ = [b_pairs.make_pair(rng, "mut", 1400), b_pairs.make_pair(rng, "del", 1500)]
    write_set("long", long_, ends)
    write_set("tgapf", shape_pairs(4)[18:], [(0, 2, 0.5), (0, 3, 0.5), (5, 2, 0.5)])
    write_set("local", local_pairs(5), [(16, 2, 1.0), (16, 3, 1.0)])


if __name__ == "__main__":
    main()
