#!/usr/bin/env python3
"""Protein pairs end to end: what `spaln -Q0 -A0 -ip -pw` prints for two protein files against the library's unspliced
aligner (spdp_align_b + spdp_skl_rng_b), corner for corner and statistic for statistic, both timed.

    python tools/b_pairs.py --pairs 300 [--seed 1] [--threads 16] [--mean-len 350] [--yl3] [--lcl 15] [--qck 3] [--repeat 5]
                                                                       (an MI355X box; oracle/_ref/spaln for the comparison)

--qck N (1 .. 3): the program with -QN (its seeded path; -Q3 is its default) against spdp_align_b_seeded; the line then also
carries the call's counters (spdp_seeded_stats_b), the share of DP requests of at most 16 rows and of the cells in them, and the
time of the full DP (spdp_align_b) on the same pairs.  SPDP_B_THIN=0 in the environment sends every request through the tiled kernel.

The pairs are generated here: mutated copies with indels, copies with a deleted block, an embedded domain between unrelated
flanks.  The program reads its FIRST file as b and its second as a; so does this tool.  Prints one JSON line.

Also the home of the pair generator and of the parsers of the program's records: tests/golden/make_b_goldens.py uses them.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REF = os.path.join(ROOT, "oracle", "_ref", "spaln")
ENV = dict(os.environ, ALN_TAB=os.path.join(ROOT, "oracle", "_ref", "table"))       # the program's parameter tables, built beside it
AA = "ARNDCQEGHILKMFPSTWYV"
# rough background frequencies of the twenty residues, in the order above
AA_FREQ = np.array([8.3, 5.5, 4.1, 5.5, 1.4, 3.9, 6.8, 7.1, 2.3, 5.9, 9.7, 5.8, 2.4, 3.9, 4.7, 6.6, 5.3, 1.1, 2.9, 6.9])
AA_FREQ = AA_FREQ / AA_FREQ.sum()


def random_protein(rng, n: int) -> str:
    return "".join(AA[i] for i in rng.choice(20, size=n, p=AA_FREQ))


def mutate(rng, s: str, sub=0.15, indel=0.03, max_indel=12) -> str:
    """substitutions everywhere, now and then an insertion or a deletion of 1 .. max_indel residues"""
    out = []
    i = 0
    while i < len(s):
        r = rng.random()
        if r < indel / 2:
            out.append(random_protein(rng, int(rng.integers(1, max_indel + 1))))
        elif r < indel:
            i += int(rng.integers(1, max_indel + 1))
            continue
        out.append(AA[rng.choice(20, p=AA_FREQ)] if rng.random() < sub else s[i])
        i += 1
    return "".join(out) or s[:1]


def make_pair(rng, kind: str, n: int):
    """(a, b) of kind `mut` (mutated copy), `del` (a block deleted), `emb` (a copy of a inside unrelated flanks), `unr`"""
    a = random_protein(rng, n)
    if kind == "mut":
        b = mutate(rng, a)
    elif kind == "del":
        cut = max(1, n // 5)
        at = int(rng.integers(0, max(1, n - cut)))
        b = mutate(rng, a[:at] + a[at + cut:], indel=0.01) if n > 3 else a
    elif kind == "emb":
        fl = max(1, n // 3)
        b = random_protein(rng, int(rng.integers(0, fl + 1))) + mutate(rng, a, sub=0.1, indel=0.01) + random_protein(rng, int(rng.integers(0, fl + 1)))
    elif kind == "unr":
        b = random_protein(rng, max(1, n + int(rng.integers(-n // 8 - 1, n // 8 + 2))))
    else:
        raise ValueError(kind)
    return a, b


def write_fasta(path: str, prefix: str, seqs) -> None:
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(f">{prefix}{i}\n")
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + "\n")


def run_spaln(args, a_seqs, b_seqs, threads=1, tmp=None):
    """runs the program on the pairs (i-th of b against i-th of a) with the given output options; returns (stdout, seconds)"""
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        write_fasta(os.path.join(d, "a.faa"), "a", a_seqs)
        write_fasta(os.path.join(d, "b.faa"), "b", b_seqs)
        cmd = [REF, "-Q0", "-A0", "-ip", "-pw", f"-t{threads}", "-l0"] + list(args) + ["b.faa", "a.faa"]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, env=ENV)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} ended with {r.returncode}: {r.stderr[-400:]}")
        return r.stdout, dt


def parse_o1(txt: str, n: int):
    """-O1: per pair (corners 1-based [[m, n] ..], val / scale); None where the program printed nothing for the pair"""
    out = [None] * n
    lines = txt.splitlines()
    for k, ln in enumerate(lines):
        if not ln.startswith(">a"):
            continue
        i = int(ln[2:].split()[0])
        f = ln.split()
        nums = [int(x) for x in lines[k + 1].split()]
        assert len(nums) == 2 * int(f[-2]), ln
        out[i] = ([[nums[2 * j], nums[2 * j + 1]] for j in range(len(nums) // 2)], float(f[-1]))
    return out


def parse_o0(txt: str, n: int):
    """-O0: per pair dict(val raw, mch, mmc, gap, unp)"""
    out = [None] * n
    for ln in txt.splitlines():
        f = ln.split("\t")
        if len(f) < 5 or not f[-2].startswith("a"):
            continue
        v = f[0].split()
        out[int(f[-2][1:])] = dict(val=float(v[1]), mch=float(v[2]), mmc=float(v[3]), gap=float(v[4]), unp=float(v[5]))
    return out


def parse_o8(txt: str, n: int):
    """-O8: per pair the Cigar operations as a list [[op, len] ..]"""
    out = [None] * n
    for ln in txt.splitlines():
        if not ln.startswith("cigar:"):
            continue
        f = ln.split()
        i = int(f[1][1:])
        ops = f[10:]
        out[i] = [[ops[2 * j], int(ops[2 * j + 1])] for j in range(len(ops) // 2)]
    return out


def exg_of(lcl: int):
    """(a_exgl, a_exgr, b_exgl, b_exgr) of `-L<lcl>` (src/spaln.cc:759-764); bit 16: local, all ends free"""
    if lcl & 16:
        return (1, 1, 1, 1)
    return (1 if lcl & 4 else 0, 1 if lcl & 8 else 0, 1 if lcl & 1 else 0, 1 if lcl & 2 else 0)


def library_records(eng, sc, up, pairs, lcl, seeded=None, grp=None):
    """the library's record per pair: (corners 1-based after trimskl, stat dict, engine score); (None, None, score) where
    there is no alignment.  seeded = (SeedParams, WilipModel): through spdp_align_b_seeded instead of spdp_align_b; grp: an
    engine.Group that runs the call in place of the engine (spdp_group_align_b / _align_b_seeded)"""
    from spaln_amd import abi, synth
    ps = abi.ProblemSet()
    for a, b in pairs:
        ps.add(synth.encode_protein(np.frombuffer(a.encode(), dtype=np.uint8)), synth.encode_protein(np.frombuffer(b.encode(), dtype=np.uint8)),
               None, None, exg=exg_of(lcl))
    who = grp or eng
    alns = who.align_b_seeded(sc, up, seeded[0], ps, model=seeded[1]) if seeded else who.align_b(sc, up, ps)
    dt = who.last_call_s                   # the call alone: upload, walks, kernels, download, corner lists
    stats = eng.skl_rng_b(sc, up, ps, [s for _, s in alns])
    out = []
    for (score, skl), st in zip(alns, stats):
        if skl.shape[0] < 3:
            out.append((None, None, score))
            continue
        c = skl[st["first"]:st["first"] + st["n_trim"]] + 1
        out.append((c.tolist(), st, score))
    return out, dt, ps


def same_record(lib_rec, corners, val_scaled, o0, scale) -> bool:
    c, st, _ = lib_rec
    if c is None:
        return corners is None
    if corners is None or c != corners:
        return False
    if abs(st["val"] / scale - val_scaled) > 0.005 + 1e-9:
        return False
    if o0 is not None:
        if abs(st["val"] - o0["val"]) > 0.005 or st["mch"] != o0["mch"] or st["mmc"] != o0["mmc"]:
            return False
        if abs(st["gap"] - o0["gap"]) > 0.05 + 1e-6 or abs(st["unp"] - o0["unp"]) > 0.05 + 1e-6:
            return False
    return True


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--mean-len", type=int, default=350)
    ap.add_argument("--lcl", type=int, default=15)
    ap.add_argument("--yl3", action="store_true")
    ap.add_argument("--no-reference", action="store_true", help="library only (a profiler run): nothing is compared")
    ap.add_argument("--qck", type=int, default=0, help="1 .. 3: the reference with -Q<n> against the seeded entry (spdp_align_b_seeded); 0: -Q0")
    ap.add_argument("--repeat", type=int, default=1, help="timed repetitions of the library call (after the warm-up call)")
    ap.add_argument("--members", type=int, default=0, help="N: the call also goes through a device group of N contexts, all on device 0 (spdp_group_align_b / "
                    "_align_b_seeded); the records compared are then the group's.  Members on one card share it: no scaling figure")
    ap.add_argument("--gpus", default="", help="a,b,..: the same with one context on each of these devices")
    args = ap.parse_args()
    from spaln_amd import abi, defaults, engine

    rng = np.random.default_rng(args.seed)
    kinds = ["mut", "del", "emb"]
    pairs = []
    for i in range(args.pairs):
        n = int(np.clip(rng.normal(args.mean_len, args.mean_len / 4), 30, 3 * args.mean_len))
        pairs.append(make_pair(rng, kinds[i % 3], n))
    opts = [f"-L{args.lcl}"] + (["-yl3"] if args.yl3 else []) + ([f"-Q{args.qck}"] if args.qck else [])     # (the later -Q wins)
    a_seqs, b_seqs = [p[0] for p in pairs], [p[1] for p in pairs]
    want1 = want0 = None
    ref_s = float("nan")
    if not args.no_reference:
        o1, ref_s = run_spaln(opts + ["-O1"], a_seqs, b_seqs, threads=args.threads)
        o0, _ = run_spaln(opts + ["-O0"], a_seqs, b_seqs, threads=args.threads)
        want1, want0 = parse_o1(o1, len(pairs)), parse_o0(o0, len(pairs))

    eng = engine.Engine(0)
    sc = defaults.scoring_b(noll=3 if args.yl3 else 2, local=1 if args.lcl & 16 else 0)
    up = abi.UnsplicedParams(1.0, 0)
    seeded = (defaults.seed_params_b(args.qck, args.lcl), defaults.wilip_model_b()) if args.qck else None
    library_records(eng, sc, up, pairs[:min(len(pairs), 64)], args.lcl, seeded)          # first call: allocations, module load
    got, lib_s, ps = library_records(eng, sc, up, pairs, args.lcl, seeded)
    times = [lib_s]
    for _ in range(args.repeat - 1):
        got, lib_s, ps = library_records(eng, sc, up, pairs, args.lcl, seeded)
        times.append(lib_s)
    lib_s = float(np.median(times))
    extra = {}
    devices = [int(x) for x in args.gpus.split(",")] if args.gpus else [0] * max(args.members, 0)
    if devices:                                         # the same call on the group: its records are the ones compared below
        grp = engine.Group(devices)
        library_records(eng, sc, up, pairs[:min(len(pairs), 64 * len(devices))], args.lcl, seeded, grp)
        g_times = []
        for _ in range(max(1, args.repeat)):
            got, g_s, ps = library_records(eng, sc, up, pairs, args.lcl, seeded, grp)
            g_times.append(g_s)
        member = grp.shards(len(pairs))
        cost = np.array([eng.cells_b(p, sc.sh) for p in ps.items], dtype=np.int64)
        extra["group"] = dict(devices=devices, library_align_s=round(float(np.median(g_times)), 4), library_align_s_all=[round(t, 4) for t in g_times],
                              pairs_per_member=[int((member == r).sum()) for r in range(len(devices))],
                              cells_per_member=[int(cost[member == r].sum()) for r in range(len(devices))], largest_cost=int(cost.max()),
                              over_one_context=round(float(np.median(g_times)) / lib_s, 3))
        grp.close()
    if seeded:
        st = eng.seeded_stats_b()
        dp = st["thin_requests"] + st["wide_requests"] + st["requests_not_computed"]
        extra.update({"seeded_stats": st, "share_requests_le16_rows": round(st["requests_le16_rows"] / max(dp, 1), 4),
                      "share_cells_le16_rows": round(st["cells_le16_rows"] / max(st["cells"], 1), 4)})
        eng.align_b(sc, up, ps)                                                    # (warm) the full DP on the same pairs
        eng.align_b(sc, up, ps)
        extra["library_full_dp_align_s"] = round(eng.last_call_s, 4)
    if args.repeat > 1:
        extra["library_align_s_all"] = [round(t, 4) for t in times]
    t0 = time.perf_counter()
    eng.homscore_b(sc, up, ps)
    score_s = time.perf_counter() - t0
    cells = sum(eng.cells_b(p, sc.sh) for p in ps.items)
    bad = [] if want1 is None else [i for i in range(len(pairs))
           if not same_record(got[i], want1[i][0] if want1[i] else None, want1[i][1] if want1[i] else 0.0, want0[i], defaults.B_SCALE)]
    print(json.dumps({
        "what": "every record `spaln -Q0 -A0 -ip -pw %s` prints against %s%s + spdp_skl_rng_b" % (" ".join(opts), "spdp_group_" if devices else "spdp_",
                                                                                               "align_b_seeded" if seeded else "align_b"),
        "pairs": len(pairs), "identical": None if want1 is None else len(pairs) - len(bad), "first_differing": bad[:5], "cells": cells,
        "library_align_s": round(lib_s, 4), "library_pairs_per_s": round(len(pairs) / lib_s, 1), "library_gcups": round(cells / lib_s / 1e9, 3),
        "library_homscore_s": round(score_s, 4),
        "reference_threads": args.threads, "reference_s": None if want1 is None else round(ref_s, 4),
        "reference_pairs_per_s": None if want1 is None else round(len(pairs) / ref_s, 1),
        "reference_gcups": None if want1 is None else round(cells / ref_s / 1e9, 3), "device": eng.device_name(), **extra}))
    eng.close()
    return 0 if not bad else 1


if __name__ == "__main__":
    sys.exit(main())
