#!/usr/bin/env python3
"""Protein queries against a protein database inside the library, against the reference's own program.

    python tools/aa_search.py [--queries 300] [--sequences 580] [--threads 16] [--max-out N] [--all-out] [--library-index]
                              [--rscr slab|hash[,..]]
                                                                      (an MI355X box; oracle/_ref for the comparison)

A synthetic protein database with paralog families and queries of eight classes (mutated at 15 / 35 / 50 %, fragments, every tenth
residue X, unrelated, tiny) is formatted by the compiled reference's own `spaln -W -KA`.  Two runs on the same files:

  * reference:  oracle/_ref/spaln -Q7 -A0 -O4 -t<threads> [-M N] [-pw] -aprot q.faa      (-A0: the scalar engine of Aln2b1, the one
                the library's unspliced aligner reproduces)
  * library:    prot.bka read by spdp_blk_index_read, the database's residue codes, and then ONE spdp_map_align_b call = the vote
                of SrchBlk::finds on the device -> every candidate a pair -> spdp_align_b_seeded -> spdp_skl_rng_b -> the
                threshold and the order of the printed hits.

With --library-index the library does not read prot.bka: it builds the index itself from the database's residue codes
(spdp_blk_index_build_a; its three `seconds` are printed beside the wall time of `spaln -W -KA`, whose protein path is serial whatever
-t says), the hit lists are still held to the program's run on the program's file, and the two .bka files are compared outside the
bytes that hold the program's heap (blocks.bka_without_heap_bytes).

Compared per query: the ordered hit list (name, printed score, the corners as -O4 prints them, the aligned ranges).  One JSON line: reference
aligned, library aligned, identical, seconds of both (the library's call warm: the median of --repeat calls after a first one),
the library's split from spdp_blk_finds_stats and the vote kernel's HIP-event time.  Reads nothing of the reference's sources.

--rscr slab|hash chooses what holds the scores of the vote (SPDP_FINDS_RSCR) for every index the run searches, and
adds "rscr" to the JSON line: for the form (for each, when several are given with a comma; the first one serves the rest of the run)
a FRESH index and on it the vote alone -- the first call (wall and kernel ms: the waves' areas are allocated and cleared in it),
--repeat warm calls (kernel ms each), and spdp_blk_finds_store_stats of the last: waves, bytes of a wave's area, bytes of all,
launches, queries run again, the most blocks a query scored.  "baseline" instead of a form leaves the variable alone (and asks no
stats of a library that has no such entry: the parent's build through SPDP_LIB).

--members N puts N contexts ON DEVICE 0 behind one device group (--gpus a,b,..: one context on each of these devices), an index per
member, and the call becomes ONE spdp_group_map_align_b call: the records compared with the program's are then the group's, the
single-context call is still timed beside it, and "group" in the JSON line holds the group call's seconds and every member's load
(queries, 1 + length summed: the cost the shards are balanced by).  Several members on one card share that card: the figures say
what the fan-out and the gathering cost and that the records are the same, not how the call scales."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spaln_amd import abi, blocks, defaults, engine  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "spaln")
ENV = dict(os.environ, ALN_TAB=os.path.join(ROOT, "oracle", "_ref", "table"))
AA = "ARNDCQEGHILKMFPSTWYV"
CLASSES = ("m15", "frag", "xx", "m35", "m50", "unr", "tiny", "para")


def encode(s: str) -> np.ndarray:
    lut = np.full(256, 2, dtype=np.uint8)               # X and anything else: AMB
    for i, c in enumerate(AA):
        lut[ord(c)] = i + 3
    return lut[np.frombuffer(s.encode(), dtype=np.uint8)]


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


def make_data(rng, n_seq, n_queries):
    db = [rand_protein(rng, int(rng.integers(60, 701))) for _ in range(n_seq)]
    n_fam = max(1, n_seq // 8)
    for k in range(n_fam):                              # paralogs of others
        db[n_seq - 1 - k] = mutate(rng, db[k], 0.25, 0.04)
    queries = []
    for i in range(n_queries):
        cls = CLASSES[i % len(CLASSES)]
        src = int(rng.integers(n_fam, n_seq - n_fam)) if cls != "para" else int(rng.integers(0, n_fam))
        s = db[src]
        if cls == "m15":
            q = mutate(rng, s, 0.15, 0.03)
        elif cls == "frag":
            a = int(rng.integers(0, len(s) - 59))
            q = s[a:a + int(rng.integers(12, 61))]
        elif cls == "xx":
            q = "".join("X" if k % 10 == 9 else c for k, c in enumerate(mutate(rng, s, 0.10)))
        elif cls == "m35":
            q = mutate(rng, s, 0.35)
        elif cls == "m50":
            q = mutate(rng, s, 0.50)
        elif cls == "unr":
            q, src = rand_protein(rng, int(rng.integers(60, 400))), -1
        elif cls == "tiny":
            q = s[5:5 + int(rng.integers(3, 12))]
        else:
            q = mutate(rng, s, 0.10)
        queries.append((f"q{i}", cls, src, q))
    return db, queries


def parse_o4(txt):
    out = {}
    for ln in txt.splitlines():
        f = ln.split()
        if f and f[0] == "XYL:":
            at = f.index(":", 1)
            out.setdefault(f[1], []).append((f[5], f[9], [int(x) for x in f[at + 1:]]))
    return out


def segments(corners):
    out = []
    for (m0, n0), (m1, n1) in zip(corners[:-1], corners[1:]):
        if m1 - m0 == n1 - n0 and m1 > m0:
            out += [int(m0) + 1, int(n0) + 1, int(m1 - m0)]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=300)
    ap.add_argument("--sequences", type=int, default=580)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--max-out", type=int, default=1)
    ap.add_argument("--all-out", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true", help="library only (a profiler run): nothing is compared")
    ap.add_argument("--library-index", action="store_true", help="the library builds its own index of the database instead of reading prot.bka")
    ap.add_argument("--members", type=int, default=0, help="N: the call goes through a device group of N contexts, all on device 0 (spdp_group_map_align_b)")
    ap.add_argument("--gpus", default="", help="a,b,..: the same with one context on each of these devices")
    ap.add_argument("--rscr", default="", help="slab|hash[,..]: what holds the vote's scores (SPDP_FINDS_RSCR); measures the vote alone on a fresh index per form")
    args = ap.parse_args()
    forms = [f for f in args.rscr.split(",") if f]
    if any(f not in ("slab", "hash", "baseline") for f in forms):
        ap.error("--rscr: slab, hash or baseline")
    if forms and forms[0] != "baseline":
        os.environ["SPDP_FINDS_RSCR"] = forms[0]
    devices = [int(x) for x in args.gpus.split(",")] if args.gpus else [0] * max(args.members, 0)
    rng = np.random.default_rng(args.seed)
    db, queries = make_data(rng, args.sequences, args.queries)
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "prot.faa"), "w") as f:
            for i, s in enumerate(db):
                f.write(f">p{i}\n{s}\n")
        with open(os.path.join(td, "q.faa"), "w") as f:
            for name, _, _, q in queries:
                f.write(f">{name}\n{q}\n")
        t0 = time.perf_counter()
        r = subprocess.run([REF, "-W", "-KA", f"-t{args.threads}", "prot.faa"], cwd=td, env=ENV, capture_output=True, text=True)
        format_s = time.perf_counter() - t0
        if r.returncode or not os.path.exists(os.path.join(td, "prot.bka")):
            print("spaln -W -KA failed: " + r.stderr[-400:], file=sys.stderr)
            return 2
        want, ref_s, ref_default_s, default_differs = None, None, None, None
        if not args.no_reference:
            opts = ([f"-M{args.max_out}"] if args.max_out > 1 else []) + (["-pw"] if args.all_out else [])
            cmd = [REF, "-Q7", "-A0", "-O4", f"-t{args.threads}"] + opts + ["-aprot", "q.faa"]
            subprocess.run(cmd, cwd=td, env=ENV, capture_output=True, text=True)        # (warm: the files in the page cache)
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=td, env=ENV, capture_output=True, text=True)
            ref_s = time.perf_counter() - t0
            if r.returncode:
                print("spaln ended with %d: %s" % (r.returncode, r.stderr[-400:]), file=sys.stderr)
                return 2
            want = parse_o4(r.stdout)
            # the program as it runs without -A0 (its default engine of Aln2b1), on the same files: its time, and how many queries'
            # records differ from the -A0 run's
            cmd_d = [c for c in cmd if c != "-A0"]
            subprocess.run(cmd_d, cwd=td, env=ENV, capture_output=True, text=True)
            t0 = time.perf_counter()
            r = subprocess.run(cmd_d, cwd=td, env=ENV, capture_output=True, text=True)
            ref_default_s = time.perf_counter() - t0
            want_d = parse_o4(r.stdout) if r.returncode == 0 else None
            default_differs = None if want_d is None else sum(1 for name, _, _, _ in queries if want_d.get(name, []) != want.get(name, []))
        eng = engine.Engine(0)
        seqs = [encode(s) for s in db]
        db_off = np.zeros(len(seqs) + 1, dtype=np.int64)
        db_off[1:] = np.cumsum([len(s) for s in seqs])
        db_codes = np.concatenate(seqs)
        build = None
        t0 = time.perf_counter()
        if args.library_index:
            prm = blocks.build_params_default_a(eng.lib, int(db_off[-1]))
            blocks.build_index_a(eng, db_codes[:db_off[min(64, len(seqs))]], db_off[:min(64, len(seqs)) + 1], prm)      # first call: module load
            t0 = time.perf_counter()
            mine_bka = os.path.join(td, "library.bka")
            arrays, fprm, build_sec = blocks.build_index_a(eng, db_codes, db_off, prm, write_to=mine_bka, max_out=args.max_out)
            with open(mine_bka, "rb") as f, open(os.path.join(td, "prot.bka"), "rb") as g:
                a, b = f.read(), g.read()
            build = dict(seconds_device_host_call=[round(x, 4) for x in build_sec], ktuple=int(prm.b.ktuple), tabsize=int(arrays["tabsize"]),
                         postings=int(arrays["blk_blkb"].size), files_equal_outside_heap_bytes=blocks.bka_without_heap_bytes(a) == blocks.bka_without_heap_bytes(b),
                         library_maxblk=int(arrays["maxblk"]), program_maxblk=int.from_bytes(b[78:80], "little"))
        else:
            arrays, fprm = blocks.read_protein_db_index(eng.lib, os.path.join(td, "prot.bka"), max_out=args.max_out)
        dix = blocks.BlockIndex(eng, arrays)
        load_s = time.perf_counter() - t0
        grp = engine.Group(devices) if devices else None
        gix = blocks.GroupIndex(grp, arrays) if grp else None
    sc, up, model = defaults.scoring_b(), abi.UnsplicedParams(1.0, 0), defaults.wilip_model_b()
    sp = defaults.seed_params_b(3, 15)
    sp.wilip = C.addressof(model)
    q_codes = [encode(q) for _, _, _, q in queries]
    blocks.map_align_b(dix, db_codes, db_off, sc, up, sp, fprm, q_codes[:min(64, len(q_codes))], all_out=args.all_out)     # first call: allocations, module load
    times, splits, kernel_ms = [], [], []
    for _ in range(max(1, args.repeat)):
        t0 = time.perf_counter()
        got, sec = blocks.map_align_b(dix, db_codes, db_off, sc, up, sp, fprm, q_codes, all_out=args.all_out)
        times.append(time.perf_counter() - t0)
        splits.append(blocks.finds_stats(eng))
    k = int(np.argsort(times)[len(times) // 2])
    lib_s, st = times[k], splits[k]
    _, ms = blocks.finds(dix, fprm, q_codes)             # the vote alone: HIP-event time
    dix.free()
    rscr = {}
    for form in forms:                                  # the vote alone on a fresh index: what its first call costs, what a warm one
        if form != "baseline":
            os.environ["SPDP_FINDS_RSCR"] = form
        vix = blocks.BlockIndex(eng, arrays)
        t0 = time.perf_counter()
        first, first_ms = blocks.finds(vix, fprm, q_codes)
        first_s = time.perf_counter() - t0
        warm, walls = [], []
        for _ in range(max(1, args.repeat)):
            t0 = time.perf_counter()
            again, w_ms = blocks.finds(vix, fprm, q_codes)
            walls.append(time.perf_counter() - t0)
            warm.append(w_ms)
        sst = blocks.finds_store_stats(eng) if hasattr(eng.lib, "spdp_blk_finds_store_stats") else None
        vix.free()
        rscr[form] = dict(first_call_s=round(first_s, 4), first_kernel_ms=round(first_ms, 3), warm_kernel_ms=[round(x, 3) for x in warm],
                          warm_call_s=[round(x, 4) for x in walls], stats=sst, allocated_bytes=None if sst is None else sst["waves"] * sst["area_bytes"],
                          records_crc=int(np.bitwise_xor.reduce(again.view(np.uint32).reshape(-1) * np.arange(1, again.size + 1, dtype=np.uint32))),
                          same_as_first_call=bool(np.array_equal(first, again)))
    if forms and forms[0] != "baseline":
        os.environ["SPDP_FINDS_RSCR"] = forms[0]
    group = None
    if grp:                                             # the same call on the group: its records are the ones compared below
        blocks.group_map_align_b(gix, db_codes, db_off, sc, up, sp, fprm, q_codes[:min(64 * len(devices), len(q_codes))], all_out=args.all_out)
        g_times, g_secs = [], []
        for _ in range(max(1, args.repeat)):
            t0 = time.perf_counter()
            got, sec = blocks.group_map_align_b(gix, db_codes, db_off, sc, up, sp, fprm, q_codes, all_out=args.all_out)
            g_times.append(time.perf_counter() - t0)
            g_secs.append(sec)
        member = grp.shards(len(q_codes))
        k = int(np.argsort(g_times)[len(g_times) // 2])
        cost = np.array([1 + len(q) for q in q_codes], dtype=np.int64)
        group = dict(devices=devices, library_s=round(g_times[k], 4), library_s_all=[round(t, 4) for t in g_times],
                     seconds_vote_align_host_call=[round(x, 4) for x in g_secs[k]],
                     queries_per_member=[int((member == r).sum()) for r in range(len(devices))],
                     load_per_member=[int(cost[member == r].sum()) for r in range(len(devices))], largest_cost=int(cost.max()),
                     split_per_member=[blocks.finds_stats(grp.context(r)) for r in range(len(devices))],
                     over_one_context=round(g_times[k] / lib_s, 3))
        gix.free()
        grp.close()
    def spans(t):                                       # where the first triple begins and the last one ends
        return (t[0], t[-3] + t[-1] - 1, t[1], t[-2] + t[-1] - 1)
    want = None if want is None else {k: [(b, v, t, spans(t)) for b, v, t in recs] for k, recs in want.items()}
    mine = {name: [(f"p{h['seq']}", "%.1f" % (h["val"] / defaults.B_SCALE), segments(h["corners"].tolist()),
                    (h["a_rng"][0] + 1, h["a_rng"][1], h["b_rng"][0] + 1, h["b_rng"][1])) for h in hits]
            for (name, _, _, _), hits in zip(queries, got) if hits}
    bad = None if want is None else [name for name, _, _, _ in queries if mine.get(name, []) != want.get(name, [])]
    per_class = {}
    for (name, cls, src, _), hits in zip(queries, got):
        c = per_class.setdefault(cls, dict(queries=0, aligned=0, source_first=0))
        c["queries"] += 1
        c["aligned"] += bool(hits)
        c["source_first"] += bool(hits) and hits[0]["seq"] == src
    print(json.dumps({
        "what": "every record `spaln -Q7 -A0 -O4%s%s -a<db>` prints against one %s call" %
                (f" -M{args.max_out}" if args.max_out > 1 else "", " -pw" if args.all_out else "", "spdp_group_map_align_b" if group else "spdp_map_align_b"),
        "group": group, "rscr": rscr or None,
        "sequences": len(db), "queries": len(queries), "reference_aligned": None if want is None else len(want), "library_aligned": len(mine),
        "identical": None if bad is None else len(queries) - len(bad), "of": len(queries), "first_differing": None if bad is None else bad[:5],
        "reference_threads": args.threads, "reference_s": None if ref_s is None else round(ref_s, 3),
        "reference_default_engine_s": None if ref_default_s is None else round(ref_default_s, 3), "queries_whose_records_differ_without_A0": default_differs, "library_s": round(lib_s, 4),
        "library_s_all": [round(t, 4) for t in times], "index_load_s": round(load_s, 3), "format_s": round(format_s, 3), "library_index": build,
        "library_over_reference": None if ref_s is None else round(ref_s / lib_s, 2),
        "split": st, "vote_kernel_ms": round(ms, 3), "vote_queries_per_s": round(len(queries) / (ms * 1e-3), 1) if ms > 0 else None,
        "candidates_per_query": round(st["candidates"] / max(st["searched"], 1), 3), "per_class": per_class, "device": eng.device_name()}))
    eng.close()
    return 0 if not bad and (build is None or build["files_equal_outside_heap_bytes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
