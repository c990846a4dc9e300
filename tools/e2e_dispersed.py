#!/usr/bin/env python3
"""Dispersed loci end to end: what `spaln -pr` prints of queries whose parts lie in different places, against the library's
spdp_map_align_s_dispersed / _h_dispersed.

    python tools/e2e_dispersed.py [--joined 120] [--controls 30] [--genes 40] [--ori 1|3] [--tails] [--protein]
                                                                       (an MI355X box; oracle/_ref for the comparison)

The data set of tools/dropin_demo.py (a synthetic genome with planted multi-exon genes, formatted by the compiled reference's
own `spaln -W`); the queries are JOINED transcripts of two different genes, by a fixed seed, in three classes --

    0  whole + whole                1  whole + first third                2  last quarter + whole

-- followed by unjoined controls.  Two runs:

  * reference:  oracle/_ref/spaln -Q7 [-S1] -O4 -pr -t<threads> -dgnm q.fa      (algmode.mlt = 1: quick4 searches the genome again
                with what the first alignment left uncovered on each side)
  * library:    ONE spdp_map_align_s_dispersed call (with --tails through its prep argument; --protein: _h_dispersed on fused
                proteins against the translated index), then spdp_map_align_s / _h on the same queries: the entry that reports
                one locus per query.  min_seg_len = 2 Ktuple + Nshift of the index as the program's recorder holds them.

--ori 3 runs the program in its default orientation with every query in sense (what the program does after a locus aligned
with the query reverse-complemented is not reproduced: include/spdp.h).  Compared: per query the LIST of records in print order
(chromosome, strand, exon table).  One JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dropin_demo  # noqa: E402
from e2e_q7 import add_tails, cli_parameters, loci_of, read_fasta, reference_loci  # noqa: E402
from spaln_amd import abi, blocks, engine, synth  # noqa: E402
from tests import spdg  # noqa: E402


def shares_a_word(a, b, k=24):
    """two mutated copies of one transcript share a k-mer; transcripts of different genes do not"""
    words = {a[i:i + k] for i in range(0, len(a) - k + 1)}
    return any(b[i:i + k] in words for i in range(0, len(b) - k + 1))


def write_queries(path, joined, controls, seed, protein):
    """q.fa (2 joined + controls single transcripts, one per line pair) rewritten in place: `joined` joined queries j<k>_<class>,
    then the controls c<k>.  -> (names of the joined ones, names of the controls)"""
    rng = np.random.default_rng(seed)
    seqs = [ln for ln in open(path).read().split("\n")[1::2] if ln]
    assert len(seqs) == 2 * joined + controls, (len(seqs), joined, controls)
    pool, ctl = seqs[:2 * joined], seqs[2 * joined:]
    k_word = 8 if protein else 24
    out, jn, cn = [], [], []
    for k in range(joined):
        a, b = pool[2 * k], pool[2 * k + 1]
        for _ in range(50):                                  # (the partner must come from another gene)
            if not shares_a_word(a, b, k_word):
                break
            b = pool[int(rng.integers(0, len(pool)))]
        cls = k % 3
        if cls == 1:
            b = b[:len(b) // 3]
        elif cls == 2:
            a = a[len(a) - len(a) // 4:]
        name = f"j{k}_{cls}"
        jn.append(name)
        out.append(f">{name}\n{a + b}\n")
    for k, s in enumerate(ctl):
        cn.append(f"c{k}")
        out.append(f">c{k}\n{s}\n")
    open(path, "w").write("".join(out))
    return jn, cn


def rests_of(want):
    """the program's records that came from a rest: (left, right) -- of three records the second is the left rest's and the third the
    right one's; of two the second is a left rest's when it begins in front of the first one on the query"""
    left = right = 0
    for recs in want.values():
        if len(recs) == 3:
            left += 1
            right += 1
        elif len(recs) == 2 and recs[0][2] and recs[1][2]:
            lo = [min(min(e[0], e[1]) for e in r[2]) for r in recs]
            if lo[1] < lo[0]:
                left += 1
            else:
                right += 1
    return left, right


def parts_against_rests(lib, lists, covered, ranges, turned, min_seg_len):
    """`part` and `covered` against quick4's rule and blkaln's narrowing.
      * a query's first record has part 0 and the parts ascend;
      * where the first search aligned ONE locus (n_loci = 1) and reports it, `covered` is known exactly: the range of that record,
        [first exon's rleft, last exon's rright) (src/spaln.cc:950-954) -- with more loci it is what the last one that passed left,
        which the output does not tell;
      * a record of part 1 / 2 exists only where spdp_dispersed_rests gives a left / right rest for `covered`.  Its FAR end -- the one
        at the query's own boundary -- lies inside that rest.  Its NEAR end, the one towards the covered stretch, may overhang, in
        the program too: the block search looks for words inside the range, but Wlp::eval extends an HSP back to the query's first
        residue and forward to its tlen whatever the range is (src/wln.cc:365-367, 383, 394, 404), and the alignment keeps what the
        HSP took -- a residue or two of chance matches, or as much of a gene as the covered stretch had cut into.  The overhang is
        held below the part of the record that lies inside the rest: a record belongs to the rest its larger part lies in.
    -> (queries where any of this does not hold, queries whose `covered` was held exactly, rest records that overhang, the longest
    overhang).  (turned[i]: the preparation reverse-complemented query i -- the program's left is then the right of the query as
    given, in whose positions ranges and covered are)"""
    bad, exact, outside, longest = [], 0, 0, 0
    for i, lst in enumerate(lists):
        org = tuple(int(x) for x in ranges[i])
        cov = tuple(int(x) for x in covered[i])
        by_part = {}
        for r in engine.dispersed_rests(lib, org, cov, min_seg_len):
            as_given = 1 if (r[0] == org[0] and r[1] == cov[0]) else 2          # (the left rest ends where the covered stretch begins)
            by_part[3 - as_given if turned[i] else as_given] = (r, as_given)
        parts = [g["part"] for g in lst]
        if parts and (parts[0] != 0 or parts != sorted(set(parts))):
            bad.append(i)
        if lst and lst[0]["n_loci"] == 1:
            pos = [p for e in lst[0]["exons"] for p in e[:2]]
            exact += 1
            if (min(pos) - 1, max(pos)) != cov:
                bad.append(i)
        if not lst and cov != org:
            bad.append(i)
        for g in lst[1:]:
            r, side = by_part.get(g["part"], (None, 0))
            pos = [p for e in g["exons"] for p in e[:2]]
            if r is None or not pos:
                bad.append(i)
                continue
            lo, hi = min(pos) - 1, max(pos)
            far_inside = lo >= r[0] if side == 1 else hi <= r[1]
            over = max(0, hi - r[1]) if side == 1 else max(0, r[0] - lo)
            inside = min(hi, r[1]) - max(lo, r[0])
            if not far_inside or inside <= 0 or over >= inside:
                bad.append(i)
            outside += over > 0
            longest = max(longest, over)
    return sorted(set(bad)), exact, outside, longest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--joined", type=int, default=120)
    ap.add_argument("--controls", type=int, default=30)
    ap.add_argument("--genes", type=int, default=40)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--show", type=int, default=3)
    ap.add_argument("--ori", type=int, default=1, choices=[1, 3], help="1: `spaln -S1`; 3: the program's default orientation (queries in sense)")
    ap.add_argument("--tails", action="store_true", help="poly-A tails on a third of the queries (tools/e2e_q7.py --tails); the library prepares them")
    ap.add_argument("--planted-a", type=int, default=20)
    ap.add_argument("--protein", action="store_true", help="fused proteins against the translated index: spdp_map_align_h_dispersed")
    ap.add_argument("--repeat", type=int, default=2, help="calls of the entry (the first one of a context also loads the code objects)")
    ap.add_argument("--dump-diff", default="")
    ap.add_argument("--reference-only", action="store_true", help="the program's side alone: what the data set makes it print (needs no device)")
    args = ap.parse_args()
    if args.protein and (args.tails or args.ori != 1):
        ap.error("--protein takes neither --tails nor --ori")
    args.queries = 2 * args.joined + args.controls
    t_all = time.perf_counter()
    with tempfile.TemporaryDirectory(prefix="spdp_e2e_d_") as td:
        genome_nt, env = dropin_demo.make_dataset(td, args)
        qfa = os.path.join(td, "q.fa")
        joined, controls = write_queries(qfa, args.joined, args.controls, args.seed, args.protein)
        if args.tails:
            add_tails(qfa, args.ori)
        strand = ["-S1"] if args.ori == 1 and not args.protein else []
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(dropin_demo.REF, "spaln"), "-Q7"] + strand + ["-O4", "-pr", f"-t{args.threads}", "-dgnm", "q.fa"],
                           cwd=td, env=env, capture_output=True, text=True)
        ref_s = time.perf_counter() - t0
        if r.returncode:
            raise SystemExit("reference run failed: " + r.stderr[-300:])
        want = reference_loci(r.stdout)
        if args.reference_only:
            left, right = rests_of(want)
            print(json.dumps({"what": "the program alone (no device)", "reference_records": sum(len(v) for v in want.values()), "reference_queries": len(want),
                              "reference_left_rest_records": left, "reference_right_rest_records": right,
                              "joined_with_two_or_more_records": sum(1 for k in joined if len(want.get(k, [])) >= 2),
                              "controls_with_one_record": sum(1 for k in controls if len(want.get(k, [])) == 1), "reference_wall_s": round(ref_s, 2)}))
            return

        eng = engine.Engine(0)
        lib = eng.lib
        cli = cli_parameters(td, env, strand)
        min_seg_len = 2 * int(cli["blk_prm"][1]) + int(cli["blk_prm"][5])       # SrchBlk::MinQuery(): 2 Ktuple + Nshift
        model = abi.wilip_model_from_fixture(cli)
        chr_names, chroms = read_fasta(os.path.join(td, "gnm.mfa"))
        gen = np.concatenate(chroms).astype(np.uint8)
        off = np.array([0] + list(np.cumsum([len(c) for c in chroms])), dtype=np.int64)
        ip = np.ascontiguousarray(cli["find_intpen"], dtype=np.int16)
        llmt, minl, _rlmt, maxl = (int(x) for x in cli["cli_intron_prm"][:4])
        fx = blocks.read_index_file(lib, os.path.join(td, "gnm.bkp" if args.protein else "gnm.bkn"), ext_block=int(cli["blk_prm"][blocks._PRM["extblock"]]))
        fx["blk_convtab"][:2] = 255
        dix = blocks.BlockIndex(eng, fx)
        prm = blocks.find_params_from_fixture(cli)
        prm.phase1t = int(dix.desc.rbscons)
        if args.protein:
            q_names, q_raw = [], []
            for blk_ in open(qfa).read().split(">")[1:]:
                nm, seq = blk_.split("\n", 1)
                q_names.append(nm.split()[0]); q_raw.append(seq.replace("\n", ""))
            queries = [synth.encode_protein(np.frombuffer(s_.encode(), dtype=np.uint8)) for s_ in q_raw]
            qh = "live_h_q7555.spdg" if model.crs else "qh_0013.spdg"
            fq = spdg.load(os.path.join(ROOT, "tests", "golden", qh))
            fsig = fq if "pm5_f32" in fq else spdg.load(os.path.join(ROOT, "tests", "golden", "h1_basic.spdg"))
            sc = spdg.scoring_h(fq, intpen=ip, llmt=llmt, minl=minl)
            sc.scalar_engines = 1
            sp = abi.seed_params_from_fixture(fq)
            sp.qck, sp.minl, sp.ip_maxl = 3, minl, maxl
            sigmodel = abi.signal_model_h_from_fixture(fsig)
            rp = [int(x) for x in fq["rparams"]]
            hp = dict(zip(spdg.HPARAM_NAMES, (int(x) for x in fq["hparams"])))
            rescore = abi.RescoreParamsH(minl, rp[4], hp["lcl"], rp[1])
            sp.wilip = C.addressof(model)
            call = lambda: blocks.map_align_h_dispersed(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, min_seg_len) + (None,)  # noqa: E731
            single = lambda: blocks.map_align_h(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries)[0]  # noqa: E731
        else:
            q_names, queries = read_fasta(qfa)
            fq = spdg.load(os.path.join(ROOT, "tests", "golden", "q_c2_seed0.spdg"))
            sigmodel = abi.signal_model_from_fixture(fq)
            sc = spdg.scoring(fq, intpen=ip, scalar_engines=1, llmt=llmt, minl=minl)
            sp = abi.seed_params_from_fixture(fq)
            sp.minl, sp.ip_maxl = minl, maxl
            sp.wilip = C.addressof(model)
            fs = fq["rng_fstat_A0"] if "rng_fstat_A0" in fq else [0, 0, 0, 0, 0, 0, 3, 1]
            rescore = (fq["prm"]["codonk1"], minl, int(fs[6]), int(fs[7]))
            prep = (args.ori, 12) if args.tails else None
            call = lambda: blocks.map_align_dispersed(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, min_seg_len, ori=args.ori, prep=prep)  # noqa: E731
            if args.tails:
                single = lambda: blocks.map_align_prep(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, q_mns=args.ori, polya_thr=12)[0]  # noqa: E731
            else:
                single = lambda: blocks.map_align(dix, gen, off, sc, sp, sigmodel, prm, rescore, queries, ori=args.ori)[0]  # noqa: E731
        runs = []
        for _ in range(max(1, args.repeat)):
            t0 = time.perf_counter()
            lists, covered, phases, rc, recs = call()
            runs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ones = single()
        single_s = time.perf_counter() - t0

        got = {q_names[i]: v for i, v in enumerate(loci_of(lists, chr_names)) if v}
        one = {q_names[i]: (chr_names[g["chr"]], "-" if g["rvs"] else "+", [tuple(e) for e in g["exons"]]) for i, g in enumerate(ones) if g is not None}
        names = sorted(set(want) | set(got))
        same = [k for k in names if want.get(k) == got.get(k)]
        diff = [k for k in names if want.get(k) != got.get(k)]
        for k in diff[:args.show]:
            sys.stderr.write(f"{k}\n  reference {want.get(k)}\n  library   {got.get(k)}\n")
        if args.dump_diff:
            os.makedirs(os.path.dirname(os.path.abspath(args.dump_diff)), exist_ok=True)
            gi = {q_names[i]: (v, [int(x) for x in covered[i]]) for i, v in enumerate(lists)}
            json.dump([{"name": k, "reference": want.get(k), "library": got.get(k), "library_genes": gi.get(k)} for k in diff],
                      open(args.dump_diff, "w"), indent=1)
        # the range of every query's first search, in positions of the query as given
        if recs is not None:
            turned = [int(recs[i][0]) == 2 for i in range(len(queries))]
            ranges = [((len(queries[i]) - int(recs[i][3]), len(queries[i]) - int(recs[i][2])) if turned[i] else (int(recs[i][2]), int(recs[i][3])))
                      for i in range(len(queries))]
        else:
            turned = [False] * len(queries)
            ranges = [(0, len(q)) for q in queries]
        left, right = rests_of(want)
        inconsistent, exact, outside, longest = parts_against_rests(lib, lists, covered, ranges, turned, min_seg_len)
        for i in inconsistent[:args.show]:
            sys.stderr.write(f"{q_names[i]}: range {ranges[i]}, covered {covered[i].tolist()}, parts " +
                             ", ".join(f"{g['part']}: {g['exons'][0][0]}..{g['exons'][-1][1]}" for g in lists[i]) + "\n")
        print(json.dumps({
            "what": "every record `spaln -Q7 %s-O4 -pr` prints against %s" % ("-S1 " if strand else "", "spdp_map_align_h_dispersed" if args.protein else
                                                                          "spdp_map_align_s_dispersed"),
            "query_type": "protein" if args.protein else "cDNA", "ori": args.ori, "tails": bool(args.tails), "min_seg_len": min_seg_len,
            "joined": len(joined), "controls": len(controls), "genome_nt": genome_nt,
            "reference_records": sum(len(v) for v in want.values()), "library_records": sum(len(v) for v in got.values()),
            "reference_queries": len(want), "library_queries": len(got),
            "identical_record_lists": len(same), "different": len(diff), "queries": len(q_names),
            "identical_of_all_queries": sum(1 for k in q_names if want.get(k) == got.get(k)),
            "reference_left_rest_records": left, "reference_right_rest_records": right,
            "joined_with_two_or_more_records": sum(1 for k in joined if len(want.get(k, [])) >= 2),
            "controls_with_one_record_equal_to_the_single_entry": sum(1 for k in controls if len(want.get(k, [])) == 1 and len(got.get(k, [])) == 1 and
                                                                      got[k][0] == one.get(k) and want[k][0] == one.get(k)),
            "single_entry_fewer_records": sum(1 for k in q_names if (1 if k in one else 0) < len(want.get(k, []))),
            "parts_inconsistent": inconsistent, "covered_held_exactly": exact, "rest_records_reaching_outside_their_range": outside,
            "longest_overhang": longest, "turned_by_the_preparation": sum(turned),
            "reference_wall_s": round(ref_s, 2), "reference_threads": args.threads,
            "library_s": {"dispersed_call": round(runs[-1], 3), "first_call": round(runs[0], 3), "single_entry_call": round(single_s, 3),
                          "find": round(phases[0], 3), "regions_and_signals": round(phases[1], 3), "align": round(phases[2], 3),
                          "rescore": round(phases[3], 3)},
            "return_code": rc, "wall_s": round(time.perf_counter() - t_all, 1)}))
        dix.free()
        eng.close()


if __name__ == "__main__":
    main()
