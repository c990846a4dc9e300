#!/usr/bin/env python3
"""Fixtures of map + align with several loci per query (`spaln -M N`): tests/golden/map_multi_par.{json,npz} (cDNA queries on a
genome with every gene twice, `spaln -W -KD`) and map_multi_p1.{json,npz} (protein queries, the translated index `spaln -W -KP`).

Build container only (needs oracle/_ref/spaln and oracle/_ref/spaln_blktap).  The genomes and queries are those of the block-search
generators (make_blk_goldens.py: paralog_genome_and_queries, protein_genome_and_queries) for the seeds below; the reference formats
the genome (no -t: the builder's threaded = 0) and maps the queries with -Q7 -O4 -M4 and a raised output threshold -H, with and
without -pw (cDNA: with -S1 and in both orientations).  Recorded:
  * .json: per run (S1, S3: cDNA with -S1 / in both orientations; P: protein; _pw: with -pw) the records the program PRINTED
    for every query, in print order (chromosome, strand, exon table), and their scores (the summary line's S:);
  * .npz: the parameters the program held (spaln_blktap on the first query: the block search's find_prm / blk_prm, the HSP-search
    model, the IntPen table, the intron-length limits) and the index build's inputs (FASTA size, threaded).
The test (tests/test_gpu_map_multi.py) regenerates the genome from the seeds and builds the index with the library's builder.

    python tests/golden/make_map_multi_goldens.py [name ...]
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_blk_goldens as mb  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.dirname(os.path.abspath(__file__))
PARAM_KEYS = ("blk_prm", "find_prm", "find_intpen", "cli_intron_prm", "wl_levels", "wl_bitpat", "wl_convtab", "wl_mtx", "wl_glob")
# name, protein, (n_genes, n_chr, seed), -H, orientations
CASES = (("map_multi_par", False, (60, 2, 1300), 1200, ("-S1", "")),
         ("map_multi_p1", True, (40, 2, 1400), 395, ("",)))      # (-H395: q14 prints a locus the threshold dropped, ahead of a kept one)
MAX_OUT = 4


def main():
    from e2e_q7 import reference_loci
    from tests import spdg
    only = sys.argv[1:]
    for name, prot, (n_genes, n_chr, seed), thr, oris in CASES:
        if only and name not in only:
            continue
        chroms, queries = (mb.protein_genome_and_queries if prot else mb.paralog_genome_and_queries)(n_genes, n_chr, seed)
        with tempfile.TemporaryDirectory() as td:
            with open(os.path.join(td, "gnm.mfa"), "w") as f:
                for c, s in enumerate(chroms):
                    f.write(f">chr{c + 1}\n")
                    t = bytes(s).decode()
                    f.writelines(t[i:i + 60] + "\n" for i in range(0, len(t), 60))
            with open(os.path.join(td, "q.fa"), "w") as f:
                for i, s in enumerate(queries):
                    f.write(f">q{i}\n{bytes(s).decode()}\n")
            with open(os.path.join(td, "one.fa"), "w") as f:
                f.write(f">q0\n{bytes(queries[0]).decode()}\n")
            env = dict(os.environ, ALN_TAB=os.path.join(REF, "table"), ALN_DBS=td)
            subprocess.run([os.path.join(REF, "spaln"), "-W", "-KP" if prot else "-KD", "gnm.mfa"], cwd=td, env=env, check=True, capture_output=True)
            opts = ["-Q7", "-O4", "-t1", f"-M{MAX_OUT}", f"-H{thr}"]
            runs, scores, prm = {}, {}, None
            for ori in oris:
                log = os.path.join(td, "prm.spdg")
                subprocess.run([os.path.join(REF, "spaln_blktap")] + opts + ([ori] if ori else []) + ["-dgnm", "one.fa"], cwd=td,
                               env=dict(env, SPDP_BLK_LOG=log), check=True, capture_output=True)
                fx = spdg.load(log)
                got = {k: np.asarray(fx[k]) for k in PARAM_KEYS}
                assert prm is None or all(np.array_equal(prm[k], got[k]) for k in PARAM_KEYS), "parameters differ between orientations"
                prm = got
                for pw in ("", "-pw"):
                    r = subprocess.run([os.path.join(REF, "spaln")] + opts + ([ori] if ori else []) + ([pw] if pw else []) + ["-dgnm", "q.fa"],
                                       cwd=td, env=env, check=True, capture_output=True, text=True)
                    loci = reference_loci(r.stdout)
                    key = ("P" if prot else (ori or "-S3").lstrip("-")) + pw.replace("-", "_")
                    runs[key] = {q: [[c, s, [list(e) for e in ex]] for c, s, ex in v] for q, v in loci.items()}
                    # the score of every printed record (the summary line's S:, Gsinfo::scr / scale; NEVSEL / scale for a locus the
                    # threshold dropped that was printed all the same)
                    scores[key] = {}
                    for line in r.stdout.splitlines():
                        if line.startswith("@"):
                            scores[key].setdefault(re.search(r"\) (\S+) \[", line).group(1), []).append(float(re.search(r" S: (\S+)", line).group(1)))
            setup = dict(protein=prot, n_genes=n_genes, n_chr=n_chr, seed=seed, fasta_bytes=os.path.getsize(os.path.join(td, "gnm.mfa")),
                         threaded=0, max_out=MAX_OUT, max_out2=MAX_OUT, H=thr, options=" ".join(opts), n_queries=len(queries),
                         chr_names=[f"chr{c + 1}" for c in range(n_chr)])
            with open(os.path.join(OUT, name + ".json"), "w") as f:
                json.dump(dict(setup=setup, runs=runs, scores=scores), f, indent=0, sort_keys=True)
            np.savez_compressed(os.path.join(OUT, name + ".npz"), **prm)
            for k, v in runs.items():
                base = runs[k.replace("_pw", "")]
                print(f"{name} {k}: {sum(len(x) for x in v.values())} records for {len(v)} queries; "
                      f"{sum(1 for q in v if len(v[q]) != len(base.get(q, [])))} queries whose list -pw changes; printed though dropped: "
                      f"{[q for q, x in scores[k].items() if '_pw' not in k and min(x) <= thr]}")


if __name__ == "__main__":
    main()
