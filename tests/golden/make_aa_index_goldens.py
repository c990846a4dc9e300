"""Fixtures of the amino-acid index builder from the program itself: runs where oracle/_ref/spaln is built (make -C oracle/ref_build)
and writes DATA only --
    tests/golden/aa_idx_<set>.bka.gz    the index `spaln -W -KA -t1` wrote of the set's database
    tests/golden/aa_idx_<set>.json.gz   {"set": .., "db": [the sequences, as the letters of the FASTA file]}

    python tests/golden/make_aa_index_goldens.py [--sets edge wide]

The script stops with a message unless the program's file shows what the set is there for (see `require`)."""
import argparse
import gzip
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "spaln")
ENV = dict(os.environ, ALN_TAB=os.path.join(ROOT, "oracle", "_ref", "table"))
AA = "ARNDCQEGHILKMFPSTWYV"
TILE = 4096                                                     # residues per workgroup of the library's words pass


def rand_protein(rng, n):
    return "".join(AA[i] for i in rng.integers(0, 20, size=n))


def make_edge():
    """k = 3: what the per-residue rule can get wrong, one sequence each, then a few hundred ordinary ones"""
    rng = np.random.default_rng(31)
    head = "MKW"                                                # at the start of (nearly) every sequence: a word in every block
    long_x = list(head + rand_protein(rng, 9000 - 3))
    long_x[TILE - 1] = "X"                                      # the sequence starts on a tile boundary: the last residue of that tile
    db = [head + rand_protein(rng, TILE - 3),                   # 4096: the next sequence starts on a tile boundary
          head + rand_protein(rng, TILE - 1 - 3),               # 4095
          head + rand_protein(rng, TILE + 1 - 3),               # 4097: three sequences = three tiles, the next starts on a boundary
          "".join(long_x),                                      # two tile boundaries inside, an X as a tile's last residue
          head + rand_protein(rng, 66000),                      # no X: the run counter (16 bits) wraps
          "A", "AR", "ARN", "ARND",
          "X" + head + rand_protein(rng, 20), head + rand_protein(rng, 20) + "X",
          "".join("X" if i % 3 == 2 else c for i, c in enumerate(head + rand_protein(rng, 30))),
          head + "ARNXXXXDCQEGXXHILKMXFPSTW", "XXXX" + head, "X",
          head + "ARNDUCQEGHUU" + rand_protein(rng, 9),
          head + "ARBNDZCQOEGJHILBBKMFZOJPST", "B" + head + "Z", "JJJJJJ" + head,
          "A" * 40, head + "W" * 25]
    twin = head + rand_protein(rng, 57)
    db += [twin, twin]
    for _ in range(320):
        db.append(head + rand_protein(rng, int(rng.integers(9, 70))))
    for i in range(len(db) - 40, len(db), 5):                   # ... some of them with the letters of no class
        s = list(db[i])
        for j, ch in zip(rng.integers(3, len(s), size=4), "XBZJ"):
            s[j] = ch
        db[i] = "".join(s)
    return db


def make_wide():
    """more than 65 535 sequences (BytBlk 4), at least 620 000 counted residues (Ktuple 4, Nshift 4)"""
    rng = np.random.default_rng(37)
    db = [rand_protein(rng, int(n)) for n in rng.integers(6, 13, size=66200)]
    for i in rng.choice(len(db), size=100, replace=False):
        db[int(i)] = rand_protein(rng, int(rng.integers(900, 1100)))
    for i in rng.choice(len(db), size=300, replace=False):      # X, and letters of no class, in short sequences too
        s = list(db[int(i)])
        s[int(rng.integers(0, len(s)))] = "XXBZUJ"[int(rng.integers(0, 6))]
        if any(c in AA for c in s):
            db[int(i)] = "".join(s)
    return db


SETS = {"edge": make_edge, "wide": make_wide}


def require(cond, msg):
    if not cond:
        sys.exit("make_aa_index_goldens: the program's file does not show what the set is there for: " + msg)


def header(raw):
    nalpha, ktuple, _, tabsize, _, nshift, blklen, _, nbitpat, _ = struct.unpack_from("<8IhH", raw, 0)
    _, _, wordno, _, chrno, glen, _, _, bytblk, _ = struct.unpack_from("<II4Q4H", raw, 36)
    at = 36 + 88 + 24 + 8 * (chrno + 1)
    chrid = np.frombuffer(raw, dtype="<u4", count=2 * (chrno + 1), offset=36 + 88 + 24)
    nblk = np.frombuffer(raw, dtype="<u2", count=tabsize, offset=at)
    blkp = np.frombuffer(raw, dtype="<i4", count=tabsize, offset=at + 2 * tabsize)
    wscr = np.frombuffer(raw, dtype="<i2", count=tabsize, offset=at + 6 * tabsize + bytblk * wordno)
    return dict(ktuple=ktuple, nshift=nshift, blklen=blklen, chrno=chrno, glen=glen, bytblk=bytblk, chrid=chrid, nblk=nblk, blkp=blkp, wscr=wscr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="*", default=list(SETS))
    args = ap.parse_args()
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/spaln is not built (make -C oracle/ref_build)")
    for name in args.sets:
        db = SETS[name]()
        td = tempfile.mkdtemp(prefix="aa_idx_gold_")
        try:
            with open(os.path.join(td, "prot.faa"), "w") as f:
                for i, s in enumerate(db):
                    f.write(f">p{i}\n{s}\n")
            r = subprocess.run([REF, "-W", "-KA", "-t1", "prot.faa"], cwd=td, env=ENV, capture_output=True, text=True)
            if r.returncode or not os.path.exists(os.path.join(td, "prot.bka")):
                sys.exit("spaln -W -KA failed: " + r.stderr[-500:])
            raw = open(os.path.join(td, "prot.bka"), "rb").read()
            h = header(raw)
            counted = [sum(1 for c in s if c not in "BZO") for s in db]
            require(h["chrno"] == len(db) and h["glen"] == sum(counted), "the letters of no class are not skipped, or a sequence is missing")
            require(h["blklen"] == max(counted), "blklen is not the longest sequence")
            require(int(h["chrid"][-1]) == len(db) + 1, "a sequence without a block")
            starts = h["chrid"][0::2]
            if name == "edge":
                require(h["ktuple"] == 3 and h["nshift"] == 3 and h["bytblk"] == 2, "k = 3 with 2-byte block numbers")
                require(h["blklen"] > 65536 + 3, "no sequence long enough for the run counter to wrap")
                require(sum(1 for s in starts[1:-1] if s % TILE == 0) >= 2, "no sequence start on a tile boundary")
                x_at = int(starts[3]) + TILE - 1
                require(x_at % TILE == TILE - 1 and db[3][TILE - 1] == "X", "no X as the last residue of a tile")
                lost = (h["wscr"] >= 0) & (h["blkp"] == 0)
                require(lost.any(), "no word that lies in so many sequences that it loses its list")
                require({len(s) for s in db} >= {1, 2, 3, 4}, "sequences of 1 .. 4 residues")
            if name == "wide":
                require(h["ktuple"] == 4 and h["nshift"] == 4 and h["bytblk"] == 4, f"k = 4 with 4-byte block numbers, not {h['ktuple'], h['bytblk']}")
            for fn, data in ((f"aa_idx_{name}.json.gz", json.dumps(dict(set=name, db=db), separators=(",", ":")).encode()), (f"aa_idx_{name}.bka.gz", raw)):
                with gzip.GzipFile(os.path.join(HERE, fn), "wb", mtime=0) as f:
                    f.write(data)
                print(name, fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")
            print(name, "sequences", len(db), "residues", h["glen"], "k", h["ktuple"], "BytBlk", h["bytblk"], "postings", int(h["nblk"].sum()))
        finally:
            shutil.rmtree(td, ignore_errors=True)


if __name__ == "__main__":
    main()
