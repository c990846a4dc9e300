"""Databases for the amino-acid index builder beyond what the program can be made to write (fixed seeds, a few ten thousand
residues each), with the parameters each is built with -- shared by the host checker's test and the device test, which both hold
the result to tests/aa_index_restate.py.  Also: what the library is handed for a case (codes, offsets, the class table)."""
import functools

import numpy as np

from tests import aa_index_restate as air

AA = air.AA


def _rand(rng, n, x_rate=0.01, odd_rate=0.004):
    s = [AA[i] for i in rng.integers(0, 20, size=n)]
    for i in np.flatnonzero(rng.random(n) < x_rate):
        s[i] = "X"
    for i in np.flatnonzero(rng.random(n) < odd_rate):
        s[i] = "UBZOJ"[int(rng.integers(0, 5))]
    return "".join(s)


def _db(seed, n=300, lo=5, hi=200):
    rng = np.random.default_rng(seed)
    db = [_rand(rng, int(k)) for k in rng.integers(lo, hi, size=n)]
    return [s if any(c not in "BZO" for c in s) else "A" + s for s in db]


def _prm(seqs, nalpha=20, **over):
    p = air.default_params(seqs, nalpha)
    p.update(over)
    if "ktuple" in over and "bitpat" not in over:
        p["bitpat"] = (1 << p["ktuple"]) - 1
    if "ktuple" in over and "nshift" not in over:
        p["nshift"] = p["ktuple"]
    return p


@functools.lru_cache(maxsize=None)
def case(name):
    """(sequences, parameters)"""
    if name in ("ns1", "ns2", "ns5"):
        db = _db(101 + int(name[2:]))
        return db, _prm(db, nshift=int(name[2:]))
    if name in ("k4", "k5"):
        db = _db(110 + int(name[1:]), n=400, hi=300)
        return db, _prm(db, ktuple=int(name[1:]))
    if name == "na12":
        db = _db(120)
        return db, _prm(db, nalpha=12)
    if name == "spaced":                                        # weight 3, width 5: positions 0, 1 and 4
        db = _db(121)
        return db, _prm(db, bitpat=0b10011)
    if name == "single":
        db = [_rand(np.random.default_rng(122), 9000, x_rate=0.002)]
        return db, _prm(db)
    if name == "exact_k":                                       # 5 000 sequences of exactly k residues
        rng = np.random.default_rng(123)
        db = ["".join(AA[i] for i in rng.integers(0, 20, size=3)) for _ in range(5000)]
        return db, _prm(db)
    if name == "slots":                                         # lengths of 17 and 33: a sequence start on every residue slot of a thread
        rng = np.random.default_rng(124)
        db = ["".join(AA[i] for i in rng.integers(0, 20, size=17 if i % 3 else 33)) for i in range(400)]
        assert {int(x) % 16 for x in np.cumsum([len(s) for s in db])} == set(range(16))
        return db, _prm(db)
    if name in ("afact1", "afact40"):
        db = _db(125)
        return db, _prm(db, afact=int(name[5:]))
    raise KeyError(name)


NAMES = ("ns1", "ns2", "ns5", "k4", "k5", "na12", "spaced", "single", "exact_k", "slots", "afact1", "afact40")


def class_table(nalpha):
    """the 26 ConvTab entries the library is given: the program's where ReducWord assigns them, X ambiguous, 0 / 1 / Asx skipped"""
    cls = air.a2r(nalpha)
    t = np.full(26, nalpha + 1, dtype=np.uint8)
    for i, ch in enumerate(AA):
        t[3 + i] = cls[ch]
    t[2], t[25] = nalpha, nalpha
    return t


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's index of a case or of a fixture ("a", "b", "edge", "wide": the program's own parameters)"""
    if name in NAMES:
        seqs, prm = case(name)
    else:
        seqs = air.golden_db(name)
        prm = air.default_params(seqs)
    return seqs, prm, air.build(seqs, prm)
