"""Recipes for the vote of SrchBlk::finds on small protein databases (60 - 300 sequences, queries of 7 - 300 residues), each with
the effect it is built to have.  tests/test_finds_cases.py holds every recipe to its effect by the restatement alone
(tests/finds_restate.py); tests/test_finds_host.py runs them through the host emulation of the wave's logic,
tests/test_gpu_finds_cases.py through spdp_blk_finds, both against the restatement's records, int for int.

The indexes are made HERE, in plain Python, in the layout the library's reader gives (blk_nblk, blk_blkp, ...): one block per
sequence as `spaln -W -KA` writes them, a posting list per word = the blocks that hold it (ascending), a word score that falls
with the list's length, and -- what the program's builder does to words in too many blocks -- a list dropped while the score
stays (blkp = 0, wscr >= 0: "ubiquitous").  That keeps list lengths, table sizes and ties in the recipe's hand.  What the
PROGRAM's builder writes is covered by the fixtures under tests/golden/ (tests/test_finds_restate.py)."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import finds_restate as fr

AA = "ARNDCQEGHILKMFPSTWYV"
X_CODE = 2                                      # AMB of the reference's amino-acid alphabet; A = 3 .. V = 22


def encode(s: str) -> np.ndarray:
    return np.array([X_CODE if c == "X" else AA.index(c) + 3 for c in s], dtype=np.uint8)


def rand_protein(rng, n: int) -> str:
    return "".join(AA[i] for i in rng.integers(0, 20, size=n))


def mutate(rng, s: str, sub: float) -> str:
    return "".join(AA[rng.integers(0, 20)] if rng.random() < sub else c for c in s)


PATTERNS = {1: ["111"], 3: ["111", "1011"], 5: ["111", "1011", "10011"]}        # nbitpat -> the patterns of its kk = nbitpat / 2 + 1


def make_index(seqs, nshift=3, nbitpat=1, ubiq_over=None, maxblk=None, max_out=1, local=0, rbs_fact=0.0, rbs_base=0.5, max_mmc=15) -> dict:
    """the index of a list of protein strings; ubiq_over: a word in more blocks than this loses its list; maxblk: ContBlk::MaxBlk
    (default the longest list: a small run hash, which lives in the wave's LDS and has collisions to get right)"""
    nalpha, pats = 20, PATTERNS[nbitpat]
    weight = 3
    tabsize = nalpha ** weight
    kk = len(pats)
    exams = [[i for i, c in enumerate(p) if c == "1"] for p in pats]
    codes = [np.array([AA.index(c) if c in AA else 99 for c in s], dtype=np.int64) for s in seqs]
    lists = [dict() for _ in range(kk)]
    blk, chr_tab, spos = 0, [], 0
    for s in codes:
        chr_tab.append((spos, blk + 1))
        spos += len(s)
        if len(s) == 0:
            continue                            # (a sequence without residues has no block: its first block is the next one's)
        blk += 1
        for k, ex in enumerate(exams):
            for at in range(0, len(s) - len(pats[k]) + 1):
                r = s[[at + e for e in ex]]
                if (r >= nalpha).any():
                    continue
                w = int(r[0] * 400 + r[1] * 20 + r[2])
                lists[k].setdefault(w, set()).add(blk)
    chr_tab.append((spos, blk + 1))
    nseg = blk + 1
    # one table over all patterns, as the reference has it: a word's list is the union over the patterns that vote for it
    nblk = np.zeros(tabsize, dtype=np.uint16)
    wscr = np.full(tabsize, -1, dtype=np.int16)
    blkp = np.zeros(tabsize, dtype=np.int32)
    blkb = []
    merged = {}
    for k in range(kk):
        for w, bl in lists[k].items():
            merged.setdefault(w, set()).update(bl)
    longest = 1
    for w in sorted(merged):
        bl = sorted(merged[w])
        wscr[w] = max(1, int(100 * (math.log(nseg) - math.log(len(bl)))))
        if ubiq_over is not None and len(bl) > ubiq_over:
            continue
        nblk[w] = len(bl)
        blkp[w] = len(blkb) + 1
        blkb += bl
        longest = max(longest, len(bl))
    kept = wscr[blkp > 0]
    avrscr = max(1, int(kept.mean())) if kept.size else 1
    convtab = np.full(26, 20, dtype=np.uint8)
    convtab[3:23] = np.arange(20)
    bitpat = []
    for p, ex in zip(pats, exams):
        bitpat += [weight, len(p), 2 * (weight - 1)] + ex + [len(p) - 1 - e for e in reversed(ex)]
    maxblk = longest if maxblk is None else maxblk
    fx = dict(nalpha=nalpha, tabsize=tabsize, nshift=nshift, nbitpat=nbitpat, convts=26, n_chr=len(seqs), maxblk=maxblk, kk=kk, drna=0,
              nseg=nseg, minsigpr=3, ncand=max_out + 10, nascr=2, maxblock=1, extblock=1, extblockl=1, shortquery=8 * weight,
              hh_step=8, hb_size=37, hb_step=8, ha_size=31, ha_step=8, gdb=0, blklen=max([len(s) for s in seqs] + [1]),
              bclw=0.0, bcup=0.0, bcce=0.0, cfact=0.75, avrscr=avrscr, max_out=max_out, local=local,
              blk_convtab=convtab, blk_nblk=nblk, blk_wscr=wscr, blk_blkp=blkp, blk_blkb=np.array(blkb if blkb else [0], dtype=np.uint32),
              blk_chr=np.array(chr_tab, dtype=np.int32).reshape(-1), blk_bitpat=np.array(bitpat, dtype=np.int32))
    ix = restate_index(fx, rbs_fact=rbs_fact, rbs_base=rbs_base, max_mmc=max_mmc)
    # what SrchBlk::initialize derives, as the library's descriptor holds it
    fx.update(maxmmc=ix.maxmmc, hh_size=ix.hh_size, rbscoef=ix.rbscoef, rbscons=ix.rbscons, blk_rscrtab=np.array(ix.rscrtab, dtype=np.int32),
              ptpl=ix.ptpl, rlncoef=ix.rlncoef, rbs_fact=rbs_fact, rbs_base=rbs_base, max_mmc=max_mmc)
    return fx


def restate_index(fx: dict, **opts) -> fr.Index:
    o = dict(rbs_fact=fx.get("rbs_fact", 0.0), rbs_base=fx.get("rbs_base", 0.5), max_mmc=fx.get("max_mmc", 15))
    o.update(opts)
    return fr.index_from_arrays(fx, fx["avrscr"], max_out=fx["max_out"], local=fx["local"], **o)


# ---- the recipes: name -> dict(cls, fx, queries = [(codes, left, right)], tags, out_cap, check(recipe, results)) ------------------
def _db(rng, n, lo=100, hi=300):
    return [rand_protein(rng, int(rng.integers(lo, hi + 1))) for _ in range(n)]


def _top_is(src):
    def check(rcp, res):
        for (q, l, r), x, s in zip(rcp["queries"], res, src):
            assert x["flags"] == fr.REACHED and x["sigm"] > 0 and x["cands"][0] == s, (rcp["name"], s, x)
    return check


@functools.lru_cache(maxsize=None)
def recipes() -> dict:
    out = {}

    def add(name, cls, fx, queries, check, out_cap=64, tags=None):
        assert all(0 <= l <= r <= len(q) for q, l, r in queries), name
        out[name] = dict(name=name, cls=cls, fx=fx, queries=queries, check=check, out_cap=out_cap, tags=tags or [""] * len(queries))

    # 1. query lengths at every residue of (right - left) mod Nshift, and the three lengths around Nshift + width
    for nshift in (3, 2):
        rng = np.random.default_rng(100 + nshift)
        db = _db(rng, 80, 120, 300)
        fx = make_index(db, nshift=nshift, max_out=2)
        width = 3
        qs, src = [], []
        for i, ln in enumerate(list(range(40, 40 + 2 * nshift)) + list(range(95, 95 + 2 * nshift))):
            qs.append((encode(db[i][5:5 + ln]), 0, ln)); src.append(i)
        # a range inside a longer query: left / right are not the query's ends
        for i in range(4):
            s = db[20 + i]
            qs.append((encode(s), 7 + i, 7 + i + 50 + i)); src.append(20 + i)
        add(f"phase_ns{nshift}", "phase", fx, qs, _top_is(src))
        edge = [(encode(db[3][:ln]), 0, ln) for ln in (nshift + width - 1, nshift + width, nshift + width + 1)] * 4

        def check_edge(rcp, res, lim=nshift + width):
            for (q, l, r), x in zip(rcp["queries"], res):
                assert (x["flags"] == fr.SHORT) == (r - l - lim < 1), (rcp["name"], r - l, x)
        add(f"edge_ns{nshift}", "phase", fx, edge, check_edge)

    # 2. the two endings: the directions meet in round 0 (c < ptpl clamps rms) / the scan ends at maxmmc rounds
    rng = np.random.default_rng(2)
    # (a run ends once its words have scored base() = 3.6 avr, some four words: a pointer moves some 15 residues a round, both ends
    # together some 450 residues in maxmmc = 15 rounds -- the long queries have 700, beyond the 300 of the other recipes)
    db = _db(rng, 88, 120, 300) + _db(rng, 12, 700, 700)
    fx = make_index(db, max_out=1, rbs_fact=0.606, rbs_base=3.0)         # (the -yX0 constants: base() is large enough that ptpl > 0)
    ix = restate_index(fx)
    assert ix.ptpl > 0
    short = [(encode(db[i][10:10 + 7 + i]), 0, 7 + i) for i in range(12)]
    long_ = [(encode(mutate(rng, db[88 + i], 0.5)), 0, 700) for i in range(12)]

    def check_endings(rcp, res, maxmmc=ix.maxmmc):
        n1 = sum(x["nmmc"] == 1 for x in res[:12])
        assert n1 >= 6 and all(x["nmmc"] < maxmmc for x in res[:12]), [x["nmmc"] for x in res]
        assert all(x["nmmc"] == maxmmc for x in res[12:]), [x["nmmc"] for x in res]
    add("endings", "endings", fx, short + long_, check_endings, tags=["short"] * 12 + ["long"] * 12)

    # 3. ambiguous residues inside the first word of a run, and in the middle of one
    rng = np.random.default_rng(3)
    db = _db(rng, 90, 120, 300)
    fx = make_index(db, max_out=1)
    qs, src = [], []
    for i in range(12):
        s = list(db[i][:90])
        for at in ((0, 1, 2)[i % 3], 30 + i, 89 - (i % 3)):
            s[at] = "X"
        qs.append((encode("".join(s)), 0, 90)); src.append(i)
    for i in range(12, 22):
        s = "".join("X" if k % 10 == 9 else c for k, c in enumerate(db[i][:120]))
        qs.append((encode(s), 0, 120)); src.append(i)
    add("ambiguous", "ambiguous", fx, qs, _top_is(src))

    # 4. a ubiquitous word: a motif in so many sequences that its list is dropped while its score stays
    rng = np.random.default_rng(4)
    motif = "WCHMW"
    db = [s[:30] + motif + s[30:] if i % 2 == 0 else s for i, s in enumerate(_db(rng, 120))]
    fx = make_index(db, max_out=1, ubiq_over=40)
    words = [AA.index(motif[i]) * 400 + AA.index(motif[i + 1]) * 20 + AA.index(motif[i + 2]) for i in range(3)]
    assert all(fx["blk_blkp"][w] == 0 and fx["blk_wscr"][w] >= 0 for w in words)
    qs = [(encode(db[2 * i][20:80]), 0, 60) for i in range(12)]
    add("ubiquitous", "ubiquitous", fx, qs, _top_is([2 * i for i in range(12)]))

    # 5. posting lists of 63, 64, 65, 128 and 129 blocks for the words of a run
    for n_in in (63, 64, 65, 128, 129):
        rng = np.random.default_rng(500 + n_in)
        sixmer = "HWMCFY"
        db = _db(rng, 200, 60, 120)
        db = [s[:20] + sixmer + s[20:] if i < n_in else s.replace("HWM", "AAA").replace("WMC", "AAA").replace("MCF", "AAA").replace("CFY", "AAA")
              for i, s in enumerate(db)]
        fx = make_index(db, max_out=4)
        w0 = AA.index("H") * 400 + AA.index("W") * 20 + AA.index("M")
        assert fx["blk_nblk"][w0] == n_in, (fx["blk_nblk"][w0], n_in)
        qs = [(encode(db[i][14:14 + 18]), 0, 18) for i in range(10)]          # the 6-mer in every phase of the query's words

        def check_lists(rcp, res, n_in=n_in):
            for i, x in enumerate(res):
                assert x["sigm"] == 14 and x["cands"][0] == i, (rcp["name"], i, x)
                # (with the default constants base() is half a word's score: every block a word hits enters the heap, so the
                # heap is full; only its top is the recipe's to predict)
                assert x["heap"][0][0] == i + 1 and x["heap"][0][1] > x["heap"][1][1], x
        add(f"lists_{n_in}", "lists", fx, qs, check_lists)

    # 6. more than Ncand significant blocks: a family of 30 paralogs, MaxOut 1 and 4 -- the heap replaces its minimum
    for max_out in (1, 4):
        rng = np.random.default_rng(60 + max_out)
        anc = rand_protein(rng, 150)
        db = _db(rng, 100)
        fam = list(range(10, 40))
        for k in fam:
            db[k] = mutate(rng, anc, 0.10 + 0.01 * (k % 7))
        fx = make_index(db, max_out=max_out)
        qs = [(encode(mutate(rng, anc, 0.05 * (i % 4))), 0, 150) for i in range(10)]

        def check_family(rcp, res, max_out=max_out):
            for x in res:
                assert x["sigm"] == max_out + 10 and len(x["cands"]) == max_out, x
                assert all(10 < b <= 40 for b, _ in x["heap"][:max_out + 4]), x
        add(f"family_m{max_out}", "family", fx, qs, check_family)

    # 7. blocks with equal rscr at the edge of the MaxOut cut: a sequence planted under several names
    rng = np.random.default_rng(7)
    db = _db(rng, 90)
    for k in (50, 51, 52, 70):
        db[k] = db[5]
    for k in (60, 61):
        db[k] = db[6]
    qs = [(encode(db[5][i:i + 80]), 0, 80) for i in range(6)] + [(encode(db[6][i:i + 70]), 0, 70) for i in range(6)]
    for max_out in (1, 2, 4):
        fx = make_index(db, max_out=max_out)

        def check_ties(rcp, res, max_out=max_out):
            for i, x in enumerate(res):
                twins = 5 if i < 6 else 3
                top = [s for _, s in x["heap"][:twins]]
                assert len(set(top)) == 1 and x["heap"][twins][1] < top[0], (rcp["name"], i, x["heap"][:6])
                assert len(x["cands"]) == max_out
        add(f"ties_m{max_out}", "ties", fx, qs, check_ties)

    # 8. database sequences of 0, 1, 2 and `width` residues among the others
    rng = np.random.default_rng(8)
    db = _db(rng, 80)
    for k, ln in ((0, 0), (7, 1), (8, 2), (9, 3), (30, 0), (31, 0), (79, 2)):
        db[k] = db[k][:ln]
    fx = make_index(db, max_out=2)
    src = [1, 2, 10, 29, 32, 33, 40, 50, 60, 78, 77, 76]
    qs = [(encode(db[i][:60]), 0, min(60, len(db[i]))) for i in src]
    add("tiny_sequences", "tiny_sequences", fx, qs, _top_is(src))

    # 9. local = 1: maxmmc = INT_MAX, the scan ends where its two directions meet
    rng = np.random.default_rng(9)
    db = _db(rng, 70, 100, 300)
    fx = make_index(db, max_out=1, local=1)
    fx0 = make_index(db, max_out=1, local=0)
    qs = [(encode(mutate(rng, db[i], 0.3)), 0, len(db[i])) for i in range(10)]
    add("not_local", "local", fx0, qs, lambda rcp, res: None)

    def check_local(rcp, res, fx0=fx0):
        ix0 = restate_index(fx0)
        other = [fr.finds(ix0, q, l, r) for q, l, r in rcp["queries"]]
        assert all(x["nmmc"] >= y["nmmc"] for x, y in zip(res, other)) and any(x["nmmc"] > y["nmmc"] for x, y in zip(res, other))
        assert all(x["testword"][0] + x["testword"][1] >= y["testword"][0] + y["testword"][1] for x, y in zip(res, other))
    add("local", "local", fx, qs, check_local)

    # 10. other geometries: Nshift 1 and 4, two and three bit patterns (the last pattern scores but does not vote; two voting
    # lists are merged), the run hash of the program's size (in the slab, not in LDS)
    for name, kw in (("ns1", dict(nshift=1)), ("ns4", dict(nshift=4)), ("bp3", dict(nbitpat=3)), ("bp5", dict(nbitpat=5)),
                     ("bp5_ns2", dict(nbitpat=5, nshift=2)), ("bighash", dict(maxblk=17990))):
        rng = np.random.default_rng(sum(map(ord, name)))
        db = _db(rng, 120)
        fx = make_index(db, max_out=2, **kw)
        qs, src = [], []
        for i in range(10):
            qs.append((encode(mutate(rng, db[i], 0.1)[:40 + 20 * i]), 0, min(40 + 20 * i, len(db[i])))); src.append(i)
        add(f"geometry_{name}", "geometry", fx, qs, _top_is(src))

    # a malformed index: zeros inside posting lists.  A zero ends the list it stands in (Qwords::next_mrglist: a front of 0 is never
    # advanced); of two merged lists the other goes on.  One pattern, and three (two voting lists merged)
    for name, kw in (("bp1", dict()), ("bp5", dict(nbitpat=5))):
        rng = np.random.default_rng(1200 + len(kw))
        db = _db(rng, 150)
        fx = make_index(db, max_out=2, **kw)
        blkb = fx["blk_blkb"].copy()
        blkb[5::7] = 0
        clean = restate_index(fx)
        fx["blk_blkb"] = blkb
        qs = [(encode(mutate(rng, db[i], 0.05)[:100]), 0, 100) for i in range(10)]

        def check_zeros(rcp, res, clean=clean):
            other = [fr.finds(clean, q, l, r) for q, l, r in rcp["queries"]]
            assert all(x["flags"] == fr.REACHED for x in res) and any(x["heap"] != y["heap"] for x, y in zip(res, other))
        add(f"zeros_{name}", "zeros", fx, qs, check_zeros)

    # an out_cap too small for the record: SPDP_BLK_CUT (the only recipe that may come back flagged)
    rng = np.random.default_rng(11)
    db = _db(rng, 60)
    fx = make_index(db, max_out=1)
    add("cut", "cut", fx, [(encode(db[i]), 0, len(db[i])) for i in range(3)], lambda rcp, res: None, out_cap=8)
    return out


def names():
    return list(recipes())


@functools.lru_cache(maxsize=None)
def wanted(name: str):
    """the restatement's result of every query of a recipe, computed once"""
    rcp = recipes()[name]
    ix = restate_index(rcp["fx"])
    return [fr.finds(ix, q, l, r) for q, l, r in rcp["queries"]]


def wanted_record(x: dict, out_cap: int) -> list:
    """the record spdp_blk_finds writes for a result: cut to out_cap with SPDP_BLK_CUT when it does not fit"""
    rec = fr.record(x)
    if len(rec) > out_cap:
        rec = rec[:out_cap]
        rec[0] = out_cap
        rec[2] |= fr.CUT
    return rec


def lenadj_of(fx: dict) -> list:
    """per block Randbs::lencor(SegLen[blk]), as the restatement has it"""
    ix = restate_index(fx)
    return [ix.lencor(ix.seglen[b]) for b in range(fx["nseg"] + 1)]


def dump_index(fx: dict) -> str:
    """an index as tests/finds_host_check.cpp reads it"""
    ix = restate_index(fx)
    head = [fx["nalpha"], fx["tabsize"], fx["nshift"], fx["nbitpat"], fx["convts"], fx["n_chr"], fx["kk"], fx["nseg"], fx["ncand"],
            max(int(fx["maxblk"]), int(np.max(fx["blk_nblk"])), 1), fx["hh_size"], fx["hh_step"], fx["gdb"], fx["max_out"], fx["ptpl"], ix.maxmmc,
            len(fx["blk_blkb"]), len(fx["blk_bitpat"])]
    lines = ["INDEX " + " ".join(str(int(v)) for v in head),
             " ".join(repr(float(v)) for v in (fx["rbscoef"], fx["rbscons"], fx["bclw"], fx["bcup"], fx["bcce"], ix.app_c))]
    for key in ("blk_convtab", "blk_nblk", "blk_wscr", "blk_blkp", "blk_blkb", "blk_rscrtab", "blk_chr", "blk_bitpat"):
        lines.append(" ".join(str(int(v)) for v in np.asarray(fx[key]).reshape(-1)))
    lines.append(" ".join(str(v) for v in lenadj_of(fx)))
    return "\n".join(lines) + "\n"


def dump_query(case_id: int, q, left: int, right: int, out_cap: int, want: list) -> str:
    return (f"QUERY {case_id} {left} {right} {out_cap} {len(q)} " + " ".join(str(int(c)) for c in q) + f"\n{len(want)} " +
            " ".join(str(int(v)) for v in want) + "\n")
