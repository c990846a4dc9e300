"""SrchBlk::finds restated plainly (ogotoh/spaln v3.0.7 src/blksrc.cc:3271-3362) with what it is built from: init2 (:1925-1938),
Bhit2 (:3147-3179) over PrQueue<BlkScr> (src/clib.h:446-565), the run hash Dhash<INT,int>(2 MaxBlk, 0) (src/clib.h:193-355),
Randbs::randbs / lencor / base (:2047-2069, src/blksrc.h:459-461), setSegLen (:1966-1983), findChrNo (:1985-2002), the
one-argument Qwords::querywords (:2836-2878) and init_mrglist / next_mrglist (:2938-2969).  Sequential, one query at a time, every
container with the semantics the results depend on spelled out.  It uses nothing of the product's code: an index is the dict of
arrays a reference-side dump holds (blk_nblk, blk_blkp, ...) plus the scalars named in `Index`.

The checker of the device vote (tests/test_gpu_finds_cases.py) and of its host emulation (tests/test_finds_host.py); itself held
to the program's printed records by tests/test_finds_restate.py."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

REACHED, CUT, TABLE, SHORT = 1, 2, 4, 16
ERROR = -1
INT_MAX = 2 ** 31 - 1


def f32(x: float) -> float:
    return float(np.float32(x))


def supprime(n: int) -> int:
    """the smallest prime >= n (src/supprime.cc:375)"""
    if n <= 3:
        return n
    n |= 1
    while True:
        x = 3
        while x * x <= n and n % x:
            x += 2
        if x * x > n:
            return n
        n += 2


@dataclass
class Index:
    """what SrchBlk holds of a -KA index after initialize (:2179-2226) with gnmdb = false"""
    nalpha: int
    tabsize: int
    nshift: int
    nbitpat: int
    n_chr: int
    maxblk: int
    nseg: int                   # chrblk(ChrNo): sequences + 1 when every sequence is one block
    avrscr: int
    convtab: np.ndarray
    nblk: np.ndarray
    wscr: np.ndarray
    blkp: np.ndarray            # offset of the word's list in blkb + 1, 0 = none
    blkb: np.ndarray
    chr: np.ndarray             # (n_chr + 1, 2): ChrID.spos, segn
    patterns: list              # per pattern (weight, width, exam[weight])
    bclw: float
    bcup: float
    bcce: float
    blklen: int
    cfact: float = 0.75
    rbs_fact: float = f32(0.303 * 2)        # RbsFactSqr (src/blksrc.h:389)
    rbs_base: float = 3.0                   # RbsBase (:66)
    rln_fact: float = f32(0.00520 * 2)      # RlnFact (src/blksrc.h:390)
    max_mmc: int = 15                       # MaxMmc (:63)
    local: int = 0                          # algmode.lcl & 16
    max_out: int = 1                        # OutPrm.MaxOut
    # derived in __post_init__
    kk: int = field(init=False)
    rscrtab: list = field(init=False)
    seglen: list = field(init=False)

    def __post_init__(self):
        self.kk = self.nbitpat // 2 + 1
        weight = self.patterns[0][0]
        avr = float(self.avrscr) * weight / self.nshift                 # Randbs(avr, gdb = false)
        self.rbscoef = f32(self.rbs_fact * avr)
        self.rbscons = f32(self.rbs_base * avr)
        self.rlncoef = f32(self.rln_fact * avr * self.nbitpat)
        self.rscrtab = [int(self.rbscoef * math.sqrt(float(i + 1)) + self.rbscons) for i in range(128)]
        self.maxmmc = INT_MAX if (self.max_mmc == 0 or self.max_mmc > INT_MAX // weight or self.local) else weight * self.max_mmc // self.nshift
        self.ptpl = self.base() // self.avrscr
        self.ncand = self.max_out + 10                                  # NCAND2PHS (:30, 2220)
        self.app_c = float(self.nbitpat) ** self.cfact if self.kk > 1 else 1.0
        n = int(np.float32(1.2) * np.float32(2 * self.maxblk))          # Dhash(n, ud, hf = 1.2f): n = int(hf * n), in single precision
        self.hh_size = 31 if n < 31 else supprime(n)
        self.hh_step = 8                                                # SecondHS
        # setSegLen: a chromosome's blocks are blklen long but the last
        self.seglen = [0]
        for c in range(self.n_chr):
            ln = int(self.chr[c + 1][0]) - int(self.chr[c][0])
            while ln > self.blklen:
                self.seglen.append(self.blklen)
                ln -= self.blklen
            if ln > 0:
                self.seglen.append(ln)
        self.seglen += [0] * max(0, self.nseg + 1 - len(self.seglen))

    def base(self) -> int:
        return self.rscrtab[0]

    def randbs(self, mmc: int) -> int:
        if mmc < 128:
            return self.rscrtab[mmc]
        if self.rbscoef == 0:
            return int(self.rbscons)
        return int(self.rbscoef * math.sqrt(float(mmc + 1)) + self.rbscons)

    def lencor(self, ln: int) -> int:
        return int(self.rlncoef * math.sqrt(float(ln)))

    def chrblk(self, c: int) -> int:
        return int(self.chr[c][1])

    def find_chr_no(self, blk: int) -> int:
        lw = int(self.bclw + self.bcce * (blk - 1)) - 1
        up = int(self.bcup + self.bcce * (blk - 1)) + 1
        if lw < 0:
            lw = 0
        if up > self.n_chr:
            up = self.n_chr
        if self.chrblk(lw) > blk:
            lw = 0
        if self.chrblk(up) < blk:
            up = self.n_chr
        while up - lw > 1:
            md = (lw + up) // 2
            if self.chrblk(md) > blk:
                up = md
            elif self.chrblk(md + 1) > blk:
                return md
            else:
                lw = md
        return lw if self.chrblk(up) > blk else up


class Dhash:
    """Dhash<INT, int>(n, 0): open addressing, a slot whose value is 0 is EMPTY -- writing 0 into a live slot cuts every probe
    chain that ran over it, and the block search does exactly that to a block that fails to continue"""

    def __init__(self, size1: int, size2: int):
        self.size1, self.size2 = size1, size2
        self.clear()

    def clear(self):
        self.key = [0] * self.size1
        self.val = [0] * self.size1

    def map(self, key: int) -> int:
        v = key % self.size1
        u = self.size2 - key % self.size2
        v0 = v
        while self.val[v] != 0 and self.key[v] != key:
            v = (v + u) % self.size1
            if v == v0:
                raise OverflowError("Dhash full: the reference would grow it (never with lists no longer than MaxBlk)")
        if self.val[v] == 0:
            self.key[v] = key
        return v

    def incr(self, key: int) -> int:
        v = self.map(key)
        self.val[v] += 1
        return v


class PrQueue:
    """PrQueue<BlkScr>(data, Ncand, 0, maxi = false, rep = true): a min-heap by bscr; find looks at every entry"""

    def __init__(self, capacity: int):
        self.capacity, self.data = capacity, []

    @staticmethod
    def lt(a, b):
        return a[1] < b[1]

    def downheap(self, k: int, kmax: int = 0):
        d = self.data
        v = d[k]
        if kmax == 0:
            kmax = len(d)
        while k < kmax // 2:
            c = 2 * k + 1
            if c + 1 < kmax and self.lt(d[c + 1], d[c]):
                c += 1
            if not self.lt(d[c], v):
                break
            d[k] = d[c]
            k = c
        d[k] = v

    def upheap(self, k: int):
        d = self.data
        v = d[k]
        h = int((k - 1) / 2)                    # C's division: (0 - 1) / 2 = 0
        while k and self.lt(v, d[h]):
            d[k] = d[h]
            k = h
            h = int((h - 1) / 2)
        d[k] = v

    def find(self, key: int) -> int:
        for i, e in enumerate(self.data):
            if e[0] == key:
                return i
        return -1

    def put(self, x, p: int):
        if p < 0:
            if len(self.data) < self.capacity:
                self.data.append(x)
                self.upheap(len(self.data) - 1)
                return
            p = 0
        if self.lt(self.data[p], x):
            self.data[p] = x
            self.downheap(p)

    def hsort(self):
        d = self.data
        for k in range(len(d) - 1, 0, -1):
            d[0], d[k] = d[k], d[0]
            self.downheap(0, k)


def querywords(ix: Index, q, q_len: int, right: int, ss: int):
    """-> (wdscr, the posting lists that vote).  q: residue codes; a position outside the query reads as unusable"""
    def residue(i):
        if i < 0 or i >= q_len:
            return 255
        c = int(q[i])
        return int(ix.convtab[c]) if c < len(ix.convtab) else 255

    def spell(k):
        weight, _, exam = ix.patterns[k]
        w = 0
        for i in range(weight):
            c = residue(ss + exam[i])
            if c >= ix.nalpha:
                return w, i
            w = w * ix.nalpha + c
        return w, weight

    def posting(w):
        lp = int(ix.blkp[w])
        return [int(b) for b in ix.blkb[lp - 1:lp - 1 + int(ix.nblk[w])]]

    if ix.kk == 1:
        w, good = spell(0)
        if not ix.blkp[w]:
            return 0, []                        # "ubiquitous": asked before the word is known to be whole
        if good != ix.patterns[0][0]:
            return -1, []
        return int(ix.wscr[w]), [posting(w)]
    c = wdscr = 0
    lists = []
    for k in range(ix.kk):
        if ss >= right - ix.patterns[k][1]:
            break
        w, good = spell(k)
        if w >= ix.tabsize or ix.wscr[w] < 0 or good < ix.patterns[k][0] or not ix.blkp[w]:
            continue
        c += 1
        wdscr += int(ix.wscr[w])
        if k < ix.kk - 1:                       # (the last pattern scores but does not vote: next_mrglist's loop from 1)
            lists.append(posting(w))
    if not c:
        return -1, []
    return int(float(wdscr) / ix.app_c), lists


def merged(lists):
    """next_mrglist: ascending over the lists, a block of several once; a zero ends the list it stands in"""
    cut = []
    for l in lists:
        cut.append(l[:l.index(0)] if 0 in l else l)
    if len(cut) == 1:
        return cut[0]
    out, at = [], [0] * len(cut)
    while True:
        fronts = [l[a] for l, a in zip(cut, at) if a < len(l)]
        if not fronts:
            return out
        blk = min(fronts)
        out.append(blk)
        for i, l in enumerate(cut):
            if at[i] < len(l) and l[at[i]] == blk:
                at[i] += 1


def finds(ix: Index, q, left: int = 0, right: int = None):
    """-> dict(flags, nmmc, testword, sigm, heap = [(block, score)] in hsort order, cands = candidate sequences in the order
    finds fills sqs[1..] (-1 - c: a sequence seen before, whose slot keeps what it held), ret = what finds returns)"""
    q_len = len(q)
    if right is None:
        right = q_len
    nshift, width = ix.nshift, ix.patterns[0][1]
    if right - left - (nshift + width) < 1:
        return dict(flags=SHORT, nmmc=0, testword=[0, 0], sigm=0, heap=[], cands=[], ret=ERROR)
    # init2
    rscr = {}
    heap = PrQueue(ix.ncand)
    ts = right - (width + nshift) + 1
    ph = (ts - left) % nshift
    as_ = [[0] * nshift, [0] * nshift]
    for p in range(nshift):
        as_[0][p] = left + p
        as_[1][ph] = ts + p
        ph = (ph + 1) % nshift
    c = (right - left) // (2 * nshift) - 1
    rms = right - nshift * (c if c < ix.ptpl else ix.ptpl)
    testword = [0, 0]
    meet = False
    hh = Dhash(ix.hh_size, ix.hh_step)
    nmmc = 0
    while nmmc < ix.maxmmc and not meet:
        for d in range(2):
            e = 1 - d
            for s in range(nshift):
                ms = min(as_[e][s], rms)
                cscr = p = qq = 0
                hh.clear()
                while True:                     # continuous hits
                    ss = as_[d][s]
                    as_[d][s] += -nshift if d else nshift
                    if d ^ (ss >= ms):          # has scanned
                        meet = True
                        break
                    wdscr, lists = querywords(ix, q, q_len, right, ss)
                    if wdscr < 0:
                        break
                    testword[d] += 1
                    if wdscr == 0:
                        qq = 1                  # ubiquitous
                    else:
                        p += 1
                        qq = 0
                        cscr += wdscr
                        for blk in merged(lists):
                            lenadjst = ix.lencor(ix.seglen[blk])
                            h = hh.incr(blk)
                            if p == hh.val[h]:  # let's continue
                                qq += 1
                                rscr[blk] = rscr.get(blk, 0) + wdscr
                                if rscr[blk] >= ix.randbs(nmmc) + lenadjst:
                                    x = (blk, rscr[blk])        # Bhit2::update
                                    heap.put(x, heap.find(blk))
                            else:
                                hh.val[h] = 0   # fail to continue
                    if not (qq and cscr < ix.base()):
                        break
        nmmc += 1
    sigm = len(heap.data)
    cands = []
    if sigm:
        heap.hsort()
        seen = set()
        for i in range(min(ix.max_out, sigm)):
            ch = ix.find_chr_no(heap.data[i][0])
            cands.append(-1 - ch if ch in seen else ch)
            seen.add(ch)
    return dict(flags=REACHED, nmmc=nmmc, testword=testword, sigm=sigm, heap=list(heap.data), cands=cands,
                ret=len(cands) if sigm else ERROR)


def record(r: dict) -> list:
    """the result as spdp_blk_finds lays it out (include/spdp.h)"""
    if r["flags"] & SHORT:
        return [3, 0, SHORT]
    out = [0, r["nmmc"], r["flags"], r["testword"][0], r["testword"][1], r["sigm"]]
    for b, s in r["heap"]:
        out += [b, s]
    out.append(len(r["cands"]))
    out += r["cands"]
    out[0] = len(out)
    return out


# ---- an index from the arrays the library's reader (or a reference-side dump) gives -------------------------------------------------
def index_from_arrays(fx: dict, avrscr: int, **opts) -> Index:
    bp = np.asarray(fx["blk_bitpat"], dtype=np.int64)
    pats, at = [], 0
    kk = int(fx["kk"])
    for _ in range(kk):
        weight, width = int(bp[at]), int(bp[at + 1])
        pats.append((weight, width, [int(x) for x in bp[at + 3:at + 3 + weight]]))
        at += 3 + 2 * weight
    return Index(nalpha=int(fx["nalpha"]), tabsize=int(fx["tabsize"]), nshift=int(fx["nshift"]), nbitpat=int(fx["nbitpat"]),
                 n_chr=int(fx["n_chr"]), maxblk=int(fx["maxblk"]), nseg=int(fx["nseg"]), avrscr=int(avrscr),
                 convtab=np.asarray(fx["blk_convtab"]), nblk=np.asarray(fx["blk_nblk"]), wscr=np.asarray(fx["blk_wscr"]).astype(np.int16),
                 blkp=np.asarray(fx["blk_blkp"]), blkb=np.asarray(fx["blk_blkb"]),
                 chr=np.asarray(fx["blk_chr"], dtype=np.int64).reshape(-1, 2), patterns=pats,
                 bclw=float(fx["bclw"]), bcup=float(fx["bcup"]), bcce=float(fx["bcce"]), blklen=int(fx["blklen"]),
                 cfact=float(fx.get("cfact", 0.75)), **opts)
