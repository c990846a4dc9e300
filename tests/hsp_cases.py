"""Tasks for the HSP search of a candidate region (spdp_hsp_search: spdp_hsp_tasks on the device, spdp_hsp_tasks_host in the host
form), built by named recipe; shared by tests/test_hsp_cases.py (the generator held to its effects, CPU) and
tests/test_gpu_hsp_cases.py (device against host form, record by record).

A case is one task: a query with its range, a region, a strand, and a planted diagonal -- the region holds, at nucleotide g0 of
the orientation the search reads, a copy of the query from the range's first residue on, every residue of the copy either the
query's or one of another class that scores badly (`match`).  Whatever else the region holds is noise, so a word read one off
or a walk one too far changes the result.  Regions lie one behind the other in the chromosomes of a request's genome with noise
between them; a task on the other strand has the reverse complement of what the search reads stored there.

requests() -> the calls: every case of one (model, a_exgl, a_exgr, plan) goes into the same call.  Everything is a function of
the recipe's name.  restate(request, task) is a plain restatement of the search on that task (words, segments, records, and the
branches each step took): the census of tests/test_hsp_cases.py counts classes by those branches.

Models (MODELS): the level-0 parameters of the blk_k1 (nucleotide) and blk_p1 (protein) fixtures, which are spaced patterns
(110010110111 and 11011); one copy of each with the contiguous word of the same weight; the protein model with crs = 0; the
nucleotide model with half the words at or above `mask`."""
import functools
import zlib

import numpy as np

from spaln_amd import abi
from tests import spdg
from tests.conftest import golden_files

A, C_, G, T, N = 2, 3, 5, 9, 16
NUC = np.array([A, C_, G, T], dtype=np.uint8)
COMPLEMENT = np.array([0, 1, 9, 5, 13, 3, 11, 7, 15, 2, 10, 6, 14, 4, 12, 8, 16], dtype=np.uint8)
AA = np.arange(3, 23, dtype=np.uint8)
X_AA, SER, SER2, LYS = 2, 18, 23, 14
TOO_LONG, TOO_MANY = 1, 2
MODELS = ("nt", "nt_contig", "nt_mask", "aa", "aa_contig", "aa_crs0")


# ---- the genetic code in the tron alphabet (A = 3 .. V = 22, AGY serines 23, TGA 24, TAA / TAG 25), bases in A C G T order ---------
def _code_tables():
    aas, order, acgt = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "ARNDCQEGHILKMFPSTWYV", (3, 1, 0, 2)
    tron_of = np.zeros(64, dtype=np.uint8)
    for c in range(64):
        b1, b2, b3 = acgt[c >> 4], acgt[(c >> 2) & 3], acgt[c & 3]
        aa = aas[c]
        code = (24 if (b1, b2, b3) == (3, 2, 0) else 25) if aa == "*" else 23 if aa == "S" and b1 == 0 else 3 + order.index(aa)
        tron_of[16 * b1 + 4 * b2 + b3] = code
    codon = {}
    for i in range(64):
        codon.setdefault(int(tron_of[i]), NUC[[i >> 4, (i >> 2) & 3, i & 3]])
    return tron_of, codon


TRON_OF, CODON = _code_tables()
_PLAIN = np.array([15, 15, 0, 1, 4, 2, 5, 6, 10, 3, 7, 8, 10, 9, 12, 13, 14])          # A C G T -> 0 .. 3, the rest >= 4
_FIRST_OF = np.array([0, 0, 0, 1, 2, 2, 0, 2, 0, 3, 3, 3, 1, 1, 2, 3, 0])
_LIKELY = np.array([14, 3, 10, 13])


def to_tron(nuc):
    """position p of a nucleotide sequence as the codon (p - 1, p, p + 1); the sequence's pads (0) stand before and behind it"""
    c1 = np.minimum(np.asarray(nuc, dtype=np.int64), 16)
    c0, c2 = np.concatenate([[0], c1[:-1]]), np.concatenate([c1[1:], [0]])
    r0, r1 = _PLAIN[c0], _PLAIN[c1]
    full = TRON_OF[np.minimum(16 * np.minimum(r0, 3) + 4 * np.minimum(r1, 3) + _FIRST_OF[c2], 63)]
    return np.where(c1 <= 1, 1, np.where(r1 >= 4, 2, np.where(r0 >= 4, _LIKELY[np.minimum(r1, 3)], full))).astype(np.uint8)


def other_strand(nuc):
    return COMPLEMENT[np.minimum(np.asarray(nuc, dtype=np.uint8), 16)][::-1].copy()


# ---- models ------------------------------------------------------------------------------------------------------------------------
def _fixture(name):
    return spdg.load([f for f in golden_files("blk_") if f.endswith(name + ".spdg")][0])


@functools.lru_cache(maxsize=None)
def model(key):
    m = abi.wilip_model_from_fixture(_fixture("blk_k1" if key.startswith("nt") else "blk_p1"))
    L = m.level[0]
    if key.endswith("_contig"):
        L.width = int(sum(L.bitpat[:L.bitpat_len]))
        L.bitpat_len = 0
    if key == "nt_mask":
        L.mask //= 2
    if key == "aa_crs0":
        m.crs = 0
    return m


def shape(m):
    """what the restatement and the recipes read of a model's level 0"""
    L = m.level[0]
    exam = [w for w in range(L.bitpat_len) if L.bitpat[w]] if L.bitpat_len else list(range(L.width))
    mtx = np.array(m.mtx[:m.mtx_rows * m.mtx_cols], dtype=np.int64).reshape(m.mtx_rows, m.mtx_cols)
    return dict(elem=L.elem, tpl=L.tpl, mask=L.mask, width=L.width, gain=L.gain, gain1=L.gain1, cutoff=L.cutoff, vthr=L.vthr, exam=exam,
                conv=np.array(L.convtab, dtype=np.int64), mtx=mtx, bbt=3 if m.dvsp == 1 else 1, short=m.shortquery, end_bonus=m.end_bonus,
                crs=m.crs, ser=m.ser, ser2=m.ser2)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def word_ids(S, cls, first, step, count):
    """the word whose first residue is cls[first + p], p = 0 .. count - 1, residues `step` apart; -1: none"""
    if count <= 0:
        return np.zeros(0, dtype=np.int64)
    idx = first + np.arange(count)[:, None] + step * np.array(S["exam"])[None, :]
    c = cls[idx]
    w = (c * (S["elem"] ** np.arange(len(S["exam"]) - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)
    return np.where((c < S["elem"]).all(axis=1) & (w < S["mask"]), w, -1)


def region_as_read(rq, t):
    """the task's region as the search reads it: strand, then tron codes for a protein query"""
    q, ch, base, ln, rvs = t
    g = rq["genome"][int(rq["chr_off"][ch]) + base:int(rq["chr_off"][ch]) + base + ln]
    g = np.minimum(g, 16)
    if rvs:
        g = other_strand(g)
    return to_tron(g) if rq["bbt"] == 3 and ln else g


def shared_words(rq, t):
    """(query position, region position) of every word both sides share: the word stage alone"""
    S = rq["shape"]
    q = t[0]
    a, (left, right) = rq["queries"][q], rq["ranges"][q]
    b = region_as_read(rq, t)
    bbt, w = S["bbt"], S["width"]
    nk, nn = right - left - (w - 1), len(b) - (3 * w - 1 if bbt == 3 else w - 1)
    if nk <= 0 or nn <= 0:
        return nk, nn, np.zeros((0, 2), dtype=np.int64)
    qa = word_ids(S, S["conv"][a.astype(np.int64) & 31], left, 1, nk)
    rb = word_ids(S, S["conv"][b.astype(np.int64) & 31], 1 if bbt == 3 else 0, bbt, nn)
    # every (query word, region word) pair of equal words: a sorted join (no query x region table: one case has a region of 2^20)
    order = np.argsort(qa, kind="stable")
    qs = qa[order]
    n_at = np.nonzero(rb >= 0)[0]
    lo, hi = np.searchsorted(qs, rb[n_at], "left"), np.searchsorted(qs, rb[n_at], "right")
    n = np.repeat(n_at, hi - lo)
    within = np.arange(len(n)) - np.repeat(np.cumsum(hi - lo) - (hi - lo), hi - lo)
    m = order[np.repeat(lo, hi - lo) + within]
    return nk, nn, np.stack([m, n], axis=1)


def restate(rq, t):
    """the search on one task: dict(nk, nn, words, segments, records (k, 7) in scan order, branches)"""
    S = rq["shape"]
    q = t[0]
    a, (left, right) = rq["queries"][q].astype(np.int64), rq["ranges"][q]
    a_len, tlen = len(a), (len(a) if rq["tlen"] is None else int(rq["tlen"][q]))
    exgl, exgr = rq["exg"]
    b = region_as_read(rq, t).astype(np.int64)
    b_len, bbt, w, gain, tpl = len(b), S["bbt"], S["width"], S["gain"], S["tpl"]
    conv, mtx = S["conv"], S["mtx"]
    nk, nn, pairs = shared_words(rq, t)
    br = set()
    if nk > 0 and (word_ids(dict(S, mask=1 << 62), conv[a & 31], left, 1, nk) >= S["mask"]).any():
        br.add("query_word_at_or_above_mask")
    cutoff, vthr, precutoff = S["cutoff"], S["vthr"], S["cutoff"] - gain * tpl
    if a_len < S["short"]:
        cutoff, vthr, precutoff = cutoff * a_len // S["short"], vthr * a_len // S["short"], precutoff * a_len // S["short"]
        br.add("short_query")
    mm = right - left
    out = dict(nk=nk, nn=nn, words=len(pairs), segments=[], records=np.zeros((0, 7), dtype=np.int32), branches=br)
    if nk <= 0 or nn <= 0:
        br.add("empty")
        return out
    segs, tplwt = [], tpl * gain
    by_diag = {}
    for m, n in pairs.tolist():
        by_diag.setdefault(n - bbt * m, []).append(m)
    out["per_diagonal"] = {r: len(v) for r, v in by_diag.items()}
    for r in sorted(by_diag):
        score = best = first = best_at = 0
        prev = -(w + 1)
        for m in sorted(by_diag[r]):
            gap = m - prev - w
            if gap > 0:
                floor_ = best - cutoff
                score -= gain * gap
                if prev >= 0:
                    br.add("gap_1" if gap == 1 else "gap_more")
                if floor_ > score or score < 0:
                    if floor_ > 0:
                        segs.append((first, r, best_at, best))
                        br.add("segment_closed_by_a_gap")
                    elif prev >= 0:
                        br.add("run_dropped_at_a_gap_best_%s_cutoff" % ("eq" if floor_ == 0 else "below"))
                    score = tplwt + (gain * (w - m) if m < w else 0)
                    if m < w:
                        br.add("first_word_bonus")
                    best, best_at, first = score, m, m
                else:
                    score += tplwt
                    br.add("segment_goes_on_over_a_gap")
            else:
                if gap == 0:
                    br.add("gap_0")
                score += S["gain1"] if m - first == 1 else gain
                if m - first == 1:
                    br.add("gain1")
            if score > best:
                best, best_at = score, m
            prev = m
        if best > precutoff:
            over = best_at + 2 * w - mm
            if over > 0:
                br.add("over" if best <= cutoff < best + gain * over else "over_idle")
                best += gain * over
            if best > cutoff:
                segs.append((first, r, best_at, best))
                if best == cutoff + 1:
                    br.add("segment_at_cutoff_plus_1")
            elif best == cutoff:
                br.add("diagonal_at_cutoff")
        elif best == precutoff:
            br.add("diagonal_at_precutoff")
    out["segments"] = segs
    recs = []
    for first, r, last, _best in segs:
        jx, jy, jlen = left + first, bbt * first + r, last - first + w
        as_, bs, scr = jx, jy + (1 if bbt == 3 else 0), 0
        if exgl and tpl - jx > 0:
            scr += S["end_bonus"] * min(tpl - jx, tpl)
            br.add("exgl_bonus")
        while True:
            as_ -= 1
            if as_ < 0:
                br.add("backward_to_query_0")
                break
            bs -= bbt
            if bs < 0:
                br.add("backward_to_region_0")
                break
            if conv[a[as_] & 31] != conv[b[bs] & 31]:
                break
            jx, jy, jlen = jx - 1, jy - bbt, jlen + 1
        if as_ < 0:
            bs -= bbt
        a_end, b_end = min(jx + jlen, right), min(jy + bbt * jlen, b_len)
        b_stop, from_ = (b_len - 1 if bbt == 3 else b_len), as_
        ln = nid = w_from = w_len = w_nid = restart = 0
        best = scr
        while True:
            as_ += 1
            if as_ >= tlen:
                br.add("forward_to_tlen_below_a_len" if tlen < a_len else "forward_to_query_end")
                break
            bs += bbt
            if bs >= b_stop:
                br.add("forward_to_region_end")
                break
            ca, cb = a[as_], b[bs]
            if (as_ >= a_end or bs >= b_end) and conv[ca & 31] != conv[cb & 31]:
                break
            ln += 1
            scr += mtx[ca, cb]
            if ca == cb or (ca == S["ser"] and cb == S["ser2"]):
                nid += 1
                if ca != cb:
                    br.add("ser_ser2")
            if scr < 0:
                scr, restart, ln, nid = 0, as_ - from_, 0, 0
                if as_ < a_end:
                    br.add("restart_inside_the_seed")
            if scr > best:
                best, w_from, w_len, w_nid = scr, restart, ln, nid
        jx, jy = jx + w_from, jy + bbt * w_from
        if S["crs"] == 0 and bbt == 3:
            scr -= min(w_len - w_nid, 3) * vthr
            br.add("crs0_mismatches_%d" % min(w_len - w_nid, 4))
        rend = tpl - right + jx + w_len
        if exgr and rend > 0:
            scr += S["end_bonus"] * min(rend, tpl)
            br.add("exgr_bonus")
        elif w_nid == w_len:
            scr += S["end_bonus"] * 4
            br.add("identical_bonus")
        elif w_len - w_nid == 1:
            br.add("one_mismatch_short_of_identical")
        if scr > vthr:
            recs.append((jx, jy, w_len, w_nid, scr, r, first))
            if w_from > 0:
                br.add("window_starts_after_a_restart")
        elif scr == vthr:
            br.add("record_at_vthr")
    if recs:
        out["records"] = np.array(recs, dtype=np.int32)
    return out


def flags_of(rq, t, words, segments, records, plan):
    """the flags the device form gives the task under a plan, from the three counts: arithmetic (include/spdp.h)"""
    S = rq["shape"]
    q = t[0]
    left, right = rq["ranges"][q]
    w, bbt = S["width"], S["bbt"]
    nk, nn = right - left - (w - 1), t[3] - (3 * w - 1 if bbt == 3 else w - 1)
    if nk <= 0 or nn <= 0:
        return 0
    mbits = 1
    while (1 << mbits) < nk:
        mbits += 1
    if nk > plan["hash_slots"] // 2 or nk >= 65535 or (nn + bbt * (nk - 1)) << mbits > 0xfffffff0:
        return TOO_LONG
    return TOO_MANY if words > plan["hit_cap"] or segments > plan["seg_cap"] or records > plan["out_cap"] else 0


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _letters(S):
    return NUC if S["bbt"] == 1 else AA


def _unlike(S, c):
    """a residue of another class that scores badly against query residue c (for a protein query: an amino acid)"""
    if S["bbt"] == 1:
        return {A: C_, C_: A, G: T, T: G}.get(int(c), A)
    row = S["mtx"][int(c), 3:23].copy()
    row[S["conv"][3:23] == S["conv"][int(c)]] = 10 ** 6
    return 3 + int(np.argmin(row))


class Case:
    """one task.  match: per query position True (the region holds the query's residue on the planted diagonal), False (a residue
    of another class) or an explicit residue (nucleotide code, or for a protein query a tron code that has a codon)"""

    def __init__(self, key, recipe, effect, q, left, right, g0, b_len, match, rvs, tlen=None, exg=(0, 0), plan=None, region=None):
        self.key, self.recipe, self.effect, self.q, self.left, self.right = key, recipe, effect, np.asarray(q, dtype=np.uint8), left, right
        self.g0, self.b_len, self.match, self.rvs, self.tlen, self.exg, self.plan = g0, b_len, match, rvs, tlen, exg, plan
        self.region = region

    def region_as_planted(self, rng):
        """the region's nucleotides in the orientation of the search"""
        if self.region is not None:
            return np.asarray(self.region, dtype=np.uint8)
        S = shape(model(self.key))
        bbt = S["bbt"]
        b = NUC[rng.integers(0, 4, size=self.b_len)]
        for i in range(len(self.q)):
            g = self.g0 + bbt * (i - self.left)
            mt = self.match[i] if i < len(self.match) else None
            if mt is None:
                continue
            c = int(self.q[i]) if mt is True else _unlike(S, self.q[i]) if mt is False else int(mt)
            res = np.array([c], dtype=np.uint8) if bbt == 1 else CODON[c if c in CODON else 3]
            for k in range(bbt):
                if 0 <= g + k < self.b_len:
                    b[g + k] = res[k]
        return b


def _query(S, rng, n, rich=False):
    """random residues of the alphabet; rich: for a protein query only those that score 52 or more against themselves, so that a
    dozen of them make a record"""
    letters = _letters(S)
    if rich and S["bbt"] == 3:
        letters = np.array([c for c in AA if S["mtx"][c, c] >= 52], dtype=np.uint8)
    return letters[rng.integers(0, len(letters), size=n)]


def _mild(S, c):
    """a residue that is not the query's but costs little: an ambiguity code that holds the base, the most similar amino acid"""
    if S["bbt"] == 1:
        return {A: 4, C_: 4, G: 6, T: 10}[int(c)]
    row = S["mtx"][int(c), 3:23].copy()
    row[S["conv"][3:23] == S["conv"][int(c)]] = -10 ** 6
    return 3 + int(np.argmax(row))


FLANK = 12


def _runs(a_len, *runs):
    """match list: None outside every run's surroundings, True inside a run, False on the FLANK residues before and behind a run
    (no word of noise then reaches into a run through the pattern's don't-care positions) and on every residue between two runs"""
    m = [None] * a_len
    lo, hi = min(r[0] for r in runs), max(r[0] + r[1] for r in runs)
    for i in range(max(lo - FLANK, 0), min(hi + FLANK, a_len)):
        m[i] = False
    for s, n in runs:
        for i in range(s, s + n):
            m[i] = True
    return m


def words_to_residues(S, n_words):
    return n_words + S["width"] - 1


def min_words(S, a_len=10 ** 6, start_bonus=0, gain1=True):
    """the fewest adjacent words that make a segment by themselves, far from the range's end"""
    cutoff = S["cutoff"] * a_len // S["short"] if a_len < S["short"] else S["cutoff"]
    n, score = 1, S["tpl"] * S["gain"] + start_bonus
    while score <= cutoff:
        n += 1
        score += S["gain1"] if n == 2 and gain1 else S["gain"]
    return n


def min_record_residues(S):
    """the shortest all-identical window of _query(rich=True) residues that makes a record whatever they are, no end bonus of exg"""
    self_score = 20 if S["bbt"] == 1 else 52
    n = 1
    while n * self_score + 4 * S["end_bonus"] <= S["vthr"]:
        n += 1
    return n


# ---- recipes --------------------------------------------------------------------------------------------------------------------
def _words_recipes():
    out = []
    for k in range(24):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("copy%d" % k)
        a_len = int(rng.integers(60, 601))
        left = int(rng.integers(0, 20)) if k % 3 else 0
        right = a_len - (int(rng.integers(0, 20)) if k % 3 == 1 else 0)
        b_len = min(4000, S["bbt"] * (right - left) + int(rng.integers(60, 1500)))
        g0 = int(rng.integers(1, b_len - S["bbt"] * (right - left)))
        out.append(Case(key, "words/copy", "the range's copy in noise: one long diagonal across the lanes' slices", _query(S, rng, a_len), left, right, g0, b_len,
                        _runs(a_len, (left, right - left)), (k // 6) % 2))
    # runs of adjacent words at the least number that makes a segment and one fewer, in the middle of the range; the number that is
    # enough only at the range's first word, or only at its end, there and in the middle
    for k in range(144):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("runs%d" % k)
        w, kind, fewer = S["width"], ("gain1", "first_word", "over")[(k // 6) % 3], (k // 18) % 2
        a_len, left = int(rng.integers(160, 400)), int(rng.integers(0, 9))
        right = a_len - int(rng.integers(0, 9))
        if kind != "gain1" and key == "nt_contig":                   # (the whole end bonus: this model's run makes no record with less)
            left, right = 0, a_len
        mm = right - left
        if kind == "gain1":                                          # (long enough for a record, too short for a segment were gain1 read as gain)
            n = max(min_words(S), min_record_residues(S) - w + 1) if not fewer else min_words(S) - 1
            assert n < min_words(S, gain1=False)
            start = left + int(rng.integers(2 * w, mm - words_to_residues(S, n) - 3 * w))
        elif kind == "first_word":                                   # (one word fewer than makes a segment elsewhere)
            n = min_words(S) - 1
            start = left + (2 * w + 5 if fewer else 0)
        else:
            n = min_words(S) - 1
            start = right - words_to_residues(S, n) - (3 * w if fewer else 0)
        out.append(Case(key, "words/%s%s" % (kind, "_not" if fewer else ""), "%d adjacent words %s" % (n, "where the recipe's term does not reach" if fewer else "where it does"),
                        _query(S, rng, a_len, rich=True), left, right, 7 + int(rng.integers(0, 50)), S["bbt"] * a_len + 200,
                        _runs(a_len, (start, words_to_residues(S, n))), (k // 36) % 2 if k < 72 else (k // 3) % 2,
                        exg={"gain1": (0, 0), "first_word": (1, 0), "over": (0, 1)}[kind]))   # (the end's bonus: the contiguous model's run is too short for a record without)
    # two runs on one diagonal: a gap the segment goes on over, a gap that closes it, a first run whose best is exactly the cutoff,
    # a single residue of another class
    for k in range(96):
        kind = ("goes_on", "closed", "at_cutoff", "one_residue")[(k // 6) % 4]
        key = MODELS[k % len(MODELS)] if kind != "at_cutoff" else ("nt", "nt_contig")[k % 2]     # (the protein fixture's gains never sum to its cutoff)
        S, rng = shape(model(key)), _rng("gaps%d" % k)
        w = S["width"]
        a_len = 600
        n1 = min_words(S) + (int(rng.integers(2, 9)) if kind != "at_cutoff" else -1)
        r1 = words_to_residues(S, n1)
        between = {"goes_on": int(rng.integers(4, 7)), "closed": S["cutoff"] + 40, "at_cutoff": S["cutoff"] + 40, "one_residue": 1}[kind]
        r2 = words_to_residues(S, min_words(S) + int(rng.integers(6, 30)))
        s1 = int(rng.integers(w + 2, a_len - r1 - between - r2 - 3 * w))
        out.append(Case(key, "words/two_runs_" + kind, "two runs of one diagonal, %d residues of another class between them" % between,
                        _query(S, rng, a_len), 0, a_len, 11 + int(rng.integers(0, 50)), S["bbt"] * a_len + 300,
                        _runs(a_len, (s1, r1), (s1 + r1 + between, r2)), (k // 24) % 2))
    # words exactly `step` apart on the diagonal: every residue no word at a multiple of `step` cares for is another one, a mild one
    # (step = width: gap 0, which only a spaced pattern can have; width + 1: gap 1; width + 3)
    for k in range(108):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("lattice%d" % k)
        w = S["width"]
        step = w + (0, 1, 3)[(k // 6) % 3]
        a_len = 600 if S["bbt"] == 1 else 300
        q = _query(S, rng, a_len)
        s, n = 20, a_len - 40 - (a_len - 40) % step
        m = _runs(a_len, (s, n))
        for i in range(n):
            if i % step not in S["exam"]:
                m[s + i] = _mild(S, q[s + i])
        out.append(Case(key, "words/lattice_%s" % ("width", "width_plus_1", "width_plus_3")[(k // 6) % 3], "words %d apart on the diagonal" % step, q, 0, a_len, 33,
                        S["bbt"] * a_len + 150, m, (k // 18) % 2))
    # residues outside the reduced alphabet inside a copy: N runs and IUPAC codes in the region, X in a protein query, stop codons
    for k in range(24):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("outside%d" % k)
        a_len = int(rng.integers(150, 400))
        q = _query(S, rng, a_len)
        m = _runs(a_len, (0, a_len))
        for _ in range(4):
            at, n = int(rng.integers(10, a_len - 10)), int(rng.integers(1, 5))
            for i in range(at, at + n):
                if S["bbt"] == 1:
                    m[i] = int(rng.choice([N, N, 4, 6, 7, 8, 10, 15]))
                elif (k // 6) % 2:
                    m[i] = int(rng.choice([24, 25]))
                else:
                    q[i] = X_AA
        out.append(Case(key, "words/outside_alphabet", "residues that belong to no class inside a copy", q, 0, a_len, 20, S["bbt"] * a_len + 100, m, (k // 12) % 2))
    # one word alone, a residue of another class on each position of the pattern in turn: a cared-for position loses the word
    for k in range(24):
        key = ("nt", "aa")[k % 2]
        S, rng = shape(model(key)), _rng("pattern%d" % k)
        w, a_len = S["width"], 80
        m = _runs(a_len, (30, w))
        off = (k // 2) % w
        m[30 + off] = False
        out.append(Case(key, "words/pattern_position", "a single word, position %d of the pattern unlike (%s)" % (off, "cared for" if off in S["exam"] else "don't care"),
                        _query(S, rng, a_len), 0, a_len, 9, S["bbt"] * a_len + 60, m, (k // 12) % 2))
    return out


def _stretch_recipes():
    out = []
    for k in range(144):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("stretch%d" % k)
        bbt, w = S["bbt"], S["width"]
        kind = ("query_0", "region_0", "tlen", "region_end", "restart", "one_mismatch")[(k // 6) % 6]
        a_len = int(rng.integers(250, 500))
        q = _query(S, rng, a_len)
        left, right, tlen, g0, b_len = 0, a_len, None, 15, bbt * a_len + 200
        n = words_to_residues(S, min_words(S) + 10) + int(rng.integers(0, 20))
        if kind == "query_0":
            left, g0 = int(rng.integers(3, 12)), 45
            m = _runs(a_len, (0, left + n))
        elif kind == "region_0":
            left, d = 40, int(rng.integers(5, 30))
            pad_codon = bbt == 3 and (k // 72) % 2 == 1             # the region begins inside a codon: its first base is the sequence's pad
            g0 = -(bbt * d + 1) if pad_codon else -bbt * d
            if pad_codon:
                q[left + d] = LYS                                   # (read by its middle base: A, the commonest such residue is K)
            m = _runs(a_len, (left + d, n))
        elif kind == "tlen":
            right = tlen = a_len - int(rng.integers(5, 40))
            m = _runs(a_len, (right - n, n + (a_len - right)))
        elif kind == "region_end":
            s = int(rng.integers(20, 60))
            b_len = g0 + bbt * (s + n) + (k // 72) % 2 + (k // 36) % 2
            m = _runs(a_len, (s, n + 12))
        elif kind == "restart":
            # (the residues between the runs cost more than the first run gains, and the segment still goes on over them)
            n1 = words_to_residues(S, min_words(S) + (2 if bbt == 1 else 0))
            s = int(rng.integers(20, 40))
            m = _runs(a_len, (s, n1), (s + n1 + (10 if bbt == 1 else 12), n + 30))
            if bbt == 3:
                q[s:s + n1 + 12] = np.where(rng.random(n1 + 12) < .5, 3, 19)
        else:
            s = int(rng.integers(20, 60))
            m = _runs(a_len, (s, n + 40))
            m[s + 20 + w] = False
        out.append(Case(key, "stretch/" + kind, "the walk's stop or the window's start named by the recipe", q, left, right, g0, b_len, m, (k // 36) % 2, tlen=tlen))
    # every combination of a_exgl / a_exgr, a run inside tpl of each end and one in the middle
    for k in range(144):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("exg%d" % k)
        exg = ((k // 6) & 1, (k // 12) & 1)
        a_len = int(rng.integers(200, 400))
        n = words_to_residues(S, min_words(S) + 8)
        at = (int(rng.integers(0, S["tpl"])), a_len - n - int(rng.integers(0, S["tpl"])), a_len // 2)[(k // 24) % 3 if k < 72 else (k // 24) % 2]
        out.append(Case(key, "stretch/exg", "a run %d residues from the query's start, a_exgl / a_exgr = %d / %d" % (at, exg[0], exg[1]), _query(S, rng, a_len), 0, a_len, 30,
                        S["bbt"] * a_len + 100, _runs(a_len, (at, n)), (k // 3) % 2, exg=exg))
    # protein: 0, 1, 3, 4 residues unlike the query inside a window, under crs = 0 (the term caps at 3) and crs = 1; SER against SER2;
    # the region's last codon
    for k in range(192):
        key = ("aa_crs0", "aa")[k % 2]
        S, rng = shape(model(key)), _rng("prot%d" % k)
        mis = (0, 1, 3, 4)[(k // 2) % 4]
        a_len = int(rng.integers(200, 400))
        q = _query(S, rng, a_len)
        s, n = 30, 110
        q[s + 3:s + n:9] = SER
        m = _runs(a_len, (s, n))
        for j in range(mis):
            m[s + 20 + 17 * j] = False
        if (k // 8) % 2:
            for i in range(s, s + n):
                if q[i] == SER and m[i] is True:
                    m[i] = SER2
        b_len = 3 * a_len + 100
        if (k // 16) % 3 == 2:
            b_len = 12 + 3 * (s + n) + k % 3
        out.append(Case(key, "stretch/protein_mismatches", "%d residues unlike the query inside the window" % mis, q, 0, a_len, 12, b_len, m, (k // 4) % 2))
    return out


def _range_recipes():
    out = []
    for k in range(72):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("short%d" % k)
        at_end = (k // 18) % 2
        # (the protein fixture's gains are multiples of 4 and its cutoff 51: at 49 residues no sum lies between 49 and 51; at 47 one does)
        a_len = S["short"] + (-1 if S["bbt"] == 1 else -3, 0, 1)[(k // 6) % 3] - (10 if at_end else 0)
        # in the middle: a run whose best is the unscaled cutoff exactly, a segment only under the scaled one.  At the range's end
        # (a_exgr on): a run whose best lies above the scaled precutoff only, a segment by the end's term
        n = min_words(S) - 1
        if at_end:                                                   # (the most words whose sum stays at or below the unscaled precutoff)
            n = 2 + (S["cutoff"] - 2 * S["tpl"] * S["gain"] - S["gain1"]) // S["gain"]
        r = words_to_residues(S, n)
        out.append(Case(key, "ranges/short_query", "a_len %d around shortquery %d, a run between the scaled and the unscaled cut-off" % (a_len, S["short"]), _query(S, rng, a_len), 0, a_len, 25,
                        S["bbt"] * a_len + 120, _runs(a_len, (a_len - r, r) if at_end else (S["width"], r)), (k // 36) % 2, exg=(0, at_end)))
    for k in range(48):
        key = MODELS[k % len(MODELS)]
        S, rng = shape(model(key)), _rng("tiny%d" % k)
        w, bbt = S["width"], S["bbt"]
        kind = (k // 6) % 4
        mm = (w - 1, w, 30, 30)[kind]
        b_len = (200, 200, bbt * w - 1, bbt * w)[kind]
        out.append(Case(key, "ranges/tiny", "range of %d residues, region of %d: width %d" % (mm, b_len, w), _query(S, rng, 60), 10, 10 + mm, 0, b_len,
                        _runs(60, (10, mm)), (k // 24) % 2))
    return out


def _copies(key, name, n_copies, mm, run_words, rvs, recipe, effect, plan, tlen=None, one_more_word=0):
    """a region of N with n_copies copies of one run of the query's range, each on a diagonal of its own (one_more_word: and a copy
    of the run's first word)"""
    S, rng = shape(model(key)), _rng(name)
    bbt = S["bbt"]
    a_len = mm + 12
    q = _query(S, rng, a_len)
    r = words_to_residues(S, run_words)
    at = 6 + (mm - r) // 2
    piece = q[at:at + r] if bbt == 1 else np.concatenate([CODON[int(c)] for c in q[at:at + r]])
    gap = 9 if n_copies < 100 else bbt
    b = np.full(40 + (n_copies + one_more_word) * (len(piece) + gap), N, dtype=np.uint8)
    for i in range(n_copies + one_more_word):
        part = piece if i < n_copies else piece[:bbt * S["width"]]
        b[20 + i * (len(piece) + gap):20 + i * (len(piece) + gap) + len(part)] = part
    return Case(key, recipe, effect, q, 6, 6 + mm, None, len(b), None, rvs, plan=plan, region=b, tlen=tlen)


def _cap_recipes():
    """under the small plans: shared words, segments, records and nk at the cap and one beyond -- the counts are arithmetic on regions
    that hold nothing but N and what the recipe plants"""
    out = []
    for i, key in enumerate(("nt", "aa", "nt_contig", "aa_contig", "aa_crs0")):       # (nt_mask drops words of its own: the counts would not be the recipe's)
        S = shape(model(key))
        w, bbt = S["width"], S["bbt"]
        run = min_words(S) + 2
        for beyond in (0, 1):
            rvs = (i + beyond) % 2
            tag = "%s%d" % (key, beyond)
            out.append(_copies(key, "seg" + tag, CAP_PLANS["segments"]["seg_cap"] + beyond, 100, run, rvs, "caps/segments",
                               "seed segments at seg_cap%s" % (" + 1" if beyond else ""), "segments"))
            out.append(_copies(key, "rec" + tag, CAP_PLANS["records"]["out_cap"] + beyond, 100, run, rvs, "caps/records",
                               "records at out_cap%s" % (" + 1" if beyond else ""), "records"))
            out.append(_copies(key, "nk" + tag, 1, CAP_PLANS["records"]["hash_slots"] // 2 + beyond + w - 1, run, rvs, "caps/nk",
                               "nk at hash_slots / 2%s" % (" + 1" if beyond else ""), "records"))
            # shared words: the region is N but for 128 copies of two adjacent words from the middle of the range (a diagonal each, too
            # few words for a segment) -- hit_cap shared words -- and, beyond, a copy of the first of the two
            out.append(_copies(key, "hit" + tag, CAP_PLANS["records"]["hit_cap"] // 2, 100, 2, rvs, "caps/words",
                               "shared words at hit_cap%s" % (" + 1" if beyond else ""), "records", one_more_word=beyond))
    return out


CAP_PLANS = dict(records=dict(hash_slots=256, hit_cap=256, seg_cap=8, out_cap=4), segments=dict(hash_slots=256, hit_cap=256, seg_cap=8, out_cap=16))
KEY_LIMIT_NK = 4096


def key_limit_nn():
    """the most region words a range of KEY_LIMIT_NK words can be searched against: (nn + nk - 1) << mbits <= 0xfffffff0"""
    return (0xfffffff0 >> 12) - (KEY_LIMIT_NK - 1)


def _key_limit():
    S, rng = shape(model("nt")), _rng("keylimit")
    w = S["width"]
    q = _query(S, rng, KEY_LIMIT_NK + w - 1)
    n = words_to_residues(S, min_words(S) + 30)
    out = []
    for beyond in (0, 1):
        b = np.full(key_limit_nn() + beyond + w - 1, N, dtype=np.uint8)
        b[len(b) - n - 5:len(b) - 5] = q[100:100 + n]
        out.append(Case("nt", "key_limit", "a range of %d words against %d region words: the 32-bit sort key at its limit%s" % (KEY_LIMIT_NK, key_limit_nn() + beyond, " + 1" if beyond else ""),
                        q, 0, len(q), None, len(b), None, 0, plan="key_limit", region=b))
    return out


def _mixed():
    out = []
    for i, key in enumerate(("nt", "aa")):
        S, rng = shape(model(key)), _rng("mixed" + key)
        for a_len in (30, 300, 5000):
            q = _query(S, rng, a_len)
            n = min(a_len, words_to_residues(S, min_words(S) + 12))
            out.append(Case(key, "mixed_batch", "queries of 30, 300 and 5000 residues in one call: the slots follow the longest", q, 0, a_len, 40, S["bbt"] * min(a_len, 400) + 300,
                            _runs(a_len, (a_len - n if a_len == 30 else 20, n)), (i + a_len) % 2, plan="mixed"))
    return out


def _reuse():
    """tasks in threes for a launch of three waves: wave w serves tasks w, w + 3, ..: a task with many words and segments, then an
    empty one, then one with a single word, on the same wave's LDS"""
    out = []
    for key, n_tasks in (("nt", 200), ("aa", 100)):
        S = shape(model(key))
        w = S["width"]
        kinds = []
        for k in range(n_tasks):
            kind = (k // 3) % 3
            name = "reuse%s%d" % (key, k)
            if kind == 0:
                c = _copies(key, name, 5 + k % 3, 90, min_words(S) + 3 + k % 4, k % 2, "reuse", "many words and segments", "reuse")
            elif kind == 1:
                rng = _rng(name)
                c = Case(key, "reuse", "an empty task: the range is shorter than a word", _query(S, rng, 40), 5, 5 + w - 1, 0, 100, _runs(40, (5, w - 1)), k % 2, plan="reuse")
            else:
                rng = _rng(name)
                q = _query(S, rng, 60)
                b = np.full(S["bbt"] * w + 40, N, dtype=np.uint8)
                b[20:20 + S["bbt"] * w] = q[10:10 + w] if S["bbt"] == 1 else np.concatenate([CODON[int(c)] for c in q[10:10 + w]])
                c = Case(key, "reuse", "one shared word", q, 0, 60, None, len(b), None, k % 2, plan="reuse", region=b)
            kinds.append(c)
        out += kinds
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_words_recipes() + _stretch_recipes() + _range_recipes() + _cap_recipes() + _key_limit() + _mixed() + _reuse())


PLANS = dict(CAP_PLANS, key_limit={}, mixed={}, reuse=dict(n_waves=3))
PLANS[None] = {}


@functools.lru_cache(maxsize=None)
def requests():
    """the calls: one per (model, a_exgl, a_exgr, plan) -- dict(name, key, model, shape, bbt, exg, plan (the fields given explicitly),
    queries, ranges, tlen, genome, chr_off, tasks [(query, chr, base, len, rvs)], cases)"""
    groups = {}
    for c in cases():
        groups.setdefault((c.key, c.exg, c.plan), []).append(c)
    out = []
    for (key, exg, plan), cs in groups.items():
        name = "%s/exg%d%d/%s" % (key, exg[0], exg[1], plan or "default")
        rng = _rng("genome " + name)
        chroms, tasks = [[], []], []
        at = [0, 0]
        for i, c in enumerate(cs):
            ch = i % 2 if plan != "key_limit" else i
            b = c.region_as_planted(_rng("region %s %d" % (name, i)))
            lead = NUC[rng.integers(0, 4, size=int(rng.integers(5, 20)))]
            chroms[ch] += [lead, other_strand(b) if c.rvs else b]
            tasks.append((i, ch, at[ch] + len(lead), len(b), int(c.rvs)))
            at[ch] += len(lead) + len(b)
        for ch in range(2):
            chroms[ch].append(NUC[rng.integers(0, 4, size=11)])
        seqs = [np.concatenate(x).astype(np.uint8) for x in chroms]
        m = model(key)
        out.append(dict(name=name, key=key, model=m, shape=shape(m), bbt=3 if m.dvsp == 1 else 1, exg=exg, plan=dict(PLANS[plan]),
                        queries=[c.q for c in cs], ranges=[(c.left, c.right) for c in cs],
                        tlen=np.array([len(c.q) if c.tlen is None else c.tlen for c in cs], dtype=np.int32),
                        genome=np.concatenate(seqs), chr_off=np.array([0, len(seqs[0]), len(seqs[0]) + len(seqs[1])], dtype=np.int64),
                        tasks=tasks, cases=cs))
    return tuple(out)
