"""Indexes and queries made for the paths of the block vote (spaln_amd/csrc/spdp_blk_vote.hip) that the recorded fixtures do not
reach: posting lists read in several chunks, the two ways of merging two lists, tables that grow under a query, many phases, many
chromosomes, queries longer than the wave's residue cache.  tests/test_vote_cases.py holds every class to the effect it is named
for by the oracle alone (oracle/spdp_oracle_blk.c); tests/test_gpu_vote_cases.py runs them through spdp_blk_vote against the
oracle's records, int for int, and asks the kernel's path counters (spdp_blk_vote_stats) whether the paths ran.

An index is the dict blocks.BlockIndex(eng, fx) and oracle.blk.index_of(fx) take.  Its tables come from the oracle's restatement of
the index builder (oracle.blk.index_build, held to the reference's own files elsewhere) on a synthetic genome; its parameter
record is a committed fixture's with the entries a case states overwritten; single posting lists are patched by hand where a
class needs an exact length (any ascending list of block numbers is a valid index for both sides).  Seeded; no device code."""
from __future__ import annotations

import functools
import os

import numpy as np

from oracle import blk as oblk
from tests import spdg

HERE = os.path.dirname(os.path.abspath(__file__))
NT = np.array([2, 3, 5, 9], dtype=np.uint8)          # A C G T in the reference's nucleotide codes
_COMP = np.zeros(32, dtype=np.uint8)
_COMP[[2, 3, 5, 9, 16]] = [9, 5, 3, 2, 16]
_DIGIT = np.full(32, 4, dtype=np.int64)
_DIGIT[[2, 3, 5, 9]] = [0, 1, 2, 3]
P = oblk.PRM
STOPS = (0, 1, 0, 2, 0, 1, 3, 0, 4, 1, 0, 2, 0, 1, 3, 0)     # the stop_at a class's queries ask for, in turn


@functools.lru_cache(maxsize=None)
def template(name: str) -> dict:
    return spdg.load(os.path.join(HERE, "golden", name + ".spdg"))


def random_dna(rng, n: int) -> np.ndarray:
    return NT[rng.integers(0, 4, size=int(n))]


def mutate(rng, s: np.ndarray, sub: float) -> np.ndarray:
    s = s.copy()
    hit = rng.random(s.size) < sub
    s[hit] = NT[rng.integers(0, 4, size=int(hit.sum()))]
    return s


def revcomp(s: np.ndarray) -> np.ndarray:
    return _COMP[np.asarray(s)[::-1]]


def make_genome(rng, chrom_lens, element=None, copies=0, div=0.03):
    """random chromosomes with `copies` diverged copies of `element` put over them (either strand); -> codes, chr_off"""
    chroms = [random_dna(rng, n) for n in chrom_lens]
    for _ in range(copies):
        c = chroms[int(rng.integers(len(chroms)))]
        if c.size <= element.size + 10:
            continue
        at = int(rng.integers(0, c.size - element.size))
        e = mutate(rng, element, div)
        c[at:at + e.size] = e if rng.random() < 0.5 else revcomp(e)
    off = np.zeros(len(chroms) + 1, dtype=np.int64)
    off[1:] = np.cumsum([c.size for c in chroms])
    return np.concatenate(chroms), off


def index_fx(tmpl: str, codes, off, nshift=None, blklen=None, **prm) -> dict:
    """the index of a genome with the builder parameters and the search parameters of fixture `tmpl`, but for nshift / blklen and
    the entries of the parameter record named in `prm`"""
    tm = template(tmpl)
    bp = oblk.build_params_of(tm)
    if nshift is not None:
        bp.nshift = nshift
    if blklen is not None:
        bp.blklen = blklen
    return with_prm(_fx_of_built(tm, oblk.index_build(codes, off, bp), bp.nshift, bp.blklen, len(off) - 1), **prm)


def _fx_of_built(tm: dict, built: dict, nshift: int, blklen: int, n_chr: int) -> dict:
    rec = np.asarray(tm["blk_prm"], dtype=np.int32).copy()
    rec[P["nshift"]], rec[P["blklen"]] = nshift, blklen
    rec[P["n_chr"]], rec[P["nseg"]] = n_chr, int(built["chr"][-1])
    rec[P["avrscr"]], rec[P["maxblk"]], rec[P["wordno"]] = built["avrscr"], built["maxblk"], built["word_no"]
    # the thresholds of the template follow its average word score: kept in proportion (the vote takes them as given)
    rscr = (np.asarray(tm["blk_rscrtab"], dtype=np.int64) * int(built["avrscr"]) // int(tm["blk_prm"][P["avrscr"]])).astype(np.int32)
    fx = dict(blk_prm=rec, blk_pb2c=np.frombuffer(np.asarray(built["b2c"], dtype=np.float64).tobytes(), dtype=np.uint8).copy(),
              blk_cfact=np.asarray(tm["blk_cfact"]).copy(), blk_rscrtab=rscr, blk_nblk=built["nblk"], blk_wscr=built["wscr"],
              blk_blkp=built["blkp"], blk_blkb=built["blkb"].astype(np.uint32), blk_convtab=np.asarray(tm["blk_convtab"]).copy(),
              blk_chr=built["chr"], blk_bitpat=np.asarray(tm["blk_bitpat"]).copy())
    return fx


def with_prm(fx: dict, **prm) -> dict:
    """a copy of the index (tables shared) with entries of its parameter record overwritten"""
    out = dict(fx)
    out["blk_prm"] = np.asarray(fx["blk_prm"], dtype=np.int32).copy()
    for k, v in prm.items():
        out["blk_prm"][P[k]] = v
    return out


def prm_of(fx: dict, name: str) -> int:
    return int(fx["blk_prm"][P[name]])


def patch_list(fx: dict, word: int, blocks) -> None:
    """word's posting list replaced by `blocks` (ascending block numbers; a trailing 0 is the reference's end mark), in place"""
    blocks = np.asarray(blocks, dtype=np.uint32)
    fx["blk_nblk"] = np.asarray(fx["blk_nblk"]).view(np.uint16).copy() if not fx["blk_nblk"].flags.writeable else fx["blk_nblk"].view(np.uint16)
    fx["blk_blkp"][word] = fx["blk_blkb"].size + 1
    fx["blk_nblk"][word] = blocks.size
    if fx["blk_wscr"][word] <= 0:
        fx["blk_wscr"][word] = prm_of(fx, "avrscr")
    fx["blk_blkb"] = np.concatenate([fx["blk_blkb"], blocks])
    fx["blk_prm"][P["maxblk"]] = max(prm_of(fx, "maxblk"), int(blocks.size))
    fx["blk_prm"][P["wordno"]] = fx["blk_blkb"].size


def list_lengths(fx: dict) -> np.ndarray:
    return np.where(np.asarray(fx["blk_blkp"]) != 0, np.asarray(fx["blk_nblk"]).view(np.uint16).astype(np.int64), 0)


# ---- contiguous k-mers (kk = 1): the words of a query on both strands -----------------------------------------------------------
def kmer_codes(q: np.ndarray, k: int):
    """(forward words, words of the other strand) of every window of q; -1 where a window holds no plain nucleotide"""
    d = _DIGIT[np.asarray(q, dtype=np.int64)]
    n = d.size - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    fwd = np.zeros(n, np.int64); rev = np.zeros(n, np.int64); bad = np.zeros(n, bool)
    for i in range(k):
        w = d[i:i + n]
        bad |= w > 3
        fwd = fwd * 4 + w
        rev += (3 - w) * 4 ** i
    fwd[bad] = -1; rev[bad] = -1
    return fwd, rev


def word_of(s: str) -> int:
    c = 0
    for ch in s:
        c = c * 4 + "ACGT".index(ch)
    return c


def seq_of(s: str) -> np.ndarray:
    return NT[["ACGT".index(ch) for ch in s]]


def quieten(rng, fx: dict, q: np.ndarray, limit: int, keep=()) -> np.ndarray:
    """q with every window whose word (either strand) has a list of `limit` entries or more rewritten, but for the words in `keep`"""
    k = prm_of(fx, "ktuple")
    lens = list_lengths(fx)
    q = q.copy()
    frozen = np.zeros(q.size, bool)
    for _ in range(200):
        f, r = kmer_codes(q, k)
        loud = np.zeros(f.size, bool)
        for w in (f, r):
            ok = w >= 0
            loud |= ok & (lens[np.where(ok, w, 0)] >= limit) & ~np.isin(w, keep)
        for w in (f, r):
            for at in np.nonzero(np.isin(w, keep))[0]:
                frozen[at:at + k] = True
        if not loud.any():
            return q
        for at in np.nonzero(loud)[0]:
            free = [i for i in range(at, at + k) if not frozen[i]]
            if free:
                q[free[int(rng.integers(len(free)))]] = NT[rng.integers(0, 4)]
    raise RuntimeError("quieten: no quiet sequence found")


def plant(q: np.ndarray, marker: np.ndarray, every: int, rng) -> np.ndarray:
    """the marker word written into q about every `every` residues (both ends included), alternately as it is and as the other
    strand reads it"""
    q = q.copy()
    at, i = 3, 0
    while at + marker.size <= q.size - 3:
        q[at:at + marker.size] = marker if i % 2 == 0 else revcomp(marker)
        at += every + int(rng.integers(0, 7)); i += 1
    return q


EARLY = (0, 0, 1, 0, 0, 2, 0, 0)                               # ... of a class whose queries hardly get beyond their first call


def _class(queries, start=0, stops=STOPS):
    """[(codes, left, right)] -> the class's entries, each asked for the next stop_at of `stops`"""
    out = []
    for i, q in enumerate(queries):
        codes, left, right = q if isinstance(q, tuple) else (q, 0, len(q))
        out.append(dict(codes=np.ascontiguousarray(codes, dtype=np.uint8), left=int(left), right=int(right), stop_at=stops[(start + i) % len(stops)]))
    return out


def fragment(rng, codes, lo, hi, sub=0.02):
    n = int(rng.integers(lo, hi + 1))
    at = int(rng.integers(0, len(codes) - n))
    f = mutate(rng, codes[at:at + n], sub)
    return f if rng.random() < 0.5 else revcomp(f)


# ---- the indexes ------------------------------------------------------------------------------------------------------------------
LONG_MARKS = {63: "ACGGTCA", 64: "CCGATAG", 65: "GTTACGC", 127: "TGCCGAA", 128: "AGGCTTC", 129: "CTAGTCG"}
ZERO_MARK = "TTGACCA"
N_PER_CLASS = 16


@functools.lru_cache(maxsize=None)
def long_index() -> dict:
    """a repetitive genome at kk = 1 (the parameters of blk_k1): eight chromosomes, 700 copies of a 600 nt element at 3 %.  The
    element's words have lists of up to ninety blocks (the index holds every seventh word of the genome).  Classes by the longest list a query votes with: exact lengths
    around the chunk of 64 and the LDS merge's 128 from a patched marker word in an otherwise quiet query; `longest`: copies of
    the element (and a marker word in nine blocks of twenty); `noise`: random sequences, which vote and reach nothing much; `end_mark`: a marker word whose list of 61 entries holds the end mark 0
    at its 41st"""
    rng = np.random.default_rng(20260)
    element = random_dna(rng, 600)
    codes, off = make_genome(rng, [110000 + 7000 * i for i in range(8)], element, 700, 0.03)
    fx = index_fx("blk_k1", codes, off)
    nseg = prm_of(fx, "nseg")
    classes = {}
    for n, mark in LONG_MARKS.items():
        # half the list a stretch of neighbouring blocks (their runs meet in the hash), half scattered
        first = int(rng.integers(5, nseg - n - 5))
        stretch = np.arange(first, first + n // 2)
        rest = np.setdiff1d(np.arange(1, nseg), stretch)
        blocks = np.sort(np.concatenate([stretch, rng.choice(rest, size=n - stretch.size, replace=False)]))
        patch_list(fx, word_of(mark), blocks)
    big = np.sort(rng.choice(np.arange(1, nseg), size=nseg * 9 // 20, replace=False))
    patch_list(fx, word_of("GGATCCA"), big)
    # a list with the end mark inside: 40 blocks, 0, 20 more that no one may read
    zero_list = np.sort(rng.choice(np.arange(1, nseg), size=60, replace=False))
    patch_list(fx, word_of(ZERO_MARK), np.concatenate([zero_list[:40], [0], zero_list[40:]]))
    keep_all = [word_of(m) for m in LONG_MARKS.values()] + [word_of("GGATCCA"), word_of(ZERO_MARK)]
    for n, mark in LONG_MARKS.items():
        w = word_of(mark)
        qs = []
        for i in range(N_PER_CLASS):
            f = fragment(rng, codes, 150, 900)
            f = quieten(rng, fx, plant(f, seq_of(mark), 45, rng), n, keep=[w])
            lo = int(rng.integers(0, 3)); hi = f.size - int(rng.integers(0, 3))
            qs.append((f, lo, hi))
        classes[str(n)] = _class(qs)
    qs = [mutate(rng, element, 0.03)[int(rng.integers(0, 100)):int(rng.integers(350, 600))] for _ in range(N_PER_CLASS - 4)]
    qs += [plant(fragment(rng, codes, 300, 800), seq_of("GGATCCA"), 60, rng) for _ in range(4)]
    classes["longest"] = _class([q if i % 2 else revcomp(q) for i, q in enumerate(qs)])
    classes["noise"] = _class([random_dna(rng, int(rng.integers(60, 700))) for _ in range(N_PER_CLASS)])
    classes["end_mark"] = _class([(lambda f: quieten(rng, fx, plant(f, seq_of(ZERO_MARK), 45, rng), 61, keep=[word_of(ZERO_MARK)]))(fragment(rng, codes, 150, 900))
                              for _ in range(N_PER_CLASS)])
    return dict(name="long", fx=fx, classes=classes, genome=(codes, off), element=element, keep=keep_all)


def spaced_words(fx: dict, q: np.ndarray, ss: int):
    """the forward words of patterns 0 and 1 at query position ss (-1: the window leaves the query or holds no plain nucleotide)"""
    bp = np.asarray(fx["blk_bitpat"], dtype=np.int64)
    out, at = [], 0
    for _ in range(2):
        weight, width = int(bp[at]), int(bp[at + 1])
        exam = bp[at + 3:at + 3 + weight]
        at += 3 + 2 * weight
        if ss + width > q.size:
            out.append(-1); continue
        d = _DIGIT[q[ss + exam].astype(np.int64)]
        out.append(-1 if (d > 3).any() else int(sum(int(x) * 4 ** (weight - 1 - i) for i, x in enumerate(d))))
    return out


@functools.lru_cache(maxsize=None)
def merge_index() -> dict:
    """five spaced patterns (kk = 3, the parameters of blk_k3) at blklen 256: every word votes with the lists of its first two
    patterns, merged.  Classes: `lds` both lists at most 128; `lane` one or both longer (the one-lane merge); `shared` two lists
    that share nine blocks in ten; `disjoint` two that share none; `zero` a first list with the end mark 0 half way (the reference reads
    no entry behind it) while the second goes on.  The lists of the last three are patched onto the words at the left end of their queries."""
    rng = np.random.default_rng(20261)
    element = random_dna(rng, 900)
    codes, off = make_genome(rng, [50000 + 9000 * i for i in range(6)], element, 160, 0.03)
    fx = index_fx("blk_k3", codes, off, blklen=256)
    nseg = prm_of(fx, "nseg")
    lens = list_lengths(fx)
    classes = {}
    pool = [fragment(rng, codes, 200, 800) for _ in range(60)] + [mutate(rng, element, 0.03)[int(rng.integers(0, 100)):int(rng.integers(400, 900))] for _ in range(40)]
    taken = set()

    def patched(kind, n_q):
        qs = []
        for i in range(n_q):
            q = fragment(rng, codes, 250, 700, sub=0.0)
            for ss in range(0, 70, 7):                      # (phase 0 of the scan from the left end meets these first)
                w0, w1 = spaced_words(fx, q, ss)
                if w0 < 0 or w1 < 0 or w0 == w1 or w0 in taken or w1 in taken:
                    continue
                taken.update((w0, w1))
                na, nb = (int(rng.integers(40, 120)), int(rng.integers(40, 120))) if i % 2 else (int(rng.integers(130, 260)), int(rng.integers(70, 200)))
                a = np.sort(rng.choice(np.arange(1, nseg), size=na, replace=False))
                if kind == "shared":
                    b = a.copy()
                    swap = rng.choice(b.size, size=max(1, b.size // 10), replace=False)
                    b[swap] = rng.choice(np.setdiff1d(np.arange(1, nseg), a), size=swap.size, replace=False)
                    b = np.unique(b)
                elif kind == "disjoint":
                    b = np.sort(rng.choice(np.setdiff1d(np.arange(1, nseg), a), size=nb, replace=False))
                else:                                           # zero: the first list ends in the end mark, the second holds later blocks
                    b = np.sort(rng.choice(np.arange(1, nseg), size=nb, replace=False))
                    a = a[a < int(b[-1])]
                    a = np.concatenate([a[:a.size // 2], [0], a[a.size // 2:]]).astype(np.int64)   # (what follows the mark is never read)
                patch_list(fx, w0, a)
                patch_list(fx, w1, b)
            qs.append(q)
        return qs

    classes["shared"] = _class(patched("shared", N_PER_CLASS))
    classes["disjoint"] = _class(patched("disjoint", N_PER_CLASS))
    classes["zero"] = _class(patched("zero", N_PER_CLASS))
    classes["lds"] = _class(pool[:60][:N_PER_CLASS + 8])
    classes["lane"] = _class(pool[60:][:N_PER_CLASS + 8])
    return dict(name="merge", fx=fx, classes=classes, genome=(codes, off))


GROW_GEOMETRIES = {                                             # name -> the table under test, its geometry
    "grow_hh7": ("run_hash", dict(hh_size1=7, hh_size2=5)),
    "grow_hh13": ("run_hash", dict(hh_size1=13, hh_size2=8)),
    "grow_hh31": ("run_hash", dict(hh_size1=31, hh_size2=8)),
    "grow_hh127": ("run_hash", dict(hh_size1=127, hh_size2=8)),
    "grow_hb": ("runs", dict(hb_size1=3, hb_size2=2)),
    "grow_ha": ("hits", dict(ha_size1=3, ha_size2=2, nascr=7)),
}
TABLE_SHARE = 10                                                # at most one query in ten of a grow index may end as TABLE


def measure(fx: dict, e: dict):
    """the oracle on one entry: dict(want = (vote record, pairs record) or None, forced, grows, paths, rounds, calls)"""
    ix, keep = _oracle_index(id(fx), fx)
    want = oblk.vote(ix, e["codes"], e["left"], e["right"], e["stop_at"])
    return dict(want=want, forced=bool(want is not None and oblk.last_vote_was_forced()), grows=oblk.last_grows(), paths=oblk.last_paths(),
                rounds=oblk.last_rounds(), calls=oblk.last_calls())


_IX = {}


def _oracle_index(key, fx):
    if key not in _IX:
        _IX[key] = oblk.index_of(fx) + (fx,)                   # (the fx kept: its id stays its own)
    return _IX[key][:2]


def oracle_index(fx):
    return _oracle_index(id(fx), fx)[0]


@functools.lru_cache(maxsize=None)
def grow_indexes() -> tuple:
    """the long index's tables with small table geometries: the run hash at 7, 13, 31 and 127 slots, the run lists' position table at 3,
    the hit lists' at 3 under 7 entries.  Classes by the growths of the table under test in the oracle's call: 0, 1, 2, 3 and 4 or more -- the
    product ends a query as TABLE at the fourth growth of any one table, and such queries stay under a tenth of an index's."""
    base = long_index()
    rng = np.random.default_rng(20262)
    codes, _ = base["genome"]
    pool = [e for c in base["classes"].values() for e in c]
    pool += _class([quieten(rng, base["fx"], fragment(rng, codes, 80, 400), lim) for lim in (36, 40, 44, 48, 56, 62) for _ in range(6)], start=3)
    pool += _class([random_dna(rng, int(rng.integers(40, 200))) for _ in range(20)], start=5)
    out = []
    for name, (table, geo) in GROW_GEOMETRIES.items():
        fx = with_prm(base["fx"], **geo)
        classes = {str(k): [] for k in range(5)}
        table_ones = []
        for e in pool:
            m = measure(fx, e)
            g = str(min(4, m["grows"][table]))
            if max(m["grows"].values()) >= 4:
                table_ones.append((g, e, m))
            elif len(classes[g]) < 22:
                classes[g].append((e, m))
        # the queries the product will end as TABLE: one in ten of the index at the most
        n_plain = sum(len(v) for v in classes.values())
        for g, e, m in table_ones[:n_plain // (TABLE_SHARE - 1)]:
            classes[g].append((e, m))
        out.append(dict(name=name, fx=fx, classes={f"{table}_{k}": v for k, v in classes.items() if v}, table=table))
    # a class is the growths of one table whatever the geometry: those with fewer than ten reaching queries over all geometries go
    reach = {}
    for ix in out:
        for c, v in ix["classes"].items():
            reach[c] = reach.get(c, 0) + sum(m["want"] is not None for _, m in v)
    for ix in out:
        ix["classes"] = {c: [e for e, _ in v] for c, v in ix["classes"].items() if reach[c] >= 10}
    return tuple(out)


@functools.lru_cache(maxsize=None)
def phases_indexes() -> tuple:
    """Nshift 1, 12, 13 and 32 (the kernel fetches the list heads of up to 12 phases ahead; 32 is the last slot of its scan
    positions), and Nshift 7 with queries long and empty enough that the scan opens more than 255 phases: the epoch counter of the
    run hash comes round and the table is wiped"""
    rng = np.random.default_rng(20263)
    codes, off = make_genome(rng, [40000, 52000, 47000], random_dna(rng, 700), 40, 0.03)
    out = []
    for ns in (1, 12, 13, 32):
        fx = index_fx("blk_k1", codes, off, nshift=ns, blklen=2048 if ns == 1 else 1024)
        qs = [fragment(rng, codes, 120 + 4 * ns, 900) for _ in range(N_PER_CLASS + (8 if ns > 12 else 0))]
        out.append(dict(name=f"phases_{ns}", fx=fx, classes={f"nshift_{ns}": _class(qs, stops=EARLY if ns > 12 else STOPS)}))
    fx = index_fx("blk_k1", codes, off)
    qs = [np.concatenate([fragment(rng, codes, 100, 300), random_dna(rng, int(rng.integers(900, 2000))), fragment(rng, codes, 100, 300)]) for _ in range(8)]
    qs += [random_dna(rng, int(rng.integers(1200, 2000))) for _ in range(8)]
    out.append(dict(name="phases_epochs", fx=fx, classes={"epochs": _class(qs)}))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chromosomes_index() -> dict:
    """300 chromosomes, forty of them a few dozen residues long or empty and lying, some in a row, between the others: an empty
    one begins in the block the next one begins in.  Classes: `ends` fragments that begin or end with a chromosome (the first and the last of the genome among them);
    `tiny` fragments that run across the tiny chromosomes; `inner` fragments from inside"""
    rng = np.random.default_rng(20264)
    lens = []
    for i in range(260):
        lens.append(int(rng.integers(2500, 6000)))
        if i % 13 == 5:
            lens += [0 if (i + k) % 3 else int(rng.integers(20, 120)) for k in range(1 + (i % 3))]
    lens = lens[:300] + [3000] * max(0, 300 - len(lens))
    codes, off = make_genome(rng, lens)
    fx = index_fx("blk_k1", codes, off)
    big = [c for c in range(len(lens)) if lens[c] > 1000]
    ends = []
    for i, c in enumerate([big[0], big[-1]] + [big[int(x)] for x in rng.integers(0, len(big), size=N_PER_CLASS - 2)]):
        n = int(rng.integers(200, 700))
        f = codes[off[c]:off[c] + n] if i % 2 == 0 else codes[off[c + 1] - n:off[c + 1]]
        f = mutate(rng, f, 0.01)
        ends.append(f if i % 4 < 2 else revcomp(f))
    ends[0] = codes[:400].copy(); ends[1] = codes[-400:].copy()
    tiny = []
    small = [c for c in range(len(lens)) if lens[c] < 1000]
    for i in range(N_PER_CLASS):
        c = small[int(rng.integers(len(small)))]
        lo = max(0, int(off[c]) - int(rng.integers(100, 500))); hi = min(codes.size, int(off[c + 1]) + int(rng.integers(100, 500)))
        f = mutate(rng, codes[lo:hi], 0.01)
        tiny.append(f if i % 2 else revcomp(f))
    inner = [fragment(rng, codes, 150, 800) for _ in range(N_PER_CLASS)]
    return dict(name="chromosomes", fx=fx, classes=dict(ends=_class(ends), tiny=_class(tiny), inner=_class(inner)), genome=(codes, off))


@functools.lru_cache(maxsize=None)
def long_queries_index() -> dict:
    """queries around the wave's residue cache of 2048: 2047, 2048, 2049 and 5000 residues (pieces of the genome in a row, as a
    full-length cDNA of many exons is), the searched range inside the query and at its ends; `short`: below ShortQuery (the scan's
    two ends do not wait for each other), the last eight too short for one word of every phase -- no call at all"""
    rng = np.random.default_rng(20265)
    codes, off = make_genome(rng, [70000, 90000, 80000], random_dna(rng, 800), 60, 0.03)
    fx = index_fx("blk_k1", codes, off)
    classes = {}
    for n in (2047, 2048, 2049, 5000):
        qs = []
        for i in range(12):
            parts, have = [], 0
            at = int(rng.integers(0, codes.size - 3 * n))
            while have < n:
                m = int(rng.integers(150, 600))
                parts.append(mutate(rng, codes[at:at + m], 0.01)); have += m
                at += m + int(rng.integers(200, 1500))
            q = np.concatenate(parts)[:n]
            if i % 3 == 2:
                q = revcomp(q)
            left, right = [(0, n), (0, n), (int(rng.integers(1, 40)), n - int(rng.integers(1, 40))), (n - 700, n), (0, 600), (n // 2 - 300, n // 2 + 400)][i % 6]
            qs.append((q, left, right))
        classes[str(n)] = _class(qs)
    shortq = prm_of(fx, "shortquery")
    width = int(fx["blk_bitpat"][1]); ns = prm_of(fx, "nshift")
    classes["short"] = _class([fragment(rng, codes, 24, shortq - 1, sub=0.0) for _ in range(N_PER_CLASS + 8)] +
                              [fragment(rng, codes, 1, ns + width, sub=0.0) for _ in range(6)] +
                              [(fragment(rng, codes, 300, 300, sub=0.0), 100, 100 + ns + width) for _ in range(2)], stops=EARLY)
    return dict(name="long_queries", fx=fx, classes=classes)


AA_ORDER = "ARNDCQEGHILKMFPSTWYV"                                # amino-acid codes 3 .. 22 of the reference's tron alphabet
P_MARKS = {65: (0, 5, 11, 17), 129: (3, 9, 14, 1), 300: (7, 2, 19, 12)}      # marker words (four residues) -> the length of their list


def _back_translate(aa_idx) -> np.ndarray:
    """a DNA sequence (codes) whose frame 0 reads the residues: the first codon of the standard code for each"""
    first = {}
    for g, a in enumerate(oblk._STANDARD_CODE):
        first.setdefault(a, g)
    out = []
    for k in aa_idx:
        g = first[AA_ORDER[int(k)]]
        out += [g >> 4, (g >> 2) & 3, g & 3]
    return NT[out]


@functools.lru_cache(maxsize=None)
def protein_indexes() -> tuple:
    """one translated index (oracle.blk.index_build_tron, the parameters of blk_p1: amino-acid words of four residues, level 0 of
    its run hash 157 291 slots, in HBM) of a genome with 40 copies of a coding element, and the same tables with a run hash of 31
    slots.  Classes of the first by the longest list a query votes with (patched marker words of 65, 129 and 300 blocks in protein
    queries cut from the element), of the second by the growths of the run hash."""
    from spaln_amd import defaults
    rng = np.random.default_rng(20266)
    tm = template("blk_p1")
    prot = rng.integers(0, 20, size=320)
    codes, off = make_genome(rng, [140000, 162000, 150000], _back_translate(prot), 40, 0.02)  # (some 440 blocks)
    t = np.asarray(tm["blk_prm"])
    bp = oblk.build_params_p(int(t[P["ktuple"]]), int(t[P["nshift"]]), int(t[P["blklen"]]), int(t[P["maxgene"]]), int(t[P["afact"]]), 0,
                             bytes(np.asarray(tm["blk_convtab"]).astype(np.uint8))[:27], defaults.BLOCK_ACOMP_20)
    fx = _fx_of_built(tm, oblk.index_build_tron(codes, off, bp), bp.b.nshift, bp.b.blklen, len(off) - 1)
    nseg = prm_of(fx, "nseg")
    for n, mark in P_MARKS.items():
        first = int(rng.integers(3, nseg - n // 2 - 3))
        stretch = np.arange(first, first + n // 3)
        rest = np.setdiff1d(np.arange(1, nseg), stretch)
        patch_list(fx, int(sum(c * 20 ** (3 - i) for i, c in enumerate(mark))), np.sort(np.concatenate([stretch, rng.choice(rest, size=n - stretch.size, replace=False)])))
    classes, pool = {}, []
    for n, mark in P_MARKS.items():
        qs = []
        for i in range(N_PER_CLASS + 12):
            lo = int(rng.integers(0, 120)); q = prot[lo:lo + int(rng.integers(70, 200))].copy()
            hit = rng.random(q.size) < 0.03
            q[hit] = rng.integers(0, 20, size=int(hit.sum()))
            for at in range(2, q.size - 6, 23 + i % 5):
                q[at:at + 4] = mark
            qs.append((q + 3).astype(np.uint8))
        classes[f"p_{n}"] = _class(qs, stops=EARLY)
        pool += classes[f"p_{n}"]
    pool += _class([(prot[int(a):int(a) + int(n)] + 3).astype(np.uint8) for a, n in zip(rng.integers(0, 150, size=24), rng.integers(40, 170, size=24))], start=2, stops=EARLY)
    small = with_prm(fx, hh_size1=31, hh_size2=8)
    grown = {str(k): [] for k in range(5)}
    table_ones = []
    for e in pool:
        m = measure(small, e)
        g = str(min(4, m["grows"]["run_hash"]))
        if max(m["grows"].values()) >= 4:
            table_ones.append((g, e, m))
        elif len(grown[g]) < 30:
            grown[g].append((e, m))
    for g, e, m in table_ones[:sum(len(v) for v in grown.values()) // (TABLE_SHARE - 1)]:
        grown[g].append((e, m))
    grown = {f"p_run_hash_{k}": [e for e, _ in v] for k, v in grown.items() if sum(m["want"] is not None for _, m in v) >= 10}
    return (dict(name="protein", fx=fx, classes=classes), dict(name="protein_grow", fx=small, classes=grown, table="run_hash"))


WIDE = 1 << 24


@functools.lru_cache(maxsize=None)
def wide_index() -> dict:
    """the long index's tables with 2^24 added to every block number and to every first block of the chromosome table, nseg raised
    by the same: block numbers no longer fit beside an epoch byte, the run hash is wiped at every phase.  Five queries (a wave's
    slab of such an index is a GiB, the oracle's score arrays a quarter of that per call)."""
    base = long_index()
    fx = dict(base["fx"])
    b = np.asarray(fx["blk_blkb"], dtype=np.uint32).copy()
    b[b != 0] += WIDE
    chr_ = np.asarray(fx["blk_chr"], dtype=np.int32).copy()
    chr_[1::2] += WIDE
    fx["blk_blkb"], fx["blk_chr"] = b, chr_
    fx = with_prm(fx, nseg=prm_of(fx, "nseg") + WIDE)
    pick = [base["classes"][c][i] for c, i in (("65", 0), ("129", 2), ("longest", 1), ("63", 4), ("end_mark", 0))]
    return dict(name="wide", fx=fx, classes={"wide": [dict(e, stop_at=s) for e, s in zip(pick, (0, 0, 1, 0, 2))]})


def _find_chr(first, n_chr, blk, bracket=None):
    """SrchBlk::findChrNo as the oracle and the kernel restate it; bracket = (bclw, bcup, bcce) or None for the whole table"""
    lo, hi = 0, n_chr
    if bracket is not None:
        lo = max(int(bracket[0] + bracket[2] * (blk - 1)) - 1, 0)
        hi = min(int(bracket[1] + bracket[2] * (blk - 1)) + 1, n_chr)
        if first[lo] > blk:
            lo = 0
        if first[hi] < blk:
            hi = n_chr
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if first[mid] > blk:
            hi = mid
        elif first[mid + 1] > blk:
            return mid
        else:
            lo = mid
    return lo if first[hi] > blk else hi


@functools.lru_cache(maxsize=None)
def bracket_index() -> dict:
    """the 300-chromosome tables with a linear estimate block -> chromosome that is tight (half a chromosome either way): where
    empty chromosomes share a first block the bracket then ends inside their run, and the search gives the block to another
    chromosome than a bisection of the whole table does.  The builder's own estimate has slope 0 (every bracket opens to the whole
    table), which is why the class sets its own.  Queries: pieces of exactly the blocks where the two disagree."""
    base = chromosomes_index()
    rng = np.random.default_rng(20267)
    codes, off = base["genome"]
    fx = dict(base["fx"])
    tab = np.asarray(fx["blk_chr"]).reshape(-1, 2).astype(np.int64)
    first, n_chr, nseg, blklen = tab[:, 1], prm_of(fx, "n_chr"), prm_of(fx, "nseg"), prm_of(fx, "blklen")
    bcce = n_chr / (nseg - 1)
    mid = float(np.median(np.arange(n_chr + 1) - bcce * (first - 1)))
    bracket = (mid - 0.5, mid + 0.5, bcce)
    fx["blk_pb2c"] = np.frombuffer(np.array(bracket, dtype=np.float64).tobytes(), dtype=np.uint8).copy()
    blocks = [b for b in range(1, nseg) if _find_chr(first, n_chr, b, bracket) != _find_chr(first, n_chr, b)]
    qs = []
    for i in range(N_PER_CLASS + 8):
        b = blocks[i % len(blocks)]
        c = _find_chr(first, n_chr, b)                          # (the chromosome that holds the block's residues)
        at = int(off[c]) + (b - int(first[c])) * blklen
        lo = max(int(off[c]), at - int(rng.integers(0, 150))); hi = min(int(off[c + 1]), at + blklen + int(rng.integers(0, 150)))
        f = mutate(rng, codes[lo:hi], 0.01)
        qs.append(f if i % 2 else revcomp(f))
    return dict(name="bracket", fx=fx, classes={"bracket": _class(qs, stops=EARLY)}, blocks=blocks, plain=with_prm(base["fx"]))


def all_indexes() -> list:
    return [long_index(), merge_index(), *grow_indexes(), *phases_indexes(), chromosomes_index(), bracket_index(), long_queries_index(),
            *protein_indexes(), wide_index()]


def entries_of(index: dict) -> list:
    """every entry of an index, class by class: [(class name, entry)]"""
    return [(c, e) for c, es in index["classes"].items() for e in es]


@functools.lru_cache(maxsize=None)
def _measured(name: str):
    index = next(ix for ix in all_indexes() if ix["name"] == name)
    return tuple((c, e, measure(index["fx"], e)) for c, e in entries_of(index))


def measured(index: dict) -> tuple:
    """the oracle on every entry of an index, computed once: ((class, entry, measure(..)), ...)"""
    return _measured(index["name"])
