"""Binding of the block search's vote (include/spdp.h, "block search") -- product path, device only.

`desc_from_arrays` fills SpdpBlkIndexDesc from the arrays a reference-side dump of an index holds (the layout the tests'
fixtures and the bench use: blk_prm, blk_nblk, ...); an integration fills the struct from its SrchBlk object instead
(INTEGRATION.md)."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np


class BlkIndexDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "nalpha", "tabsize", "nshift", "nbitpat", "convts", "n_chr", "maxblk", "kk", "drna", "maxmmc", "nseg",
        "minsigpr", "ncand", "nascr", "maxblock", "extblock", "extblockl", "shortquery", "hh_size", "hh_step", "hb_size", "hb_step",
        "ha_size", "ha_step", "gdb", "blklen")] + [
        ("rbscoef", C.c_float), ("rbscons", C.c_float),
        ("bclw", C.c_double), ("bcup", C.c_double), ("bcce", C.c_double), ("cfact", C.c_double),
        ("convtab", C.c_void_p), ("nblk", C.c_void_p), ("wscr", C.c_void_p), ("blkp", C.c_void_p),
        ("blkb", C.c_void_p), ("n_words", C.c_int64), ("rscrtab", C.c_void_p), ("chr", C.c_void_p),
        ("bitpat", C.c_void_p), ("n_bitpat", C.c_int32)]


# positions in the parameter record of a reference-side index dump (oracle/ref_build/blk_tap.cc, dump_index)
_PRM = dict(nalpha=0, tabsize=3, nshift=5, nbitpat=8, convts=10, n_chr=12, maxblk=14, kk=15, drna=16, maxmmc=17, nseg=19,
            minsigpr=22, ncand=23, nascr=24, maxblock=25, extblock=26, extblockl=27, shortquery=28, hh_size=29, hh_step=30, hb_size=31,
            hb_step=32, ha_size=33, ha_step=34, gdb=38, blklen=6)
REACHED, CUT, TABLE, FORCED = 1, 2, 4, 8


def desc_from_arrays(fx: dict):
    """(BlkIndexDesc, keep-alive list)"""
    prm = np.asarray(fx["blk_prm"], dtype=np.int32)
    d = BlkIndexDesc()
    for name, pos in _PRM.items():
        setattr(d, name, int(prm[pos]))
    d.rbscoef = struct.unpack("<f", struct.pack("<i", int(prm[36])))[0]
    d.rbscons = struct.unpack("<f", struct.pack("<i", int(prm[37])))[0]
    d.bclw, d.bcup, d.bcce = (float(x) for x in np.frombuffer(np.asarray(fx["blk_pb2c"], dtype=np.uint8).tobytes(), dtype=np.float64))
    d.cfact = float(np.frombuffer(np.asarray(fx["blk_cfact"], dtype=np.uint8).tobytes(), dtype=np.float64)[0])
    keep = []
    for field, key, dt in (("convtab", "blk_convtab", np.uint8), ("nblk", "blk_nblk", np.uint16), ("wscr", "blk_wscr", np.int16),
                           ("blkp", "blk_blkp", np.int32), ("blkb", "blk_blkb", np.uint32), ("rscrtab", "blk_rscrtab", np.int32),
                           ("chr", "blk_chr", np.int32), ("bitpat", "blk_bitpat", np.int32)):
        a = np.asarray(fx[key])
        a = np.ascontiguousarray(a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.astype(dt))
        keep.append(a)
        setattr(d, field, a.ctypes.data)
    d.n_words = int(keep[4].size)
    d.n_bitpat = int(keep[7].size)
    return d, keep


class BlockIndex:
    """an index resident on the engine's device"""

    def __init__(self, eng, fx: dict):
        self.eng, self.lib = eng, eng.lib
        self.lib.spdp_blk_index_create.restype = C.c_void_p
        self.lib.spdp_blk_index_create.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.spdp_blk_index_destroy.argtypes = [C.c_void_p]
        self.lib.spdp_blk_vote.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        self.lib.spdp_blk_vote_resident.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        self.lib.spdp_blk_vote_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        self.desc, self._keep = desc_from_arrays(fx)
        self.h = self.lib.spdp_blk_index_create(eng.ctx, C.byref(self.desc))
        if not self.h:
            raise RuntimeError("spdp_blk_index_create: " + self.lib.spdp_last_error(eng.ctx).decode())

    def free(self):
        if getattr(self, "h", None):
            self.lib.spdp_blk_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def vote(self, queries, ranges=None, stop_at=None, out_cap: int = 4096):
        """queries: list of uint8 code arrays; ranges: [(left, right)] (default whole query); stop_at: per query or None.
        Returns (records as an (n, out_cap) int32 array, kernel ms)."""
        n = len(queries)
        offs = np.zeros(n + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(q) for q in queries])
        codes = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.uint8) for q in queries]) if n else np.zeros(0, np.uint8))
        left = np.array([0 if ranges is None else ranges[i][0] for i in range(n)], dtype=np.int32)
        right = np.array([len(queries[i]) if ranges is None else ranges[i][1] for i in range(n)], dtype=np.int32)
        st = None if stop_at is None else np.ascontiguousarray(stop_at, dtype=np.int32)
        out = np.zeros((n, out_cap), dtype=np.int32)
        ms = C.c_float()
        rc = self.lib.spdp_blk_vote(self.eng.ctx, self.h, codes.ctypes.data, offs.ctypes.data, left.ctypes.data, right.ctypes.data,
                                    None if st is None else st.ctypes.data, n, out.ctypes.data, out_cap, C.byref(ms))
        self.eng._check(rc, "spdp_blk_vote")
        return out, ms.value

    def vote_resident(self, d_codes, d_offs, d_left, d_right, d_stop_at, n, d_out, out_cap):
        """device pointers in (ints), records written to d_out; returns kernel ms"""
        ms = C.c_float()
        rc = self.lib.spdp_blk_vote_resident(self.eng.ctx, self.h, d_codes, d_offs, d_left, d_right, d_stop_at, n, d_out, out_cap,
                                             C.byref(ms))
        self.eng._check(rc, "spdp_blk_vote_resident")
        return ms.value

    def vote_stats(self) -> dict:
        return vote_stats(self)


def vote_stats(index: "BlockIndex") -> dict:
    """spdp_blk_vote_stats: which paths the vote kernel took on this index since it was created (abi.BLK_VOTE_STATS)"""
    from . import abi
    v = (C.c_int64 * len(abi.BLK_VOTE_STATS))()
    index.eng._check(index.lib.spdp_blk_vote_stats(index.eng.ctx, index.h, v, len(abi.BLK_VOTE_STATS)), "spdp_blk_vote_stats")
    return dict(zip(abi.BLK_VOTE_STATS, (int(x) for x in v)))


def split_record(rec: np.ndarray):
    """one query's record -> dict (see include/spdp.h, spdp_blk_vote)"""
    n, calls, flags = int(rec[0]), int(rec[1]), int(rec[2])
    if not flags & REACHED or flags & CUT:
        return dict(reached=bool(flags & REACHED), calls=calls, flags=flags)
    r = rec[:n]
    j = 3
    head = r[j:j + 20].copy(); j += 20
    qb = []
    for _ in range(4):
        k = int(r[j]); qb.append(r[j + 1:j + 1 + 2 * k].reshape(k, 2).copy()); j += 1 + 2 * k
    npairs = int(r[j]); pairs = r[j + 1:j + 1 + 9 * npairs].reshape(npairs, 9).copy(); j += 1 + 9 * npairs
    nruns = int(r[j]); runs = r[j + 1:j + 1 + 2 * nruns].reshape(nruns, 2).copy(); j += 1 + 2 * nruns
    assert j == n, (j, n)
    by_d = [[] for _ in range(4)]
    for code, scr in runs:
        by_d[int(code) >> 28].append((int(code) & 0xfffffff, int(scr)))
    return dict(reached=True, calls=calls, flags=flags, head=head, qb=qb, pairs=pairs, runs=[sorted(x) for x in by_d])


class SearchOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("max_out", "max_mmc", "min_sigpr", "nascr", "ext_block", "max_intron_len", "local",
                                          "genomic_db")] + [("rbs_fact", C.c_float), ("rbs_base", C.c_float), ("cfact", C.c_double)]


def read_index_file(lib, path: str, **opts):
    """the reference's <db>.bkn read by the library (host only): dict with the same keys a reference-side dump has
    (blk_prm positions filled where the library knows them), for comparison and for BlockIndex"""
    lib.spdp_blk_index_read.restype = C.c_void_p
    lib.spdp_blk_index_read.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.spdp_blk_index_host_desc.restype = C.POINTER(BlkIndexDesc)
    lib.spdp_blk_index_host_desc.argtypes = [C.c_void_p]
    lib.spdp_blk_index_host_free.argtypes = [C.c_void_p]
    o = SearchOpts()
    lib.spdp_blk_search_opts_default(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    err = C.create_string_buffer(256)
    h = lib.spdp_blk_index_read(path.encode(), C.byref(o), err, 256)
    if not h:
        raise RuntimeError(err.value.decode())
    out = _host_index_to_dict(lib, h)
    lib.spdp_blk_index_host_free(h)
    return out


def _host_index_to_dict(lib, h) -> dict:
    """a SpdpBlkIndexHost -> the arrays in the layout of a reference-side dump (BlockIndex, the tests' oracle)"""
    lib.spdp_blk_index_host_desc.restype = C.POINTER(BlkIndexDesc)
    lib.spdp_blk_index_host_desc.argtypes = [C.c_void_p]
    d = lib.spdp_blk_index_host_desc(h).contents

    def arr(ptr, n, dt):
        if not n:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt).copy()
    out = {name: int(getattr(d, name)) for name, _ in BlkIndexDesc._fields_[:26]}
    out.update(rbscoef=float(d.rbscoef), rbscons=float(d.rbscons), bclw=d.bclw, bcup=d.bcup, bcce=d.bcce, cfact=d.cfact,
               blk_convtab=arr(d.convtab, d.convts, np.uint8), blk_nblk=arr(d.nblk, d.tabsize, np.uint16),
               blk_wscr=arr(d.wscr, d.tabsize, np.int16), blk_blkp=arr(d.blkp, d.tabsize, np.int32),
               blk_blkb=arr(d.blkb, d.n_words, np.uint32), blk_rscrtab=arr(d.rscrtab, 128, np.int32),
               blk_chr=arr(d.chr, 2 * (d.n_chr + 1), np.int32), blk_bitpat=arr(d.bitpat, d.n_bitpat, np.int32))
    prm = np.zeros(42, dtype=np.int32)
    for name, pos in _PRM.items():
        prm[pos] = out[name]
    prm[36] = struct.unpack("<i", struct.pack("<f", out["rbscoef"]))[0]
    prm[37] = struct.unpack("<i", struct.pack("<f", out["rbscons"]))[0]
    out["blk_prm"] = prm
    out["blk_pb2c"] = np.frombuffer(np.array([out["bclw"], out["bcup"], out["bcce"]], dtype=np.float64).tobytes(), dtype=np.uint8).copy()
    out["blk_cfact"] = np.frombuffer(np.array([out["cfact"]], dtype=np.float64).tobytes(), dtype=np.uint8).copy()
    return out


def read_protein_db_index(lib, path: str, max_out: int = 1, local: int = 0, cross_species: bool = True):
    """<db>.bka of `spaln -W -KA` read for SrchBlk::finds: (the arrays as read_index_file gives them, for BlockIndex;
    abi.BlkFindsParams as spdp_blk_finds_params_default fills it).  The index serves this max_out only (Ncand = max_out + 10)."""
    from . import abi, defaults
    lib.spdp_blk_index_read.restype = C.c_void_p
    lib.spdp_blk_index_read.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.spdp_blk_index_host_free.argtypes = [C.c_void_p]
    lib.spdp_blk_finds_params_default.restype = C.c_int
    lib.spdp_blk_finds_params_default.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    o = SearchOpts()
    lib.spdp_blk_search_opts_default(C.byref(o))
    for k, v in defaults.search_opts_protein_db(max_out, local, cross_species).items():
        setattr(o, k, v)
    err = C.create_string_buffer(256)
    h = lib.spdp_blk_index_read(path.encode(), C.byref(o), err, 256)
    if not h:
        raise RuntimeError(err.value.decode())
    try:
        prm = abi.BlkFindsParams()
        if lib.spdp_blk_finds_params_default(h, int(max_out), int(local), C.byref(prm)):
            raise RuntimeError("spdp_blk_finds_params_default: the index holds no average word score")
        out = _host_index_to_dict(lib, h)
    finally:
        lib.spdp_blk_index_host_free(h)
    return out, prm


SHORT = 16                               # SPDP_BLK_SHORT


def finds(index: "BlockIndex", prm, queries, ranges=None, out_cap: int = 64, resident: bool = False):
    """spdp_blk_finds (resident: spdp_blk_finds_resident on device arrays made here): the vote of SrchBlk::finds for protein
    queries (uint8 code arrays) against the index of a protein database; prm: abi.BlkFindsParams.
    Returns (records as an (n, out_cap) int32 array -- see split_finds_record --, kernel ms)."""
    eng, lib, n = index.eng, index.lib, len(queries)
    codes, offs = _packed(queries)
    left = np.array([0 if ranges is None else ranges[i][0] for i in range(n)], dtype=np.int32)
    right = np.array([len(queries[i]) if ranges is None else ranges[i][1] for i in range(n)], dtype=np.int32)
    out = np.zeros((n, out_cap), dtype=np.int32)
    ms = C.c_float()
    name = "spdp_blk_finds_resident" if resident else _entry(index, "spdp_blk_finds")
    fn = getattr(lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 8 + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    if not resident:
        rc = fn(eng.ctx, index.h, C.byref(index.desc), C.byref(prm), codes.ctypes.data, offs.ctypes.data, left.ctypes.data, right.ctypes.data, n,
                out.ctypes.data, out_cap, C.byref(ms))
        eng._check(rc, name)
        return out, ms.value
    hip = _hip_runtime()
    hosts = (codes, offs, left, right, out)
    bufs = [C.c_void_p() for _ in hosts]
    try:
        for b, a in zip(bufs, hosts):
            if hip.hipMalloc(C.byref(b), C.c_size_t(max(a.nbytes, 16))):
                raise RuntimeError("hipMalloc failed")
            if a.nbytes and hip.hipMemcpy(b, a.ctypes.data, C.c_size_t(a.nbytes), 1):
                raise RuntimeError("hipMemcpy failed")
        rc = fn(eng.ctx, index.h, C.byref(index.desc), C.byref(prm), bufs[0], bufs[1], bufs[2], bufs[3], n, bufs[4], out_cap, C.byref(ms))
        eng._check(rc, "spdp_blk_finds_resident")
        if out.nbytes and hip.hipMemcpy(out.ctypes.data, bufs[4], C.c_size_t(out.nbytes), 2):
            raise RuntimeError("hipMemcpy failed")
    finally:
        for b in bufs:
            if b:
                hip.hipFree(b)
    return out, ms.value


FINDS_STATS = ("searched", "refused_short", "candidates", "dropped_by_threshold", "vote_us", "align_us", "host_us")


def finds_stats(eng) -> dict:
    """spdp_blk_finds_stats: the counters of the last map_align_b call on this engine"""
    v = (C.c_int64 * len(FINDS_STATS))()
    eng.lib.spdp_blk_finds_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    eng.lib.spdp_blk_finds_stats(eng.ctx, v, len(FINDS_STATS))
    return dict(zip(FINDS_STATS, (int(x) for x in v)))


def finds_store_stats(eng) -> dict:
    """spdp_blk_finds_store_stats: what held the scores in the last finds() call on this engine -- form (0 slab, 1 table), waves,
    area_bytes of one wave, first_slots / last_slots of a table, launches, rerun_queries after a full table, most_blocks a query
    scored (table form)"""
    from . import abi
    v = (C.c_int64 * len(abi.BLK_FINDS_STORE_STATS))()
    eng.lib.spdp_blk_finds_store_stats.restype = C.c_int
    eng.lib.spdp_blk_finds_store_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    if eng.lib.spdp_blk_finds_store_stats(eng.ctx, v, len(v)):
        raise RuntimeError("spdp_blk_finds_store_stats: null argument")
    return dict(zip(abi.BLK_FINDS_STORE_STATS, (int(x) for x in v)))


def map_align_b(index: "BlockIndex", db_codes, seq_off, sc, up, sp, fprm, queries, all_out: bool = False):
    """spdp_map_align_b: what `spaln -Q4 .. -Q7 -a<db> [-M N] [-pw]` prints of protein queries against a protein database -- the
    vote of finds, every candidate aligned (spdp_align_b_seeded with sp.qck = 1 .. 3, spdp_align_b with 0), the threshold sp.vthr
    unless all_out, the hits ordered by fstat.val, at most fprm.max_out.  db_codes / seq_off: the database sequences in the
    index's order; sp: abi.SeedParams with its model set (defaults.seed_params_b + wilip_model_b); fprm: abi.BlkFindsParams.
    Returns (per query a list of dicts seq, a_rng, b_rng, score, val, mch, mmc, gap, unp, corners (k, 2) int32; seconds [vote,
    alignment, host, call])."""
    from . import abi
    eng, lib, n = index.eng, index.lib, len(queries)
    codes, offs = _packed(queries)
    dc = np.ascontiguousarray(db_codes, dtype=np.uint8)
    do = np.ascontiguousarray(seq_off, dtype=np.int64)
    g = Genome(dc.ctypes.data, do.ctypes.data, len(do) - 1)
    hit_off = np.zeros(n + 1, dtype=np.int64)
    hits, corners = C.POINTER(abi.MapHitB)(), C.POINTER(C.c_int32)()
    sec = (C.c_double * 4)()
    name = _entry(index, "spdp_map_align_b")
    fn = getattr(lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 10 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4
    rc = fn(eng.ctx, index.h, C.byref(index.desc), C.byref(g), C.byref(sc), C.byref(up), C.byref(sp), C.byref(fprm),
            codes.ctypes.data, offs.ctypes.data, n, int(bool(all_out)), hit_off.ctypes.data, C.byref(hits), C.byref(corners), sec)
    if rc < 0:
        eng._check(rc, name)
    out = []
    for i in range(n):
        lst = []
        for k in range(int(hit_off[i]), int(hit_off[i + 1])):
            h = hits[k]
            c = np.array([[corners[2 * (h.corner_off + j)], corners[2 * (h.corner_off + j) + 1]] for j in range(h.n_corners)], dtype=np.int32).reshape(-1, 2)
            lst.append(dict(seq=h.seq, a_rng=(h.a_left, h.a_right), b_rng=(h.b_left, h.b_right), score=h.score, val=h.val, mch=h.mch, mmc=h.mmc,
                            gap=h.gap, unp=h.unp, corners=c))
        out.append(lst)
    _free(hits, corners)
    return out, list(sec)


def split_finds_record(rec: np.ndarray) -> dict:
    """one query's record of spdp_blk_finds -> dict(flags, nmmc, testword, sigm, heap = [(block, score)] in hsort order,
    cands = the candidate sequences in the order finds fills sqs[1..]); a refused or cut record: its flags alone"""
    n, nmmc, flags = int(rec[0]), int(rec[1]), int(rec[2])
    if flags & SHORT or flags & CUT or not flags & REACHED:
        return dict(flags=flags, nmmc=nmmc)
    sigm = int(rec[5])
    heap = [(int(rec[6 + 2 * i]), int(rec[7 + 2 * i])) for i in range(sigm)]
    j = 6 + 2 * sigm
    nc = int(rec[j])
    cands = [int(x) for x in rec[j + 1:j + 1 + nc]]
    assert j + 1 + nc == n, (j, nc, n)
    return dict(flags=flags, nmmc=nmmc, testword=[int(rec[3]), int(rec[4])], sigm=sigm, heap=heap, cands=cands)


class BlkBuildParams(C.Structure):       # SpdpBlkBuildParams
    _fields_ = [("ktuple", C.c_int32), ("nshift", C.c_int32), ("blklen", C.c_int32), ("maxgene", C.c_int32), ("nbitpat", C.c_int32),
                ("afact", C.c_int32), ("bitpat", C.c_uint32), ("bitpat2", C.c_uint32), ("threaded", C.c_int32)]


def build_params_default(lib, fasta_bytes: int, nbitpat: int = 1, threaded: int = 0) -> BlkBuildParams:
    """what `spaln -W -KD [-XC<n>]` picks for a FASTA file of that size (spdp_blk_build_params_default)"""
    p = BlkBuildParams()
    lib.spdp_blk_build_params_default.argtypes = [C.c_int64, C.c_int32, C.c_void_p]
    if lib.spdp_blk_build_params_default(int(fasta_bytes), int(nbitpat), C.byref(p)):
        raise RuntimeError("spdp_blk_build_params_default: out of range")
    p.threaded = threaded
    return p


def build_index(eng, genome_codes, chr_off, prm: BlkBuildParams, write_to: str = None, **opts):
    """spdp_blk_index_build (+ spdp_blk_index_write): the block index of a genome made on the device.  Returns (the arrays in
    the layout read_index_file gives, seconds [device, host, call])."""
    lib = eng.lib
    g = Genome()
    gc = np.ascontiguousarray(genome_codes, dtype=np.uint8)
    go = np.ascontiguousarray(chr_off, dtype=np.int64)
    g.codes, g.chr_off, g.n_chr = gc.ctypes.data, go.ctypes.data, len(go) - 1
    o = SearchOpts()
    lib.spdp_blk_search_opts_default(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    sec = (C.c_double * 3)()
    lib.spdp_blk_index_build.restype = C.c_void_p
    lib.spdp_blk_index_build.argtypes = [C.c_void_p] * 5
    lib.spdp_blk_index_host_free.argtypes = [C.c_void_p]
    h = lib.spdp_blk_index_build(eng.ctx, C.byref(g), C.byref(prm), C.byref(o), sec)
    if not h:
        raise RuntimeError(lib.spdp_last_error(eng.ctx).decode())
    try:
        if write_to is not None:
            lib.spdp_blk_index_write.argtypes = [C.c_void_p, C.c_char_p]
            if lib.spdp_blk_index_write(h, write_to.encode()):
                raise RuntimeError("spdp_blk_index_write: cannot write " + write_to)
        out = _host_index_to_dict(lib, h)
    finally:
        lib.spdp_blk_index_host_free(h)
    return out, list(sec)


class BlkBuildParamsP(C.Structure):      # SpdpBlkBuildParamsP
    _fields_ = [("b", BlkBuildParams), ("nalpha", C.c_int32), ("minorf", C.c_int32), ("aaafact", C.c_double), ("acomp", C.c_double * 20),
                ("convts", C.c_int32), ("convtab", C.c_uint8 * 32)]


def build_params_default_p(lib, fasta_bytes: int, threaded: int = 0, acomp=None) -> BlkBuildParamsP:
    """what `spaln -W -KP` picks for a FASTA file of that size (spdp_blk_build_params_default_p); acomp: MakeBlk::prepacomp's terms,
    by default those of the reference's default tables (defaults.BLOCK_ACOMP_20)"""
    from . import defaults
    p = BlkBuildParamsP()
    for i, v in enumerate(defaults.BLOCK_ACOMP_20 if acomp is None else acomp):
        p.acomp[i] = float(v)
    lib.spdp_blk_build_params_default_p.argtypes = [C.c_int64, C.c_void_p]
    if lib.spdp_blk_build_params_default_p(int(fasta_bytes), C.byref(p)):
        raise RuntimeError("spdp_blk_build_params_default_p: out of range")
    p.b.threaded = threaded
    return p


def build_index_p(eng, genome_codes, chr_off, prm: BlkBuildParamsP, write_to: str = None, **opts):
    """spdp_blk_index_build_p (+ spdp_blk_index_write): the translated block index (`spaln -W -KP`, <db>.bkp) made on the device.
    Returns (the arrays in the layout read_index_file gives, seconds [device, host, call])."""
    lib = eng.lib
    g = Genome()
    gc = np.ascontiguousarray(genome_codes, dtype=np.uint8)
    go = np.ascontiguousarray(chr_off, dtype=np.int64)
    g.codes, g.chr_off, g.n_chr = gc.ctypes.data, go.ctypes.data, len(go) - 1
    o = SearchOpts()
    lib.spdp_blk_search_opts_default(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    sec = (C.c_double * 3)()
    lib.spdp_blk_index_build_p.restype = C.c_void_p
    lib.spdp_blk_index_build_p.argtypes = [C.c_void_p] * 5
    lib.spdp_blk_index_host_free.argtypes = [C.c_void_p]
    h = lib.spdp_blk_index_build_p(eng.ctx, C.byref(g), C.byref(prm), C.byref(o), sec)
    if not h:
        raise RuntimeError(lib.spdp_last_error(eng.ctx).decode())
    try:
        if write_to is not None:
            lib.spdp_blk_index_write.argtypes = [C.c_void_p, C.c_char_p]
            if lib.spdp_blk_index_write(h, write_to.encode()):
                raise RuntimeError("spdp_blk_index_write: cannot write " + write_to)
        out = _host_index_to_dict(lib, h)
    finally:
        lib.spdp_blk_index_host_free(h)
    return out, list(sec)


class BlkBuildParamsA(C.Structure):      # SpdpBlkBuildParamsA
    _fields_ = [("b", BlkBuildParams), ("nalpha", C.c_int32), ("convts", C.c_int32), ("convtab", C.c_uint8 * 32)]


def build_params_default_a(lib, total_residues: int) -> BlkBuildParamsA:
    """what `spaln -W -KA` picks for a protein database of that many counted residues, and the ConvTab it writes
    (spdp_blk_build_params_default_a)"""
    p = BlkBuildParamsA()
    lib.spdp_blk_build_params_default_a.argtypes = [C.c_int64, C.c_void_p]
    if lib.spdp_blk_build_params_default_a(int(total_residues), C.byref(p)):
        raise RuntimeError("spdp_blk_build_params_default_a: out of range")
    return p


def build_index_a(eng, codes, offs, prm: BlkBuildParamsA, write_to: str = None, max_out: int = 1, local: int = 0, cross_species: bool = True):
    """spdp_blk_index_build_a (+ spdp_blk_index_write): the amino-acid index of a protein database (`spaln -W -KA`, <db>.bka) made on
    the device; codes / offs: the database as map_align_b takes it.  Returns what read_protein_db_index returns of the program's file
    (the arrays for BlockIndex, abi.BlkFindsParams -- None when the index has no average word score) and the seconds [device, host,
    call]."""
    from . import abi, defaults
    lib = eng.lib
    g = Genome()
    gc = np.ascontiguousarray(codes, dtype=np.uint8)
    go = np.ascontiguousarray(offs, dtype=np.int64)
    g.codes, g.chr_off, g.n_chr = gc.ctypes.data, go.ctypes.data, len(go) - 1
    o = SearchOpts()
    lib.spdp_blk_search_opts_default(C.byref(o))
    for k, v in defaults.search_opts_protein_db(max_out, local, cross_species).items():
        setattr(o, k, v)
    sec = (C.c_double * 3)()
    lib.spdp_blk_index_build_a.restype = C.c_void_p
    lib.spdp_blk_index_build_a.argtypes = [C.c_void_p] * 5
    lib.spdp_blk_index_host_free.argtypes = [C.c_void_p]
    lib.spdp_blk_finds_params_default.restype = C.c_int
    lib.spdp_blk_finds_params_default.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    h = lib.spdp_blk_index_build_a(eng.ctx, C.byref(g), C.byref(prm), C.byref(o), sec)
    if not h:
        raise RuntimeError(lib.spdp_last_error(eng.ctx).decode())
    try:
        if write_to is not None:
            lib.spdp_blk_index_write.argtypes = [C.c_void_p, C.c_char_p]
            if lib.spdp_blk_index_write(h, write_to.encode()):
                raise RuntimeError("spdp_blk_index_write: cannot write " + write_to)
        fprm = abi.BlkFindsParams()
        if lib.spdp_blk_finds_params_default(h, int(max_out), int(local), C.byref(fprm)):
            fprm = None                                 # (no word kept its list -- a database of one sequence: nothing to search with)
        out = _host_index_to_dict(lib, h)
    finally:
        lib.spdp_blk_index_host_free(h)
    return out, fprm, list(sec)


def bka_without_heap_bytes(raw: bytes) -> bytes:
    """a <db>.bka with the bytes zeroed in which the program's files hold its heap, to compare a built file with the program's: the
    five pointers of ContBlk, the padding behind ConvTS, ContBlk::MaxBlk (only ever raised, from what the heap held) and the ConvTab
    entries ReducWord never assigns (0, 1, 2 and 23)"""
    b = bytearray(raw)
    convts = struct.unpack_from("<I", raw, 36)[0]
    for lo, hi in ((36 + 48, 36 + 88), (40, 44), (36 + 42, 36 + 44)):
        b[lo:hi] = bytes(hi - lo)
    for i in (0, 1, 2, 23):
        if i < convts:
            b[len(b) - convts + i] = 0
    return bytes(b)


class BlkFindParams(C.Structure):        # SpdpBlkFindParams
    _fields_ = [("vthr", C.c_int32), ("drop_rate", C.c_float), ("max_out", C.c_int32), ("max_out2", C.c_int32),
                ("min_agap", C.c_int32), ("phase1t", C.c_int32), ("a_exgl", C.c_int32), ("a_exgr", C.c_int32)]


class Genome(C.Structure):               # SpdpGenome
    _fields_ = [("codes", C.c_void_p), ("chr_off", C.c_void_p), ("n_chr", C.c_int32)]


class Locus(C.Structure):                # SpdpLocus
    _fields_ = [(k, C.c_int32) for k in ("query", "chr", "rvs", "base", "len", "left", "right", "jscr", "n_hsp")] + [("hsp_off", C.c_int64)]


def find_params_from_fixture(fx) -> BlkFindParams:
    """find_prm of a blk_* fixture (oracle/ref_build/blk_tap.cc, dump_find_prm)"""
    v = np.asarray(fx["find_prm"], dtype=np.int32)
    p = BlkFindParams()
    p.vthr = int(v[0])
    p.drop_rate = float(v[1:2].view(np.float32)[0])
    p.max_out, p.max_out2, p.min_agap, p.phase1t = int(v[4]), int(v[5]), int(v[7]), int(v[11])
    p.a_exgl, p.a_exgr = int(v[20]), int(v[21])
    return p


class MapExon(C.Structure):
    _fields_ = [("q_left", C.c_int32), ("q_right", C.c_int32), ("g_left", C.c_int32), ("g_right", C.c_int32)]


class MapGene(C.Structure):
    _fields_ = [("chr", C.c_int32), ("rvs", C.c_int32), ("q_rev", C.c_int32), ("score", C.c_int32), ("val", C.c_int32), ("n_loci", C.c_int32),
                ("n_exons", C.c_int32), ("exon_off", C.c_int64)]


def _packed(queries, lead: int = 0):
    """the queries one behind the other, `lead` bytes in front of the first: (codes, offs)"""
    n = len(queries)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[0] = lead
    offs[1:] = lead + np.cumsum([len(q) for q in queries], dtype=np.int64)
    codes = np.zeros(int(offs[n]), dtype=np.uint8)
    if n:
        codes[lead:] = np.concatenate([np.asarray(q, dtype=np.uint8) for q in queries])
    return codes, offs


def _gene(G, exons):
    ex = [(exons[G.exon_off + j].q_left, exons[G.exon_off + j].q_right, exons[G.exon_off + j].g_left, exons[G.exon_off + j].g_right)
          for j in range(G.n_exons)]
    return dict(chr=G.chr, rvs=G.rvs, q_rev=G.q_rev, score=G.score, val=G.val, n_loci=G.n_loci, exons=ex)


def _free(*ptrs):
    """what an entry malloc'ed for its caller"""
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for p in ptrs:
        libc.free(p)


class _Call:
    """One call of an entry that searches the genome for a batch of queries.  Every such entry begins (ctx, index, its description,
    genome, `models` ..., codes, offs, ...): this holds the packed queries, the Genome and the arrays they point into while the
    call runs and its outputs are read.  run() sets the entry's types from the arguments it is given -- a Python int is an int32, a
    numpy array its data, everything else a pointer -- and raises on a negative return code."""

    def __init__(self, index: "BlockIndex", genome_codes, chr_off, queries, *models):
        self.lib, self.eng, self.n = index.lib, index.eng, len(queries)
        self.codes, self.offs = _packed(queries)
        self._gc = np.ascontiguousarray(genome_codes, dtype=np.uint8)
        self._go = np.ascontiguousarray(chr_off, dtype=np.int64)
        self.g = Genome(self._gc.ctypes.data, self._go.ctypes.data, len(self._go) - 1)
        self.sec = (C.c_double * 4)()
        self._head = (C.c_void_p(index.eng.ctx), C.c_void_p(index.h), C.byref(index.desc), C.byref(self.g)) + models + (self.codes, self.offs)
        self._index = index

    def run(self, fn: str, *rest) -> int:
        fn = _entry(self._index, fn)
        args = [C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in self._head + rest]
        f = getattr(self.lib, fn)
        f.restype = C.c_int
        f.argtypes = [C.c_int32 if isinstance(a, int) else C.c_void_p for a in args]
        rc = f(*args)
        if rc < 0:
            self.eng._check(rc, fn)
        return rc

    def best(self, fn: str, *middle, tails=()):
        """an entry that reports one gene per query: (per query None or its dict, seconds, return code)"""
        genes = (MapGene * max(self.n, 1))()
        exons = C.POINTER(MapExon)()
        rc = self.run(fn, self.n, *middle, genes, C.byref(exons), self.sec, *tails)
        out = [None if genes[i].chr < 0 else _gene(genes[i], exons) for i in range(self.n)]
        _free(exons)
        return out, list(self.sec), rc

    def lists(self, fn: str, *middle, more=(), tails=()):
        """an entry that reports a list of genes per query (more: further outputs behind the three every such entry has):
        (per query the list of its dicts, in the entry's order; seconds; return code)"""
        gene_off = np.zeros(self.n + 1, dtype=np.int64)
        genes, exons = C.POINTER(MapGene)(), C.POINTER(MapExon)()
        rc = self.run(fn, self.n, *middle, gene_off, C.byref(genes), C.byref(exons), *more, self.sec, *tails)
        out = [[_gene(genes[k], exons) for k in range(int(gene_off[i]), int(gene_off[i + 1]))] for i in range(self.n)]
        _free(genes, exons)
        return out, list(self.sec), rc


def _rp_s(rescore):
    """map_align's (codonk1, minl, jneibr, lsg) as the cDNA entries take it"""
    from . import abi
    return abi.RescoreParams(*(int(x) for x in rescore))


def _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, rp, queries) -> _Call:
    """the arguments every map + align entry begins with"""
    return _Call(index, genome_codes, chr_off, queries, C.byref(sc), C.byref(sp), C.c_void_p(C.addressof(sigmodel)), C.byref(prm), C.byref(rp))


def find(index: "BlockIndex", genome_codes, chr_off, model, sc, prm: BlkFindParams, queries, ranges=None):
    """spdp_blk_find: the block search of every query up to its candidate loci.  Returns (per query a list of dicts
    {chr, rvs, base, len, left, right, jscr, hsps (n + 1, 5)}, status array)."""
    call = _Call(index, genome_codes, chr_off, queries, C.c_void_p(C.addressof(model)), C.byref(sc), C.byref(prm))
    n = call.n
    left = np.array([0 if ranges is None else ranges[i][0] for i in range(n)], dtype=np.int32)
    right = np.array([len(queries[i]) if ranges is None else ranges[i][1] for i in range(n)], dtype=np.int32)
    loci = C.POINTER(Locus)()
    hsps = C.POINTER(C.c_int32)()
    nl = C.c_int32()
    status = np.zeros(n, dtype=np.int32)
    name = _entry(index, "spdp_blk_find")
    call.eng._check(call.run(name, left, right, n, C.byref(loci), C.byref(nl), C.byref(hsps), status), name)
    out = [[] for _ in range(n)]
    for k in range(nl.value):
        L = loci[k]
        h = np.array([[hsps[5 * (L.hsp_off + j) + c] for c in range(5)] for j in range(L.n_hsp + 1)], dtype=np.int32)
        out[L.query].append(dict(chr=L.chr, rvs=L.rvs, base=L.base, len=L.len, left=L.left, right=L.right, jscr=L.jscr, hsps=h))
    _free(loci, hsps)
    return out, status


def find_stats(eng) -> dict:
    """spdp_blk_find_stats: who served the HSP searches of the last find / map_align call on this engine"""
    v = (C.c_int64 * len(FIND_STATS))()
    eng.lib.spdp_blk_find_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    eng.lib.spdp_blk_find_stats(eng.ctx, v, len(FIND_STATS))
    return dict(zip(FIND_STATS, (int(x) for x in v)))


FIND_STATS = ("tasks", "device", "too_long", "too_many", "retries", "batches")


# ---- the HSP search by itself (include/spdp.h: spdp_hsp_plan, spdp_hsp_tasks, spdp_hsp_tasks_host) -- for tests and tools
HSP_TOO_LONG, HSP_TOO_MANY = 1, 2
HSP_FIELDS = ("jx", "jy", "jlen", "nid", "jscr", "diagonal", "first")


class HspPlan(C.Structure):              # SpdpHspPlan
    _fields_ = [(k, C.c_int32) for k in ("hash_slots", "hit_cap", "seg_cap", "out_cap", "n_waves", "lds_bytes", "waves_per_cu", "reserved")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_[:7]}


class HspTask(C.Structure):              # SpdpHspTask
    _fields_ = [(k, C.c_int32) for k in ("query", "chr", "base", "len", "rvs")]


class HspRequest(C.Structure):           # SpdpHspRequest
    _fields_ = [("model", C.c_void_p), ("genome", C.c_void_p), ("codes", C.c_void_p), ("offs", C.c_void_p), ("left", C.c_void_p),
                ("right", C.c_void_p), ("tlen", C.c_void_p), ("n_queries", C.c_int32), ("tasks", C.c_void_p), ("n_tasks", C.c_int32),
                ("a_exgl", C.c_int32), ("a_exgr", C.c_int32)]


def hsp_plan(lib, longest: int, mtx_rows: int, mtx_cols: int, n_tasks: int = 1, n_cu: int = 0, **want) -> dict:
    """spdp_hsp_plan: the LDS plan spdp_blk_find picks for a batch whose longest query range is `longest` (want: fields given
    explicitly; 0 or absent = the product's choice).  Host code.  Raises RuntimeError with the refusal's text."""
    w, out = HspPlan(**{k: int(v) for k, v in want.items()}), HspPlan()
    err = C.create_string_buffer(256)
    lib.spdp_hsp_plan.restype = C.c_int
    lib.spdp_hsp_plan.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_char_p, C.c_int32]
    if lib.spdp_hsp_plan(C.byref(w), int(longest), int(mtx_rows), int(mtx_cols), int(n_tasks), int(n_cu), C.byref(out), err, 256):
        raise RuntimeError(err.value.decode())
    return out.as_dict()


class _HspCall:
    """the arrays a SpdpHspRequest points into, kept while the call runs.  tasks: (query, chr, base, len, rvs) each"""

    def __init__(self, model, genome_codes, chr_off, queries, tasks, ranges=None, tlen=None, exg=(0, 0)):
        n = len(queries)
        self.codes, self.offs = _packed(queries)
        self.left = np.array([0 if ranges is None else ranges[i][0] for i in range(n)], dtype=np.int32)
        self.right = np.array([len(queries[i]) if ranges is None else ranges[i][1] for i in range(n)], dtype=np.int32)
        self.tlen = None if tlen is None else np.ascontiguousarray(tlen, dtype=np.int32)
        self._gc = np.ascontiguousarray(genome_codes, dtype=np.uint8)
        self._go = np.ascontiguousarray(chr_off, dtype=np.int64)
        self.g = Genome(self._gc.ctypes.data, self._go.ctypes.data, len(self._go) - 1)
        self.tasks = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 5))
        self.n_tasks = self.tasks.shape[0]
        self.model = model
        self.rq = HspRequest(C.addressof(model), C.addressof(self.g), self.codes.ctypes.data, self.offs.ctypes.data, self.left.ctypes.data,
                             self.right.ctypes.data, None if self.tlen is None else self.tlen.ctypes.data, n, self.tasks.ctypes.data,
                             self.n_tasks, int(exg[0]), int(exg[1]))
        self.rec_off = np.zeros(self.n_tasks + 1, dtype=np.int64)
        self.recs = C.POINTER(C.c_int32)()

    def records(self):
        """per task its (k, 7) int32 records; frees what the entry handed out"""
        tot = int(self.rec_off[-1])
        flat = np.ctypeslib.as_array(self.recs, shape=(7 * tot,)).copy().reshape(tot, 7) if tot else np.zeros((0, 7), dtype=np.int32)
        _free(self.recs)
        return [flat[int(self.rec_off[k]):int(self.rec_off[k + 1])] for k in range(self.n_tasks)]


def hsp_tasks_host(lib, model, genome_codes, chr_off, queries, tasks, ranges=None, tlen=None, exg=(0, 0)):
    """spdp_hsp_tasks_host: the tasks through the host form of the search (level -1), no device.  Returns (per task its records as a
    (k, 7) int32 array of HSP_FIELDS in scan order, counts as an (n_tasks, 3) int32 array of shared words, seed segments, records)."""
    c = _HspCall(model, genome_codes, chr_off, queries, tasks, ranges, tlen, exg)
    counts = np.zeros((c.n_tasks, 3), dtype=np.int32)
    err = C.create_string_buffer(256)
    lib.spdp_hsp_tasks_host.restype = C.c_int
    lib.spdp_hsp_tasks_host.argtypes = [C.c_void_p] * 4 + [C.c_char_p, C.c_int32]
    if lib.spdp_hsp_tasks_host(C.byref(c.rq), counts.ctypes.data, c.rec_off.ctypes.data, C.byref(c.recs), err, 256):
        raise RuntimeError(err.value.decode())
    return c.records(), counts


def hsp_tasks(eng, model, genome_codes, chr_off, queries, tasks, ranges=None, tlen=None, exg=(0, 0), **want):
    """spdp_hsp_tasks: the tasks through the device search under a plan (want: hash_slots, hit_cap, seg_cap, out_cap, n_waves; 0 or
    absent = what find would choose).  Returns (per task its records as hsp_tasks_host gives them -- none for a flagged task --,
    flags as an int32 array, the plan as launched)."""
    c = _HspCall(model, genome_codes, chr_off, queries, tasks, ranges, tlen, exg)
    w, used = HspPlan(**{k: int(v) for k, v in want.items()}), HspPlan()
    flags = np.zeros(max(c.n_tasks, 1), dtype=np.int32)
    eng.lib.spdp_hsp_tasks.restype = C.c_int
    eng.lib.spdp_hsp_tasks.argtypes = [C.c_void_p] * 7
    eng._check(eng.lib.spdp_hsp_tasks(eng.ctx, C.byref(c.rq), C.byref(w), C.byref(used), flags.ctypes.data, c.rec_off.ctypes.data,
                                      C.byref(c.recs)), "spdp_hsp_tasks")
    return c.records(), flags[:c.n_tasks], used.as_dict()


def map_align(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries, ori: int = 1):
    """spdp_map_align_s: block search -> loci -> signals -> seeded alignment -> rescoring, one call for all queries.
    rescore = (codonk1, minl, jneibr, lsg).  Returns (per query None or dict(chr, rvs, score, val, n_loci,
    exons = [(q_left, q_right, g_left, g_right)]), seconds [find, regions + signals, align, rescore], return code)."""
    return _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, _rp_s(rescore), queries).best("spdp_map_align_s", int(ori))


def map_align_h(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries):
    """spdp_map_align_h: the same for protein queries against the translated index.  sc: abi.ScoringH; rescore = abi.RescoreParamsH;
    Returns as map_align."""
    return _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, rescore, queries).best("spdp_map_align_h")


def map_align_multi(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries, ori: int = 1,
                    all_out: bool = False):
    """spdp_map_align_s_multi: what `spaln -M N` prints of every query -- up to prm.max_out loci, highest fstat.val first, the
    threshold sp.vthr applied unless all_out (-pw); a locus printed though the threshold dropped it has score abi.NEVSEL.  The
    index must have been made for prm.max_out (ncand = max_out + 10).  ori = 3: every locus picks its orientation on its own; the
    program aligns a query's further loci with the query left reverse-complemented after a locus that took that orientation, so
    such a query's later loci can differ from spaln's (include/spdp.h).
    Returns (per query a list of dicts shaped as map_align's, in print order; seconds; return code)."""
    c = _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, _rp_s(rescore), queries)
    return c.lists("spdp_map_align_s_multi", int(ori), int(bool(all_out)))


def map_align_h_multi(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries,
                      all_out: bool = False):
    """spdp_map_align_h_multi: the same for protein queries against the translated index (arguments as map_align_h's)"""
    return _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, rescore, queries).lists("spdp_map_align_h_multi", int(bool(all_out)))


# ---- query preparation (include/spdp.h "query preparation"): poly-A tails, poly-T heads, the orientation of a cDNA query
class QueryPrep(C.Structure):            # SpdpQueryPrep
    _fields_ = [("q_mns", C.c_int32), ("polya_thr", C.c_int32)]


class QueryTail(C.Structure):            # SpdpQueryTail
    _fields_ = [(k, C.c_int32) for k in ("pol", "tlen", "left", "right", "ori")] + [("reserved", C.c_int32 * 3)]


TAIL_FIELDS = ("pol", "tlen", "left", "right", "ori")


def _tail_records(tails, n):
    return np.array([[getattr(tails[i], k) for k in TAIL_FIELDS] for i in range(n)], dtype=np.int32).reshape(n, len(TAIL_FIELDS))


def _tails_out(tails, codes_out, offs, n):
    return _tail_records(tails, n), [codes_out[int(offs[i]):int(offs[i + 1])].copy() for i in range(n)]


def _hip_runtime():
    """the HIP runtime this process has loaded with the library (not a second one)"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            hip = C.CDLL(ln.split()[-1])
            hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            return hip
    raise RuntimeError("the HIP runtime is not loaded: create an Engine first")


def polya_scan_host(lib, queries, q_mns: int = 3, polya_thr: int = 12, lead: int = 0):
    """spdp_polya_scan_host: PolyA::rmpolyA in its sequential form, no device.  Returns (records as an (n, 5) int32 array of
    pol, tlen, left, right, ori; the normalised queries)."""
    n = len(queries)
    codes, offs = _packed(queries, lead)
    prep = QueryPrep(int(q_mns), int(polya_thr))
    tails = (QueryTail * max(n, 1))()
    out = np.full(codes.size, 255, dtype=np.uint8)
    lib.spdp_polya_scan_host.restype = C.c_int
    lib.spdp_polya_scan_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    if lib.spdp_polya_scan_host(codes.ctypes.data, offs.ctypes.data, n, C.byref(prep), tails, out.ctypes.data):
        raise RuntimeError("spdp_polya_scan_host: refused (q_mns must be 1 or 3)")
    return _tails_out(tails, out, offs, n)


def polya_scan(eng, queries, q_mns: int = 3, polya_thr: int = 12, lead: int = 0, resident: bool = False):
    """spdp_polya_scan (resident: spdp_polya_scan_resident on device arrays made here): the device form.
    Returns (records, the normalised queries, kernel ms)."""
    lib = eng.lib
    n = len(queries)
    codes, offs = _packed(queries, lead)
    prep = QueryPrep(int(q_mns), int(polya_thr))
    ms = C.c_float()
    if not resident:
        tails = (QueryTail * max(n, 1))()
        out = np.full(codes.size, 255, dtype=np.uint8)
        lib.spdp_polya_scan.restype = C.c_int
        lib.spdp_polya_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = lib.spdp_polya_scan(eng.ctx, codes.ctypes.data, offs.ctypes.data, n, C.byref(prep), tails, out.ctypes.data, C.byref(ms))
        eng._check(rc, "spdp_polya_scan")
        return _tails_out(tails, out, offs, n) + (ms.value,)
    # device arrays of the caller's own, through the HIP runtime the library is linked with
    hip = _hip_runtime()
    bufs = [C.c_void_p() for _ in range(3)]
    sizes = (max(codes.size, 16), offs.size * 8, max(n, 1) * C.sizeof(QueryTail))
    try:
        for b, sz in zip(bufs, sizes):
            if hip.hipMalloc(C.byref(b), C.c_size_t(sz)):
                raise RuntimeError("hipMalloc failed")
        if hip.hipMemcpy(bufs[0], codes.ctypes.data, C.c_size_t(codes.size), 1) or hip.hipMemcpy(bufs[1], offs.ctypes.data, C.c_size_t(offs.size * 8), 1):
            raise RuntimeError("hipMemcpy failed")
        lib.spdp_polya_scan_resident.restype = C.c_int
        lib.spdp_polya_scan_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = lib.spdp_polya_scan_resident(eng.ctx, bufs[0], bufs[1], n, C.byref(prep), bufs[2], C.byref(ms))
        eng._check(rc, "spdp_polya_scan_resident")
        out = np.zeros(codes.size, dtype=np.uint8)
        tails = (QueryTail * max(n, 1))()
        if (codes.size and hip.hipMemcpy(out.ctypes.data, bufs[0], C.c_size_t(codes.size), 2)) or hip.hipMemcpy(tails, bufs[2], C.c_size_t(sizes[2]), 2):
            raise RuntimeError("hipMemcpy failed")
    finally:
        for b in bufs:
            if b:
                hip.hipFree(b)
    return _tails_out(tails, out, offs, n) + (ms.value,)


def map_align_prep(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries, q_mns: int = 3,
                   polya_thr: int = 12):
    """spdp_map_align_s_prep: map_align with PolyA::rmpolyA in front -- what `spaln -Q7` does to queries as a FASTA file holds
    them.  Returns (genes as map_align's, seconds, return code, records as polya_scan's)."""
    c = _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, _rp_s(rescore), queries)
    prep, tails = QueryPrep(int(q_mns), int(polya_thr)), (QueryTail * max(c.n, 1))()
    return c.best("spdp_map_align_s_prep", C.byref(prep), tails=(tails,)) + (_tail_records(tails, c.n),)


def map_align_multi_prep(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries,
                         q_mns: int = 3, polya_thr: int = 12, all_out: bool = False):
    """spdp_map_align_s_multi_prep: map_align_multi with PolyA::rmpolyA in front.  Returns (lists as map_align_multi's, seconds,
    return code, records as polya_scan's)."""
    c = _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, _rp_s(rescore), queries)
    prep, tails = QueryPrep(int(q_mns), int(polya_thr)), (QueryTail * max(c.n, 1))()
    return c.lists("spdp_map_align_s_multi_prep", C.byref(prep), int(bool(all_out)), tails=(tails,)) + (_tail_records(tails, c.n),)


# ---- dispersed loci (include/spdp.h "dispersed loci"): what `spaln -pr` prints of a query whose parts lie in different places
def _dispersed(c: _Call, fn: str, *middle, tails=()):
    """a _dispersed entry: its lists with every gene's part, the covered ranges, seconds, return code"""
    part = C.POINTER(C.c_int32)()
    covered = np.zeros(2 * max(c.n, 1), dtype=np.int32)
    out, sec, rc = c.lists(fn, *middle, more=(C.byref(part), covered), tails=tails)
    for k, g in enumerate(g for lst in out for g in lst):       # (the genes lie in the lists' order)
        g["part"] = int(part[k])
    _free(part)
    return out, covered[:2 * c.n].reshape(c.n, 2), sec, rc


def map_align_dispersed(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries, min_seg_len: int,
                        ori: int = 1, prep=None):
    """spdp_map_align_s_dispersed: per query the locus of its first search and of the searches on what that left uncovered on
    each side (at most three, in the program's print order).  min_seg_len: the program's MinSegLen = 2 Ktuple + Nshift of the
    index; prm.max_out must be 1.  prep = (q_mns, polya_thr): PolyA::rmpolyA in front, as map_align_prep (it replaces ori).
    Returns (per query a list of dicts shaped as map_align's plus part = 0 / 1 / 2: first search / left rest / right rest;
    covered: (n, 2) int32, the range every query has after its first search; seconds; return code; records as polya_scan's or None)."""
    c = _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, _rp_s(rescore), queries)
    qp = C.byref(QueryPrep(int(prep[0]), int(prep[1]))) if prep is not None else None
    tails = (QueryTail * max(c.n, 1))() if prep is not None else None
    res = _dispersed(c, "spdp_map_align_s_dispersed", int(ori), qp, int(min_seg_len), tails=(tails,))
    return res + (_tail_records(tails, c.n) if prep is not None else None,)


def map_align_h_dispersed(index: "BlockIndex", genome_codes, chr_off, sc, sp, sigmodel, prm: BlkFindParams, rescore, queries, min_seg_len: int):
    """spdp_map_align_h_dispersed: the same for protein queries against the translated index (arguments as map_align_h's; positions
    of the query in residues).  Returns (lists, covered, seconds, return code) as map_align_dispersed."""
    c = _map_call(index, genome_codes, chr_off, sc, sp, sigmodel, prm, rescore, queries)
    return _dispersed(c, "spdp_map_align_h_dispersed", int(min_seg_len))


# ---- device groups (include/spdp.h "device groups, third part"): the entries above on an engine.Group --------------------------
GROUP_TWINS = ("spdp_blk_finds", "spdp_map_align_b", "spdp_blk_find", "spdp_map_align_s_prep", "spdp_map_align_s_multi_prep",
               "spdp_map_align_s_dispersed", "spdp_map_align_h_dispersed")


class _GroupHandle:
    """what a call needs of an engine when a group runs it: the handle the entry takes first, and the group's error text"""

    def __init__(self, grp):
        self.grp, self.lib, self.ctx = grp, grp.lib, grp.h

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.grp.last_error()}")


class GroupIndex:
    """One BlockIndex per member of an engine.Group, all made from the same arrays (a fixture, read_index_file /
    read_protein_db_index of a file, or what build_index* returned), and the handle array the group entries take.  Where a
    function of this module takes an index, a GroupIndex makes it run its group twin (group_finds, group_map_align_b, ...)."""

    def __init__(self, grp, fx: dict):
        self.grp, self.lib = grp, grp.lib
        self.members = []
        try:
            for r in range(grp.size):
                self.members.append(BlockIndex(grp.context(r), fx))
        except Exception:
            self.free()
            raise
        self._handles = (C.c_void_p * grp.size)(*[m.h for m in self.members])
        self.h = C.addressof(self._handles)
        self.desc = self.members[0].desc
        self.eng = _GroupHandle(grp)

    def free(self):
        for m in self.members:
            m.free()
        self.members = []


def _entry(index, name: str) -> str:
    """the entry that serves this index: the single-context one, or its group twin for a GroupIndex"""
    if not isinstance(index, GroupIndex) or name.startswith("spdp_group_"):
        return name
    if name not in GROUP_TWINS:
        raise ValueError(f"{name} has no group form that goes through a GroupIndex")
    return "spdp_group_" + name[len("spdp_"):]


def _grouped(index) -> "GroupIndex":
    if not isinstance(index, GroupIndex):
        raise TypeError("a blocks.GroupIndex is needed (one index per member of the group)")
    return index


def group_finds(index: GroupIndex, prm, queries, ranges=None, out_cap: int = 64):
    """spdp_group_blk_finds: finds() with the queries sharded over the group's members; kernel ms = the slowest member's"""
    return finds(_grouped(index), prm, queries, ranges, out_cap)


def group_map_align_b(index: GroupIndex, db_codes, seq_off, sc, up, sp, fprm, queries, all_out: bool = False):
    """spdp_group_map_align_b: map_align_b() on a group; seconds [vote, alignment, host: each the slowest member's; the group call]"""
    return map_align_b(_grouped(index), db_codes, seq_off, sc, up, sp, fprm, queries, all_out)


def group_find(index: GroupIndex, genome_codes, chr_off, model, sc, prm: BlkFindParams, queries, ranges=None):
    """spdp_group_blk_find: find() on a group (nucleotide queries, or protein queries on translated indexes)"""
    return find(_grouped(index), genome_codes, chr_off, model, sc, prm, queries, ranges)


def group_map_align_prep(index: GroupIndex, *args, **kw):
    """spdp_group_map_align_s_prep: map_align_prep() on a group"""
    return map_align_prep(_grouped(index), *args, **kw)


def group_map_align_multi_prep(index: GroupIndex, *args, **kw):
    """spdp_group_map_align_s_multi_prep: map_align_multi_prep() on a group"""
    return map_align_multi_prep(_grouped(index), *args, **kw)


def group_map_align_dispersed(index: GroupIndex, *args, **kw):
    """spdp_group_map_align_s_dispersed: map_align_dispersed() on a group"""
    return map_align_dispersed(_grouped(index), *args, **kw)


def group_map_align_h_dispersed(index: GroupIndex, *args, **kw):
    """spdp_group_map_align_h_dispersed: map_align_h_dispersed() on a group"""
    return map_align_h_dispersed(_grouped(index), *args, **kw)
