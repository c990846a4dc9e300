"""The fixtures of the protein database search (tests/golden/aa_db_<set>.bka.gz, aa_search_<set>.json.gz; made by
tests/golden/make_aa_search_goldens.py from the program's own runs) as the tests read them.  The index file is parsed HERE, in plain
numpy from the layout `spaln -W -KA` writes (format version 26: BlkWcPrm, ContBlk, Block2Chr, ChrID, Nblk, blkp, blkb, wscr,
ConvTab -- src/blksrc.cc:1697-1858), not by the library's reader, so that the restatement stands on nothing of the product."""
import functools
import gzip
import json
import os
import struct

import numpy as np

from tests import finds_restate as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = ("a", "b")
AA = "ARNDCQEGHILKMFPSTWYV"


def encode(s: str) -> np.ndarray:
    """the reference's amino-acid codes: A = 3 .. V = 22 in its own order, X (AMB) = 2"""
    return np.array([2 if c == "X" else AA.index(c) + 3 for c in s], dtype=np.uint8)


def bka_path(name: str, tmp_dir: str) -> str:
    """the set's index file unpacked into tmp_dir (the library's reader takes a path)"""
    out = os.path.join(tmp_dir, f"aa_db_{name}.bka")
    if not os.path.exists(out):
        with gzip.open(os.path.join(GOLDEN, f"aa_db_{name}.bka.gz"), "rb") as f, open(out, "wb") as g:
            g.write(f.read())
    return out


@functools.lru_cache(maxsize=None)
def parse_bka(name: str) -> dict:
    raw = gzip.open(os.path.join(GOLDEN, f"aa_db_{name}.bka.gz"), "rb").read()
    nalpha, ktuple, bitpat2, tabsize, bitpat, nshift, blklen, maxgene, nbitpat, afact = struct.unpack_from("<8IhH", raw, 0)
    convts, _, wordno, wordsz, chrno, glen, avrscr, maxblk, bytblk, verno = struct.unpack_from("<II4Q4H", raw, 36)
    bclw, bcup, bcce = struct.unpack_from("<3d", raw, 36 + 88)
    assert verno == 26 and nbitpat == 1 and bytblk in (2, 4), (verno, nbitpat, bytblk)
    at = 36 + 88 + 24
    chrid = np.frombuffer(raw, dtype="<u4", count=2 * (chrno + 1), offset=at); at += 8 * (chrno + 1)
    nblk = np.frombuffer(raw, dtype="<u2", count=tabsize, offset=at); at += 2 * tabsize
    blkp = np.frombuffer(raw, dtype="<i4", count=tabsize, offset=at); at += 4 * tabsize
    blkb = np.frombuffer(raw, dtype="<u4" if bytblk == 4 else "<u2", count=wordno, offset=at).astype(np.uint32); at += bytblk * wordno
    wscr = np.frombuffer(raw, dtype="<i2", count=tabsize, offset=at); at += 2 * tabsize
    convtab = np.frombuffer(raw, dtype=np.uint8, count=convts, offset=at); at += convts
    assert at == len(raw), (at, len(raw))
    if ktuple == bitpat:
        bitpat = (1 << bitpat) - 1
    ex = [w for w in range(32) if bitpat >> w & 1]
    width = max(ex) + 1
    return dict(nalpha=nalpha, tabsize=tabsize, nshift=nshift, nbitpat=nbitpat, n_chr=chrno, maxblk=maxblk, kk=1, avrscr=avrscr,
                nseg=int(chrid[2 * chrno + 1]), blklen=blklen, bclw=bclw, bcup=bcup, bcce=bcce, cfact=0.75,
                blk_convtab=convtab, blk_nblk=nblk, blk_wscr=wscr, blk_blkp=blkp, blk_blkb=blkb, blk_chr=chrid.astype(np.int64),
                blk_bitpat=np.array([len(ex), width, 2 * (len(ex) - 1)] + ex + [width - 1 - e for e in reversed(ex)], dtype=np.int32))


def index(name: str, max_out: int, local: int = 0) -> fr.Index:
    """SrchBlk after initialize with the program's default constants for a protein database (algmode.crs set: RbsFactSqrX, RbsBaseX)"""
    fx = parse_bka(name)
    return fr.index_from_arrays(fx, fx["avrscr"], max_out=max_out, local=local, rbs_fact=0.0, rbs_base=0.5)


@functools.lru_cache(maxsize=None)
def search(name: str) -> dict:
    return json.loads(gzip.open(os.path.join(GOLDEN, f"aa_search_{name}.json.gz"), "rb").read())


# the runs whose records show the whole candidate set (-pw prints every candidate): key -> (MaxOut, local)
PW_RUNS = {"M4_pw": (4, 0), "LS_M2_pw": (2, 1)}
