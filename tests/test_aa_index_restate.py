"""The restatement of `spaln -W -KA` (tests/aa_index_restate.py) against the program's own files: the two databases of the protein
search fixtures (aa_db_a / _b.bka.gz, sequences in aa_search_a / _b.json.gz) and the builder's fixtures (aa_idx_edge / _wide,
tests/golden/make_aa_index_goldens.py).  Compared: every header field but the heap bytes the module's head lists, ChrID, Nblk, blkp,
blkb, wscr, the assigned ConvTab entries -- and the parameters the program chose from the database.  No GPU, nothing of the product."""
import numpy as np
import pytest

from tests import aa_fixture
from tests import aa_index_restate as air

SETS = ("a", "b", "edge", "wide")


@pytest.fixture(scope="module", params=SETS)
def case(request):
    name = request.param
    seqs = air.golden_db(name)
    want = air.parse(air.golden_bka(name))
    prm = air.default_params(seqs)
    return name, seqs, want, prm, air.build(seqs, prm)


def test_the_parameters_are_the_programs(case):
    name, seqs, want, prm, _ = case
    for k in ("nalpha", "ktuple", "nshift", "bitpat", "afact", "maxgene", "blklen"):
        assert prm[k] == want[k], (name, k, prm[k], want[k])
    assert prm["total"] == want["glen"] and want["tabsize"] == 20 ** prm["ktuple"] and want["nbitpat"] == 1


def test_the_index_is_the_programs(case):
    name, seqs, want, prm, got = case
    assert air.differences(got, want) == [], name
    # ContBlk::MaxBlk is only ever raised, from what the heap held: the file's number is at least the longest kept list
    assert want["maxblk"] >= got["maxblk"] == int(want["nblk"].max())


@pytest.mark.parametrize("name", aa_fixture.SETS)
def test_the_parser_agrees_with_the_search_fixtures_parser(name):
    mine, theirs = air.parse(air.golden_bka(name)), aa_fixture.parse_bka(name)
    for a, b in (("nblk", "blk_nblk"), ("blkp", "blk_blkp"), ("blkb", "blk_blkb"), ("wscr", "blk_wscr"), ("chrid", "blk_chr"), ("convtab", "blk_convtab")):
        assert np.array_equal(np.asarray(mine[a]).astype(np.int64), np.asarray(theirs[b]).astype(np.int64)), (name, a)
    assert (mine["nalpha"], mine["tabsize"], mine["nshift"], mine["chrno"], mine["maxblk"], mine["avrscr"], mine["blklen"]) == \
        tuple(int(theirs[k]) for k in ("nalpha", "tabsize", "nshift", "n_chr", "maxblk", "avrscr", "blklen"))


def test_what_the_edge_set_is_there_for():
    seqs = air.golden_db("edge")
    want = air.parse(air.golden_bka("edge"))
    assert want["ktuple"] == 3 and want["bytblk"] == 2 and want["blklen"] > 65536
    assert {1, 2, 3, 4} <= {len(s) for s in seqs} and any("U" in s for s in seqs) and any(set("BZOJ") <= set(s) for s in seqs)
    assert ((want["wscr"] >= 0) & (want["blkp"] == 0)).any()                     # a word that lost its list
    assert sum(1 for s in want["chrid"][2:-2:2] if s % 4096 == 0) >= 2            # sequence starts on tile boundaries
    wide = air.parse(air.golden_bka("wide"))
    assert wide["ktuple"] == 4 and wide["nshift"] == 4 and wide["bytblk"] == 4 and wide["chrno"] > 65535 and wide["glen"] >= 620000


def test_the_masked_bytes_are_the_only_ones_the_restatement_cannot_give():
    """the file put together from the restatement's arrays equals the program's outside the masked bytes"""
    import struct
    for name in ("a", "edge"):
        seqs = air.golden_db(name)
        raw = air.golden_bka(name)
        g = air.build(seqs, air.default_params(seqs))
        out = struct.pack("<8IhH", g["nalpha"], g["ktuple"], g["bitpat2"], g["tabsize"], g["bitpat"], g["nshift"], g["blklen"], g["maxgene"], 1, g["afact"])
        out += struct.pack("<II4Q4H5Q", g["convts"], 0, g["wordno"], g["wordsz"], g["chrno"], g["glen"], g["avrscr"], g["maxblk"], g["bytblk"], 26, 0, 0, 0, 0, 0)
        out += struct.pack("<3d", g["bclw"], g["bcup"], g["bcce"])
        out += g["chrid"].astype("<u4").tobytes() + g["nblk"].astype("<u2").tobytes() + g["blkp"].astype("<i4").tobytes()
        out += g["blkb"].astype("<u2" if g["bytblk"] == 2 else "<u4").tobytes() + g["wscr"].astype("<i2").tobytes() + g["convtab"].tobytes()
        assert len(out) == len(raw) and air.masked(out) == air.masked(raw), name
