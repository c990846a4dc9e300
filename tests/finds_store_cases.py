"""What tests/test_finds_hash_host.py (the CPU) and tests/test_gpu_finds_store.py (the device) share about the second form of the
finds vote's score store, the open-addressed table: which recipes of tests/finds_cases.py hold a query that scores more than 64
distinct blocks -- a first table of 64 slots runs full there and the query is run again --, and a malformed index with blocks
twice in one posting list."""
from __future__ import annotations

import numpy as np

from tests import finds_cases as fc

# the most blocks one query scores, per recipe, as the host run counts them (tests/test_finds_hash_host.py holds the table to it)
MOST_BLOCKS = {
    "phase_ns3": 73, "edge_ns3": 10, "phase_ns2": 75, "edge_ns2": 10, "endings": 95, "ambiguous": 80, "ubiquitous": 96,
    "lists_63": 83, "lists_64": 82, "lists_65": 86, "lists_128": 139, "lists_129": 141, "family_m1": 91, "family_m4": 93,
    "ties_m1": 74, "ties_m2": 74, "ties_m4": 74, "tiny_sequences": 57, "not_local": 66, "local": 70, "geometry_ns1": 99,
    "geometry_ns4": 105, "geometry_bp3": 118, "geometry_bp5": 120, "geometry_bp5_ns2": 120, "geometry_bighash": 106,
    "zeros_bp1": 108, "zeros_bp5": 104, "cut": 52,
}
SMALL = 64                                      # SPDP_FINDS_RSCR_SLOTS of the forced growth: the smallest first table
OVER_SMALL = [name for name, n in MOST_BLOCKS.items() if n > SMALL]
MUST_OVERFLOW = ("family_m4", "geometry_bp5", "geometry_bp5_ns2", "zeros_bp5")


def twice_in_a_list(name: str = "lists_129") -> dict:
    """a recipe's index with every fifth posting entry repeating the one before it: a block twice in one list, often in one chunk
    of 64 (the lists stay ascending and inside nseg; what the vote makes of it is not the restatement's to say)"""
    fx = dict(fc.recipes()[name]["fx"])
    blkb = np.array(fx["blk_blkb"], copy=True)
    at = np.arange(1, blkb.size, 5)
    blkb[at] = blkb[at - 1]
    fx["blk_blkb"] = blkb
    return fx
