"""tests/rescore_cases.py and the oracle's two rescoring walks, without a GPU: the oracle accepts every generated case, every
recipe has the effect it is named for (read off the oracle's output), and the set as a whole holds the numbers of accepted and
rejected intron candidates, planted ties, frame-shift records and end-gap flag sets that tests/test_gpu_rescore.py relies on.

Edit records: the properties tests/test_gpu_rescore.py holds spdp_skl_edits_s to are first tried here on the reference's own
rng_cigar_* / rng_vulgar_* arrays of the cDNA fixtures whose four end-gap flags are 0.  Four properties one would expect do not
hold for the reference's own records and are therefore not held against the kernel: Cigar's M + I = query span and M + D + N =
genomic span, Vulgar's sum of alen = query span and sum of blen = genomic span.  The reference writes a query gap at the end of
the list twice (s1_exg_0000 -A0: + 3), and a genomic gap behind an intron candidate that is still open at the end of the list
with the candidate's length taken off (s1_exg_0000 -A2: D -248, s1_subrange_global -A2: D -598).  The protein walk shares that handling
of a list's end, so its span sums are not held either.  Its records are tried on the h1_* / c1_* fixtures: the N lengths and the
5 / I / 3 triples are the gaps behind the intron records, the split-codon records S come as a pair around a triple, there is one
F per frame-shift row.  Dropped there: "an intron of phase -1 / 1 carries the S pair, one of phase 0 none" -- the reference
writes S by what the last frame shift left in `phs`, not by the junction's phase (h1_basic: phases 0, 1, 1, no S record)."""
import collections

import numpy as np
import pytest

from tests import rescore_cases as rc, spdg
from tests.conftest import golden_files

F = rc.F


def _exons(recs):
    """the records before the end marker"""
    assert recs[-1][F["left"]] == recs[-1][F["right"]] == 2 ** 31 - 1
    return recs[:-1]


@pytest.mark.parametrize("walk", ["s", "h"])
def test_oracle_takes_every_case(walk):
    """nothing raises, nothing is skipped: the generator is what keeps to the walks' domain"""
    got = rc.expected(walk)
    assert len(got) == sum(c.corners is not None for c in rc.cases(walk)) >= 90
    for c in rc.cases(walk):
        if c.corners is None:
            continue
        pts = c.corners
        assert all(b[0] >= a[0] and b[1] >= a[1] for a, b in zip(pts, pts[1:])), c.name
        assert c.rng[0] <= pts[0][0] and pts[-1][0] <= c.rng[1] and c.rng[2] <= pts[0][1] and pts[-1][1] <= c.rng[3], c.name
        score, fst, recs = got[c.name]
        assert score > rc.NEVSEL and len(_exons(recs)) >= 1


def test_sizes():
    for c in rc.cases("s"):
        assert 30 <= c.rng[1] - c.rng[0] <= 300 or c.recipe == "aligner", c.name
        assert c.arrays["b"].size <= 3000, c.name
    for c in rc.cases("h"):
        assert 15 <= c.arrays["a"].size <= 80, c.name
        assert c.arrays["b"].size <= (12001 if c.recipe == "h_window" else 3001), c.name
    assert {c.kw["jneibr"] for c in rc.cases("s")} == {c.kw["jneibr"] for c in rc.cases("h")} == set(rc.JNEIBR)


def test_condensed_lists_equal_full_ones():
    for walk in ("s", "h"):
        got = rc.expected(walk)
        n = 0
        for c in rc.cases(walk):
            twin = c.info.get("twin")
            if twin and twin != c.name:
                assert len(c.corners) < len(next(x for x in rc.cases(walk) if x.name == twin).corners), c.name
                assert got[c.name] == got[twin], c.name
                n += 1
        assert n >= 12


def test_cdna_recipes():
    got = rc.expected("s")
    seen = collections.Counter()
    for c in rc.cases("s"):
        if c.corners is None:
            continue
        score, fst, recs = got[c.name]
        ex = _exons(recs)
        if "records" in c.info:
            assert len(recs) == c.info["records"], c.name
        if c.recipe == "bound":
            assert len(recs) == len(c.corners) > len(c.corners) // 2 + 3 or len(c.corners) < 6, c.name     # beyond the slot of old
            seen["bound_beyond_old_slot"] += len(recs) > len(c.corners) // 2 + 3
        if c.recipe.startswith("tie"):
            name, pos = c.info["tie"]
            at = c.info["accepted_at"]
            lo = rc.oracle_of(c.variant(name, pos, at - 1))
            hi = rc.oracle_of(c.variant(name, pos, at))
            assert lo != hi, c.name                             # the planted value sits on the comparison's edge
            assert got[c.name] == (hi if at == 0 else lo), c.name
            if c.recipe == "tie_x":
                assert len(ex) == 2 and ex[0][F["iscr"]] == c.info["iscr"], c.name
                assert len(_exons(lo[2])) == 1, c.name
            elif c.recipe == "tie_gap":
                assert len(ex) == 1 and len(_exons(hi[2])) == 2, c.name
            else:
                k2 = c.info["path"][1][1]
                assert ex[0][F["right"]] == _exons(hi[2])[0][F["right"]] - k2, c.name    # the first candidate stays
            seen[c.recipe] += 1
        if c.recipe == "two_del":
            assert len(ex) == 2 and ex[0][F["right"]] + c.info["path"][2][1] == ex[1][F["left"]], c.name      # preint before the intron
        if c.recipe == "codonk1":
            assert fst[2] == 2 and fst[3] == 2 * c.info["gap"], c.name
        if c.recipe == "jneibr":
            jn, L, k = c.kw["jneibr"], c.info["exon_len"], c.info["exon"]
            assert ex[k][F["right"]] - ex[k][F["left"]] == L, c.name
            assert ex[k][F["mch"]] + ex[k][F["mmc"]] == L, c.name
            # an exon shorter than the neighbourhood: its 5' counts are the exon's own (`psp < jn`)
            if L < jn and k < 2:
                assert ex[k][F["mch5"]] + ex[k][F["mmc5"]] == L, c.name
            seen[("jn", jn, L - jn)] += 1
        if c.recipe == "end_gaps":
            seen[("exg", c.exg)] += 1
        seen["accepted"] += len(ex) - 1
        seen["rejected"] += c.info["candidates"] - (len(ex) - 1)
    assert seen["accepted"] >= 40 and seen["rejected"] >= 40, seen
    assert min(seen["tie_x"], seen["tie_gap"], seen["tie_iscr"]) >= 10
    assert sum(1 for k in seen if isinstance(k, tuple) and k[0] == "exg") == 16
    assert seen["bound_beyond_old_slot"] >= 3
    for jn in rc.JNEIBR:
        assert seen[("jn", jn, 0)] and seen[("jn", jn, 1)] and (jn == 1 or seen[("jn", jn, -1)])


def test_end_gaps_are_free_where_the_flag_says_so():
    """the same list under all-zero flags and under its own: the score differs exactly when a flag frees a gap that is there"""
    import dataclasses
    got = rc.expected("s")
    n_diff = 0
    for c in rc.cases("s"):
        if c.recipe != "end_gaps":
            continue
        v = int(c.name.split("_")[1])
        base = rc.oracle_of(dataclasses.replace(c, exg=(0, 0, 0, 0)))
        flush = v in (0, 2) and any(c.exg[i] for i in ((0, 1) if v == 0 else (2, 3))) and not (v == 2 and c.exg[2] and not c.exg[3])
        if v in (1, 3):
            assert got[c.name][0] == base[0], c.name               # one position inside the range: never free
        elif flush:
            assert got[c.name][0] > base[0], c.name
            n_diff += 1
    assert n_diff >= 12


def test_protein_recipes():
    got = rc.expected("h")
    seen = collections.Counter()
    for c in rc.cases("h"):
        if c.corners is None:
            continue
        score, fst, recs = got[c.name]
        ex = _exons(recs)
        fs = [r for r in ex[:-1] if r[F["iscr"]] == rc.NEVSEL]
        introns = [r for r in ex[:-1] if r[F["iscr"]] != rc.NEVSEL]
        if c.recipe == "h_forms":
            assert len(introns) == c.info["introns"] and not fs, c.name
        if c.recipe == "h_jneibr":
            jn, L, k = c.kw["jneibr"], c.info["exon_len"], c.info["exon"]
            assert len(recs) == 4 and ex[k][F["right"]] - ex[k][F["left"]] == 3 * L and ex[k][F["mch"]] + ex[k][F["mmc"]] == L, c.name
            own = ex[k][F["mch5"]] + ex[k][F["mmc5"]] == L and ex[k][F["mch"]] == ex[k][F["mch5"]]
            if (k < 2 and 3 * L < jn) or (k == 2 and 3 * L <= jn):       # inside the neighbourhood: the 5' counts are the exon's own
                assert own, c.name
            seen[("jn", jn, "own" if own else "ring")] += 1
        if c.recipe == "h_codonk1":
            import dataclasses
            short = rc.oracle_of(dataclasses.replace(c, kw=dict(jneibr=c.kw["jneibr"])))      # codonk1 `never`: every gap short
            assert (got[c.name] != short) == (c.info["gap"] > 21), c.name
            seen[("codonk1", c.info["gap"], c.exg[0])] += 1
        if c.recipe == "h_suptcodon":
            import dataclasses
            off = rc.oracle_of(dataclasses.replace(c, kw=dict(c.kw, sup_tcodon=0)))
            assert ex[-1][F["right"]] == c.info["right"] and _exons(off[2])[-1][F["right"]] == c.info["right"] + 3, c.name
            seen["suptcodon"] += 1
        if c.recipe == "h_split":
            assert len(fs) == 1 and len(introns) == 1 and introns[0][F["phs"]] == 0, c.name
            seen["split"] += 1
        if c.recipe == "h_minl":
            assert len(introns) == c.info["introns"], c.name
            seen[("minl", c.info["introns"])] += 1
        if c.recipe == "h_frameshift":
            # told apart in the records: an insertion frame shift ends phs positions before the next record begins (RIGHT = n - phs),
            # a deletion frame shift phs positions behind it (RIGHT = n + phs)
            d = [ex[j + 1][F["left"]] - r[F["right"]] for j, r in enumerate(ex[:-1]) if r[F["iscr"]] == rc.NEVSEL]
            assert all(x in (-2, -1, 1, 2) for x in d) and not introns, c.name
            assert (sum(x > 0 for x in d), sum(x < 0 for x in d)) == (c.info["ins_fs"], c.info["del_fs"]), c.name
            seen["ins_fs"] += sum(x > 0 for x in d)
            seen["del_fs"] += sum(x < 0 for x in d)
        if c.recipe == "h_junction":
            kind, ph = c.info["kind"], c.info["phase"]
            assert len(introns) == (kind != "reject"), (c.name, kind)
            if introns:
                assert introns[0][F["phs"]] == ph, c.name
                seen[("phs", ph)] += 1
            if kind == "tie":
                name, pos = c.info["tie"]
                lo = rc.oracle_of(c.variant(name, pos, -1))
                assert [r for r in _exons(lo[2])[:-1] if r[F["iscr"]] != rc.NEVSEL] == [], c.name
                seen["tie"] += 1
            seen["accepted" if introns else "rejected"] += 1
        elif c.recipe != "h_frameshift":
            seen["accepted"] += len(introns)
        if c.recipe in ("h_codes", "h_edge"):
            if c.recipe == "h_edge" and c.info["side"] == 0:
                # the exon in front of the intron is empty and gets no record; the intron shows in where the only exon begins
                assert not introns and ex[-1][F["left"]] == c.corners[1][1] - 1 and ex[-1][F["phs"]] == 1, c.name
            else:
                assert len(introns) == 1 and introns[0][F["phs"]] == c.info["phase"], c.name
            seen[c.recipe] += 1
        if c.recipe == "h_end_gaps":
            import dataclasses
            base = rc.oracle_of(dataclasses.replace(c, exg=(0, 0, 0, 0)))
            assert (score != base[0]) == bool(c.exg[0] or c.exg[1]), c.name        # a_exgl prices the first gap as unpaired, a_exgr the last
            seen[("exg", c.exg)] += 1
        if c.recipe == "h_bonus":
            assert ex[0][F["sig3"]] == c.info["sig3"] and ex[-1][F["sig5"]] == c.info["sig5"], c.name
            seen[("bonus", c.info["on"])] += 1
        if c.recipe == "h_back_to_back":
            assert len(recs) == (3 if c.info["width"] <= 1 else 4), c.name
            seen[("width", c.info["width"])] += 1
        if c.recipe == "h_window":
            lo, hi = c.corners[0][1], c.corners[-1][1]
            b_len = c.arrays["b"].size - 1
            if c.info["deep"]:
                assert lo - c.info["margin"] > 0 and hi + c.info["margin"] < b_len + 3, c.name
            else:
                assert lo - c.info["margin"] < 0 and hi + c.info["margin"] > b_len + 3, c.name
            seen[("window", c.info["deep"])] += 1
    assert seen["accepted"] >= 40 and seen["rejected"] >= 40, seen
    assert seen["tie"] >= 10 and seen["ins_fs"] >= 20 and seen["del_fs"] >= 20, seen
    assert all(seen[("phs", ph)] >= 4 for ph in (-1, 0, 1)), seen
    assert seen["h_codes"] >= 12 and seen["h_edge"] >= 6 and sum(1 for k in seen if isinstance(k, tuple) and k[0] == "exg") == 16
    assert seen[("bonus", 0)] >= 4 and seen[("bonus", 1)] >= 4
    assert all(seen[("codonk1", g, e)] for g in (21, 24) for e in (0, 1))
    assert all(seen[("jn", jn, "ring")] for jn in rc.JNEIBR) and all(seen[("jn", jn, "own")] for jn in (10, 32))
    assert seen["split"] >= 8 and seen["suptcodon"] >= 6
    assert seen[("minl", 0)] >= 3 and seen[("minl", 1)] >= 3
    assert seen[("width", 1)] >= 4 and seen[("window", True)] >= 4 and seen[("window", False)] >= 4


# ---- the edit-record properties, on the reference's own records ---------------------------------------------------------------------
def cigar_properties(cig, exons):
    """Cigar records (op, len) of a cDNA list whose end-gap flags are 0: the N lengths, in order, are the gaps between the exon records"""
    assert [int(n) for op, n in cig if chr(op) == "N"] == [b[F["left"]] - a[F["right"]] for a, b in zip(exons, exons[1:])]


def vulgar_properties(vul, exons):
    """Vulgar records (op, alen, blen): every intron as 5 / I / 3 with 2 + (len - 4) + 2, in the exon records' order"""
    vul = [(chr(o), int(a), int(b)) for o, a, b in vul]
    lens = []
    for k, (o, a, b) in enumerate(vul):
        if o == "I":
            assert vul[k - 1] == ("5", 0, 2) and vul[k + 1] == ("3", 0, 2) and a == 0
            lens.append(b + 4)
    assert lens == [b[F["left"]] - a[F["right"]] for a, b in zip(exons, exons[1:])]
    assert sum(o in "53" for o, _, _ in vul) == 2 * len(lens)


def test_edit_properties_hold_for_the_reference():
    n = 0
    for f in golden_files() + golden_files("c2_"):
        fx = spdg.load(f)
        q = fx["prm"]
        if q["a_exgl"] or q["a_exgr"] or q["b_exgl"] or q["b_exgr"] or q["local"]:
            continue
        for alg in (0, 2):
            if f"rng_cigar_A{alg}" not in fx:
                continue
            ex = _exons(fx[f"rng_eij_A{alg}"].reshape(-1, 21).tolist())
            cigar_properties(fx[f"rng_cigar_A{alg}"].reshape(-1, 2), ex)
            vulgar_properties(fx[f"rng_vulgar_A{alg}"].reshape(-1, 3), ex)
            n += 1
    assert n >= 6


def intron_gaps_h(exons):
    """the gap behind every intron record of the protein walk (the frame-shift rows, ISCR == NEVSEL, close no intron)"""
    return [b[F["left"]] - a[F["right"]] for a, b in zip(exons, exons[1:]) if a[F["iscr"]] != rc.NEVSEL]


def cigar_properties_h(cig, exons):
    """protein Cigar records of a list whose end-gap flags are 0: the N lengths, in order, are the gaps behind the intron records"""
    assert [int(n) for op, n in cig if chr(op) == "N"] == intron_gaps_h(exons)


def vulgar_properties_h(vul, exons):
    """protein Vulgar records: every intron as 5 / I / 3 with 2 + (len - 4) + 2 in the intron records' order; split-codon records
    come as a pair around the triple whose genomic parts make one codon; one F per frame-shift row"""
    vul = [(chr(o), int(a), int(b)) for o, a, b in vul]
    lens = []
    for k, (o, a, b) in enumerate(vul):
        if o == "I":
            assert vul[k - 1] == ("5", 0, 2) and vul[k + 1] == ("3", 0, 2) and a == 0
            lens.append(b + 4)
            before = vul[k - 2] if k >= 2 and vul[k - 2][0] == "S" else None
            after = vul[k + 2] if k + 2 < len(vul) and vul[k + 2][0] == "S" else None
            assert (before is None) == (after is None)
            if before:
                assert before[1] == 0 and after[1] == 1 and before[2] + after[2] == 3
    assert lens == intron_gaps_h(exons)
    assert sum(o in "53" for o, _, _ in vul) == 2 * len(lens) and sum(o == "S" for o, _, _ in vul) <= 2 * len(lens)
    assert sum(o == "F" for o, _, _ in vul) == sum(r[F["iscr"]] == rc.NEVSEL for r in exons[:-1])


def test_edit_properties_hold_for_the_reference_protein():
    """... on the h1_* / c1_* fixtures whose four flags are 0; the properties as such (no flag enters them) also on every other
    protein fixture but the one whose list the reference's flags change (h1_exg_0011 -A2: an intron behind a frame-shift row)"""
    n = n0 = n_s = 0
    for f in golden_files("h1_") + golden_files("c1_"):
        name = f.split("/")[-1][:-5]
        if name == "h1_cut_right":
            continue                                    # undefined in the reference (tests/test_oracle_h_golden.py)
        fx = spdg.load(f)
        q = fx["prm"]
        flags0 = not (q["a_exgl"] or q["a_exgr"] or q["b_exgl"] or q["b_exgr"] or q["local"])
        for alg in (0, 2):
            if f"rng_cigar_A{alg}" not in fx or (name == "h1_local_udh" and alg == 2) or (name == "h1_exg_0011" and alg == 2):
                continue
            ex = _exons(fx[f"rng_eij_A{alg}"].reshape(-1, 21).tolist())
            cigar_properties_h(fx[f"rng_cigar_A{alg}"].reshape(-1, 2), ex)
            vulgar_properties_h(fx[f"rng_vulgar_A{alg}"].reshape(-1, 3), ex)
            n += 1
            n0 += flags0
            n_s += int((fx[f"rng_vulgar_A{alg}"].reshape(-1, 3)[:, 0] == ord("S")).sum())
    assert n >= 60 and n0 >= 4 and n_s >= 8


def test_the_split_codon_records_do_not_follow_the_junction_phase():
    """the property one would expect -- an intron of phase -1 / 1 carries the S pair, one of phase 0 none -- is not the reference's:
    its S records follow what the last frame shift left in `phs` (h1_basic: phases 0, 1, 1 and no S record at all)"""
    fx = spdg.load([f for f in golden_files("h1_") if f.endswith("h1_basic.spdg")][0])
    ex = _exons(fx["rng_eij_A2"].reshape(-1, 21).tolist())
    assert any(r[F["phs"]] != 0 for r in ex[:-1]) and not (fx["rng_vulgar_A2"].reshape(-1, 3)[:, 0] == ord("S")).any()
