"""tests/hsp_cases.py held to its effects, without a GPU, and the host side of the HSP search's request path (spdp_hsp_plan,
spdp_hsp_tasks_host) with it.

Three parties: the recipes (what a case is built for), hsp_cases.restate (a plain restatement of the search that also says which
branch every step took) and the product's host form behind spdp_hsp_tasks_host.  The restatement's word stage must give the host
form's count of shared words, its segments and records the host form's, on every task; the recipes' effects and the census of
classes are then read from the restatement's branches.  The flags the device form will give a task are arithmetic on the host
form's three counts and the plan (hsp_cases.flags_of): every cap case has exactly the flag it is built for and none at the cap,
every other case is free of flags under the plan spdp_blk_find would choose -- so tests/test_gpu_hsp_cases.py cannot pass on
tasks handed back.

The census the committed generator gives (python -m pytest tests/test_hsp_cases.py -s prints it): test_every_class_is_well_populated."""
import collections
import ctypes as C

import numpy as np
import pytest

from spaln_amd import abi, blocks, engine
from tests import hsp_cases as hc
from tests import envknobs

CLASS_FLOOR = 20
CLASSES = ("gain1", "first_word_bonus", "over", "gap_0", "gap_1", "gap_more", "segment_goes_on_over_a_gap", "segment_closed_by_a_gap",
           "run_dropped_at_a_gap_best_eq_cutoff", "segment_at_cutoff_plus_1", "query_word_at_or_above_mask",
           "backward_to_query_0", "backward_to_region_0", "forward_to_tlen_below_a_len", "forward_to_region_end", "restart_inside_the_seed",
           "window_starts_after_a_restart", "identical_bonus", "one_mismatch_short_of_identical", "exgl_bonus", "exgr_bonus",
           "crs0_mismatches_0", "crs0_mismatches_1", "crs0_mismatches_3", "crs0_mismatches_4", "ser_ser2", "short_query", "empty")
RECIPE_FLOOR = dict.fromkeys(("words/copy", "words/outside_alphabet", "words/pattern_position", "words/lattice_width", "words/lattice_width_plus_1",
                              "words/two_runs_at_cutoff", "stretch/exg", "stretch/protein_mismatches", "ranges/short_query", "ranges/tiny", "reuse"), 20)
RECIPE_FLOOR.update({"caps/words": 10, "caps/segments": 10, "caps/records": 10, "caps/nk": 10, "key_limit": 2, "mixed_batch": 6})


@pytest.fixture(scope="module")
def lib():
    return engine.load_library()


def host(lib, rq):
    return blocks.hsp_tasks_host(lib, rq["model"], rq["genome"], rq["chr_off"], rq["queries"], rq["tasks"], rq["ranges"], rq["tlen"], rq["exg"])


def plan_of(lib, rq):
    """the plan the request runs under: its explicit fields, the rest as spdp_blk_find chooses for the request's longest range"""
    longest = max(r - l for l, r in rq["ranges"])
    return blocks.hsp_plan(lib, longest, rq["model"].mtx_rows, rq["model"].mtx_cols, len(rq["tasks"]), 256, **rq["plan"])


@pytest.fixture(scope="module")
def runs(lib):
    """per request: the host form's records and counts, the restatement of every task"""
    out = []
    for rq in hc.requests():
        recs, counts = host(lib, rq)
        out.append((rq, recs, counts, [hc.restate(rq, t) for t in rq["tasks"]]))
    return out


def test_word_stage_and_every_record_equal_the_restatement(runs):
    n = n_rec = 0
    for rq, recs, counts, rs in runs:
        for k, r in enumerate(rs):
            where = (rq["name"], k, rq["cases"][k].recipe)
            assert r["words"] == counts[k][0], where                  # the word stage alone: classes, pattern, mask
            assert len(r["segments"]) == counts[k][1], where
            assert r["records"].tolist() == recs[k].tolist(), where
            assert len(recs[k]) == counts[k][2], where
            n += 1
            n_rec += len(recs[k])
    assert n >= 1000 and n_rec >= 1000


def test_every_class_is_well_populated(runs):
    """What the committed generator gives (tasks per class; a task counts for every branch its search takes): 1368 tasks in 39
    calls, 683 of them on the other strand.  gain1 957, first_word_bonus 259, over 69 (the end's term decides: over_idle 137 more
    take it idly), gap_0 24, gap_1 43, gap_more 170, segment_goes_on_over_a_gap 150, segment_closed_by_a_gap 28,
    run_dropped_at_a_gap_best_eq_cutoff 24, segment_at_cutoff_plus_1 28, query_word_at_or_above_mask 126, backward_to_query_0 76,
    backward_to_region_0 31, forward_to_tlen_below_a_len 24, forward_to_region_end 85, restart_inside_the_seed 24,
    window_starts_after_a_restart 24, identical_bonus 549, one_mismatch_short_of_identical 96, exgl_bonus 43, exgr_bonus 86,
    crs0_mismatches 0 / 1 / 3 / 4 and more: 104 / 32 / 24 / 50, ser_ser2 96, short_query 149, empty 123.
    gap_0 needs a spaced pattern (adjacent words of a contiguous one overlap).  A first run whose best equals the cutoff exists
    for the nucleotide models only: the protein fixture's gains are multiples of 4, its cutoff is 51."""
    count, recipes, strands = collections.Counter(), collections.Counter(), collections.Counter()
    for rq, recs, counts, rs in runs:
        for k, r in enumerate(rs):
            count.update(r["branches"])
            recipes[rq["cases"][k].recipe] += 1
            strands[rq["tasks"][k][4]] += 1
    print("\n%d tasks in %d calls, %d on the other strand" % (sum(strands.values()), len(runs), strands[1]))
    for c in sorted(count):
        print("  %-44s %d" % (c, count[c]))
    for c in sorted(recipes):
        print("  recipe %-37s %d" % (c, recipes[c]))
    for c in CLASSES:
        assert count[c] >= CLASS_FLOOR, (c, count[c])
    for c, floor in RECIPE_FLOOR.items():
        assert recipes[c] >= floor, (c, recipes[c])
    assert 0.4 <= strands[1] / sum(strands.values()) <= 0.6


def _on_diagonal(recs, r):
    return [x for x in recs.tolist() if x[5] == r]


def test_recipes_have_the_effects_they_are_named_for(runs):
    seen = collections.Counter()
    for rq, recs, counts, rs in runs:
        S = rq["shape"]
        for k, (c, r) in enumerate(zip(rq["cases"], rs)):
            br, mine = r["branches"], (_on_diagonal(recs[k], c.g0) if c.g0 is not None else None)
            plain = rq["key"] in ("nt", "nt_contig", "aa", "aa_contig")       # (nt_mask loses words of its own; aa_crs0 prices mismatches)
            if c.recipe == "words/copy":
                assert len(mine) == 1 and mine[0][0] == c.left and mine[0][2] >= c.right - c.left and ("gain1" in br or not plain), (rq["name"], k)
            elif c.recipe in ("words/gain1", "words/first_word", "words/over") and plain:
                # the term the recipe is named for makes the segment: a record on the planted diagonal; its neighbour, one word fewer
                # or the same run where the term does not reach, has none
                want = {"words/gain1": "gain1", "words/first_word": "first_word_bonus", "words/over": "over"}[c.recipe]
                if c.recipe == "words/gain1":
                    assert r["per_diagonal"][c.g0] < hc.min_words(S, gain1=False), (rq["name"], k)
                assert want in br and len(mine) == 1 and mine[0][3] == mine[0][2], (rq["name"], k, br)
            elif c.recipe in ("words/gain1_not", "words/first_word_not", "words/over_not"):
                assert not mine and not r["segments"], (rq["name"], k)
            elif c.recipe == "words/two_runs_goes_on" and plain:
                assert "segment_goes_on_over_a_gap" in br and len(r["segments"]) == 1 and len(mine) == 1, (rq["name"], k)
            elif c.recipe == "words/two_runs_closed" and plain:
                assert "segment_closed_by_a_gap" in br and len(r["segments"]) == 2 and len(mine) == 2, (rq["name"], k)
            elif c.recipe == "words/two_runs_at_cutoff":
                assert "run_dropped_at_a_gap_best_eq_cutoff" in br and len(r["segments"]) == 1 and len(mine) == 1, (rq["name"], k)
            elif c.recipe == "words/pattern_position":
                cared = "cared for" in c.effect
                assert r["per_diagonal"].get(c.g0, 0) == (0 if cared else 1), (rq["name"], k, c.effect)
            elif c.recipe == "words/lattice_width":
                assert ("gap_0" in br) == (len(S["exam"]) < S["width"]), (rq["name"], k)
            elif c.recipe == "words/lattice_width_plus_1" and plain and rq["key"] != "aa":      # (11011 read six apart matches itself three apart)
                assert "gap_1" in br, (rq["name"], k)
            elif c.recipe == "stretch/query_0":
                assert "backward_to_query_0" in br and mine and mine[0][0] == 0, (rq["name"], k)
            elif c.recipe == "stretch/region_0" and plain:
                assert "backward_to_region_0" in br and mine and mine[0][1] in (0, -1), (rq["name"], k, mine)
            elif c.recipe == "stretch/tlen":
                assert "forward_to_tlen_below_a_len" in br and mine and mine[0][0] + mine[0][2] == c.tlen < len(c.q), (rq["name"], k)
            elif c.recipe == "stretch/region_end" and plain:
                stop = c.b_len - 1 if S["bbt"] == 3 else c.b_len
                assert "forward_to_region_end" in br and mine and stop - S["bbt"] <= mine[0][1] + S["bbt"] * mine[0][2] <= stop + 1, (rq["name"], k, mine, stop)
            elif c.recipe == "stretch/restart" and plain:
                assert "window_starts_after_a_restart" in br and len(mine) == 1, (rq["name"], k)
            elif c.recipe == "stretch/one_mismatch" and plain:
                assert mine and mine[0][2] - mine[0][3] == 1, (rq["name"], k)
            elif c.recipe == "ranges/tiny":
                usable = c.right - c.left >= S["width"] and c.b_len >= S["bbt"] * S["width"]
                assert ("empty" in br) == (not usable) and not len(recs[k]), (rq["name"], k)
            elif c.recipe == "ranges/short_query" and plain:
                # a record exactly where the query is below shortquery: the run lies between the scaled and the unscaled cut-off
                # (the contiguous nucleotide word's run of 22 residues is a segment there, and too short for a record)
                assert bool(r["segments"]) == (len(c.q) < S["short"]) and (bool(mine) == bool(r["segments"]) or rq["key"] == "nt_contig" or (c.exg == (0, 1) and S["bbt"] == 3)), (rq["name"], k, len(c.q), r["segments"])
            else:
                continue
            seen[c.recipe] += 1
    # the score differs by exactly the term the recipe toggles against its neighbour: exg on and off on the same run
    by_run = {}
    for rq, recs, counts, rs in runs:
        for k, c in enumerate(rq["cases"]):
            if c.recipe == "stretch/exg" and len(recs[k]):
                x = recs[k][0]
                S = rq["shape"]
                seed_at = c.left + x[6]                               # (the left end's bonus is taken where the seed begins, before the walk back)
                at_left, at_right = seed_at < S["tpl"], S["tpl"] - c.right + x[0] + x[2] > 0
                base = int(S["mtx"][c.q[x[0]:x[0] + x[2]], c.q[x[0]:x[0] + x[2]]].sum()) if x[2] == x[3] else None
                if base is None or rq["key"] == "aa_crs0":
                    continue
                want = base + (S["end_bonus"] * min(S["tpl"] - seed_at, S["tpl"]) if c.exg[0] and at_left else 0)
                want += S["end_bonus"] * min(S["tpl"] - c.right + x[0] + x[2], S["tpl"]) if c.exg[1] and at_right else S["end_bonus"] * 4
                assert x[4] == want, (rq["name"], k, x.tolist(), want)
                by_run[(c.exg, at_left, at_right)] = by_run.get((c.exg, at_left, at_right), 0) + 1
    assert len(by_run) >= 10 and min(by_run.values()) >= 2, by_run
    for name in ("words/copy", "words/gain1", "words/first_word", "words/over", "words/two_runs_at_cutoff", "stretch/tlen", "stretch/query_0"):
        assert seen[name] >= 12, (name, seen[name])


def test_flags_are_the_ones_the_cases_are_built_for(lib, runs):
    """the condition that keeps the GPU test from passing on fallbacks, established by the host form alone"""
    n_flagged = collections.Counter()
    for rq, recs, counts, rs in runs:
        plan = plan_of(lib, rq)
        for k, c in enumerate(rq["cases"]):
            f = hc.flags_of(rq, rq["tasks"][k], *[int(x) for x in counts[k]], plan)
            words, segs, n_rec = (int(x) for x in counts[k])
            nk = c.right - c.left - (rq["shape"]["width"] - 1)
            if c.recipe.startswith("caps/"):
                beyond = c.effect.endswith("+ 1")
                what = c.recipe[5:]
                assert f == (0 if not beyond else hc.TOO_LONG if what == "nk" else hc.TOO_MANY), (rq["name"], k, c.effect, counts[k])
                over = dict(words=words - plan["hit_cap"], segments=segs - plan["seg_cap"], records=n_rec - plan["out_cap"], nk=nk - plan["hash_slots"] // 2)
                assert over[what] == (1 if beyond else 0), (rq["name"], k, c.effect, over)              # at the cap exactly, or one beyond
                assert all(v <= 0 for w, v in over.items() if w != what), (rq["name"], k, over)            # ... and the one intended
                n_flagged[what] += beyond
            elif c.recipe == "key_limit":
                beyond = c.effect.endswith("+ 1")
                nn = c.b_len - (rq["shape"]["width"] - 1)
                assert nk == hc.KEY_LIMIT_NK and ((nn + nk - 1) << 12 > 0xfffffff0) == beyond and ((nn + nk - 2) << 12 > 0xfffffff0) is False
                assert f == (hc.TOO_LONG if beyond else 0) and len(recs[k]) == 1
            elif c.recipe == "mixed_batch":
                assert plan["hash_slots"] == 8192 and f == (hc.TOO_LONG if len(c.q) == 5000 else 0) and len(recs[k]) >= 1
            else:
                assert f == 0, (rq["name"], k, c.recipe, counts[k], plan)
    assert all(n_flagged[w] >= 4 for w in ("words", "segments", "records", "nk")), n_flagged


def test_reuse_order_puts_busy_empty_and_single_word_tasks_on_one_wave(runs):
    for rq, recs, counts, rs in runs:
        if rq["plan"].get("n_waves") != 3:
            continue
        assert len(rq["tasks"]) in (100, 200)
        for k in range(0, len(rq["tasks"]) - 6, 9):                     # wave w serves tasks w, w + 3, w + 6, ..
            for w in range(3):
                busy, empty, one = counts[k + w], counts[k + 3 + w], counts[k + 6 + w]
                assert busy[0] >= 40 and busy[1] >= 5 and empty.tolist() == [0, 0, 0] and one.tolist() == [1, 0, 0], (rq["name"], k, busy, empty, one)


def test_plan_function(lib):
    """the slots, hit_cap and waves of today's HspBatch::run: slots = the power of two from 256 that holds twice the longest range, at
    most 8192; hit_cap 4096 up to 1024 slots, else 8192; seg_cap 256, out_cap 96; waves = min(tasks, CUs x min(8, 160 KB / LDS))"""
    for longest, slots, hits in ((1, 256, 4096), (128, 256, 4096), (129, 512, 4096), (4096, 8192, 8192), (4097, 8192, 8192), (100000, 8192, 8192)):
        for rows, cols in ((17, 17), (23, 26)):
            p = blocks.hsp_plan(lib, longest, rows, cols, 100000, 256)
            lds = 4 * (8 + 32 + 32 + rows * cols + 16 + slots + hits + 4 * 256 + slots // 2 + slots // 4 + 8)
            per_cu = max(1, min(8, (160 << 10) // lds))
            assert (p["hash_slots"], p["hit_cap"], p["seg_cap"], p["out_cap"], p["lds_bytes"], p["waves_per_cu"], p["n_waves"]) == \
                (slots, hits, 256, 96, lds, per_cu, 256 * per_cu), (longest, p)
            assert blocks.hsp_plan(lib, longest, rows, cols, 7, 256)["n_waves"] == 7
            assert blocks.hsp_plan(lib, longest, rows, cols, 7, 0)["n_waves"] == per_cu
    p = blocks.hsp_plan(lib, 100, 17, 17, 10, 256, hash_slots=256, hit_cap=256, seg_cap=8, out_cap=4, n_waves=3)
    assert (p["hash_slots"], p["hit_cap"], p["seg_cap"], p["out_cap"], p["n_waves"]) == (256, 256, 8, 4, 3)


def test_plan_rounds_spdp_hsp_hits_up_to_a_power_of_two(lib):
    """the sort pads the list of shared words to the next power of two in place: any other hit_cap let it write past the list"""
    for given, want in (("1", 256), ("256", 256), ("257", 512), ("300", 512), ("4096", 4096), ("5000", 8192), ("8193", 16384), ("junk", 256)):
        with envknobs.Env(SPDP_HSP_HITS=given):
            assert blocks.hsp_plan(lib, 100, 17, 17)["hit_cap"] == want, given
            assert blocks.hsp_plan(lib, 100, 17, 17, hit_cap=1024)["hit_cap"] == 1024         # (an explicit value stands)
    with envknobs.Env(SPDP_HSP_HITS="65536"):
        with pytest.raises(RuntimeError, match="LDS exceeds"):
            blocks.hsp_plan(lib, 100, 17, 17)
    assert blocks.hsp_plan(lib, 100, 17, 17)["hit_cap"] == 4096


def test_refusals_by_name(lib):
    for bad, why in ((dict(hash_slots=300), "hash_slots is not a power of two"), (dict(hash_slots=32), "hash_slots is not a power of two"),
                     (dict(hit_cap=1000), "hit_cap is not a power of two"), (dict(hit_cap=32), "hit_cap is not a power of two"),
                     (dict(hit_cap=1 << 16, hash_slots=8192), "LDS exceeds"), (dict(hash_slots=1 << 16), "LDS exceeds"), (dict(seg_cap=-1), "out of range")):
        with pytest.raises(RuntimeError, match=why):
            blocks.hsp_plan(lib, 100, 17, 17, **bad)
    m = hc.model("nt")
    q = [np.full(40, hc.A, dtype=np.uint8)]
    gen, off = np.full(300, hc.C_, dtype=np.uint8), np.array([0, 100, 300], dtype=np.int64)
    ok = dict(model=m, genome_codes=gen, chr_off=off, queries=q, tasks=[(0, 0, 10, 90, 0)])

    def refused(why, **change):
        with pytest.raises(RuntimeError, match=why):
            blocks.hsp_tasks_host(lib, **dict(ok, **change))
    blocks.hsp_tasks_host(lib, **ok)
    refused("outside its chromosome", tasks=[(0, 0, 10, 91, 0)])
    refused("outside its chromosome", tasks=[(0, 1, 150, 51, 1)])
    refused("outside its chromosome", tasks=[(0, 0, -1, 20, 0)])
    refused("left / right / tlen outside the query", ranges=[(0, 41)])
    refused("left / right / tlen outside the query", ranges=[(-1, 40)])
    refused("left / right / tlen outside the query", ranges=[(30, 20)])
    refused("left / right / tlen outside the query", tlen=[41])
    refused("a query code at or above mtx_rows", queries=[np.array([2] * 39 + [m.mtx_rows], dtype=np.uint8)])
    refused("names no query", tasks=[(1, 0, 10, 20, 0)])
    odd = abi.WilipModel.from_buffer_copy(m)
    odd.level[0].bitpat_len = odd.level[0].width - 1
    refused("pattern's length differs from width", model=odd)
    few = abi.WilipModel.from_buffer_copy(m)
    few.mtx_cols = 16
    refused("no column for every genomic code", model=few)


def test_genome_codes_beyond_the_alphabet_read_as_n(lib):
    """the host form cuts a region with codes above 16 read as 16 on both strands, as the device form does"""
    rq = next(r for r in hc.requests() if r["name"] == "nt/exg00/default")
    gen = rq["genome"].copy()
    at = np.arange(5, len(gen), 37)
    gen[at] = hc.N
    want = blocks.hsp_tasks_host(lib, rq["model"], gen.copy(), rq["chr_off"], rq["queries"], rq["tasks"], rq["ranges"], rq["tlen"], rq["exg"])
    assert sum(len(r) for r in want[0]) >= 50
    gen[at[::2]] = 17
    gen[at[1::2]] = 255
    got = blocks.hsp_tasks_host(lib, rq["model"], gen, rq["chr_off"], rq["queries"], rq["tasks"], rq["ranges"], rq["tlen"], rq["exg"])
    assert all(a.tolist() == b.tolist() for a, b in zip(got[0], want[0])) and got[1].tolist() == want[1].tolist()


@pytest.mark.parametrize("name", ["blk_k1", "blk_p1"])
def test_the_searches_of_a_block_search_replayed_as_tasks_chain_to_the_same_units(lib, name):
    """every search the host path of the block search makes on a fixture (tests/test_blk_find.py pins that path to the reference's
    recorded runs; the checker taps its searches) run again as a task of spdp_hsp_tasks_host, its raw records chained with
    spdp_hsp::chain: the units the search itself handed to the locus logic"""
    from oracle import blk, oracle
    from tests import spdg
    from tests.conftest import golden_files
    from tests.test_blk_find import CASES, PROTEIN_CASES, find_calls, genome_of
    case = next(c for c in CASES + PROTEIN_CASES if c[0] == name)
    fx = spdg.load([f for f in golden_files("blk_") if f.endswith(name + ".spdg")][0])
    gen, off = genome_of(*case)
    ix, keep = blk.index_of(fx)
    model = abi.wilip_model_from_fixture(fx)
    prm = np.ascontiguousarray(fx["find_prm"], dtype=np.int32)
    ip = np.ascontiguousarray(fx["find_intpen"], dtype=np.int16)
    chk = C.CDLL(oracle._BLK_SO)
    chk.blk_check_tap.argtypes = [C.c_void_p, C.c_int]
    chk.blk_check_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    chk.blk_check_tap(None, 0)
    n_tasks = n_units = 0
    buf = np.zeros(1 << 20, dtype=np.int32)
    for q in blk.parse_log(fx)[:40]:
        find_calls(chk, fx, ix, keep, gen, off, model, prm, ip, q)
        n = chk.blk_check_tap(buf.ctypes.data, len(buf))
        assert n <= len(buf)
        tasks, want, i = [], [], 0
        while i < n:
            ch, rvs, base, ln, nf = (int(x) for x in buf[i:i + 5])
            tasks.append((0, ch, base, ln, rvs))
            want.append(buf[i + 5:i + 5 + nf].tolist())
            i += 5 + nf
        if not tasks:
            continue
        codes = np.ascontiguousarray(q["codes"], dtype=np.uint8)
        recs, _counts = blocks.hsp_tasks_host(lib, model, gen, off, [codes], tasks, [(q["left"], q["right"])], None, (int(prm[20]), int(prm[21])))
        for t, r, w in zip(tasks, recs, want):
            r = np.ascontiguousarray(r, dtype=np.int32)
            out = np.zeros(len(w) + 64, dtype=np.int32)
            k = chk.blk_check_chain(C.addressof(model), prm.ctypes.data, ip.ctypes.data, len(ip), len(codes), q["left"], q["right"], t[3],
                                    r.ctypes.data, len(r), out.ctypes.data, len(out))
            assert out[:k].tolist() == w, (name, t)
            n_units += w[0]
        n_tasks += len(tasks)
    assert n_tasks >= 40 and n_units >= 20, (n_tasks, n_units)
