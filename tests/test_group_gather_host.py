"""spaln_amd/csrc/spdp_group_gather.h -- what puts the ragged results of a group's members back into the caller's order -- on
generated shards, without a GPU: tests/group_gather_host_check.cpp (a program with its own main) is built with
-fsanitize=address,undefined and run on a text dump of the cases; nothing is loaded into Python.  The gathered arrays must be the
plain restatement's: the members' lists concatenated in the caller's query order, the offsets counted again.  The sanitizers must
have nothing to say (the program's pools are exactly as large as the header's totals() says)."""
import os
import random
import subprocess

import pytest

from spaln_amd import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = (1, 2, 3, 5, 8)


def lists_of(rng, n, shape):
    """per query its records [(value, [side entries])]"""
    out = []
    for i in range(n):
        if shape == "no_side":                      # lists whose pooled side arrays are empty
            k = rng.randrange(0, 4)
            out.append([(rng.randrange(-99, 100), []) for _ in range(k)])
            continue
        if shape == "all_empty":
            out.append([])
            continue
        k = rng.randrange(0, 5)
        if shape == "edges" and (i in (0, 1, n - 1) or i % 4 == 2):     # empty lists at the start, between full ones, at the end
            k = 0
        elif shape == "edges":
            k = max(k, 2)
        out.append([(rng.randrange(-999, 1000), [rng.randrange(1, 10 ** 6) for _ in range(rng.randrange(0, 4))]) for _ in range(k)])
    return out


def cases():
    rng = random.Random(20260101)
    out = []
    for w in MEMBERS:
        for n in sorted({0, 1, 2, max(w - 1, 0), w, w + 1, 3 * w + 1, 23}):
            for shape in ("edges", "mixed", "no_side", "all_empty"):
                lists = lists_of(rng, n, shape)
                # who serves what: the product's rule on costs of its kind (1 + a length), and once a member set with holes
                costs = [1 + rng.randrange(0, 50) for _ in range(n)]
                shards = shard.balanced_shards(costs, w)
                owner = [-1] * n
                for r, s in enumerate(shards):
                    for i in s:
                        owner[i] = r
                out.append((w, owner, lists))
        # every query on the LAST member: the others stay empty
        lists = lists_of(rng, 6, "mixed")
        out.append((w, [w - 1] * 6, lists))
        # a query nobody served keeps an empty slot
        lists = lists_of(rng, 7, "mixed")
        out.append((w, [(-1 if i == 3 else i % w) for i in range(7)], lists))
    return out


def dump(cs):
    lines = []
    for w, owner, lists in cs:
        lines.append(f"CASE {w} {len(lists)}")
        for m, recs in zip(owner, lists):
            lines.append(f"Q {m} {len(recs)}")
            for v, side in recs:
                lines.append(" ".join(str(x) for x in ["R", v, len(side)] + side))
    return "\n".join(lines) + "\n"


def restated(w, owner, lists):
    """concatenate in caller order, recompute offsets"""
    n = len(lists)
    served = [recs if m >= 0 else [] for m, recs in zip(owner, lists)]
    want = {"V": [], "O": [0], "L": [], "K": [], "S": [], "D": [], "P": {}}
    for i, (m, recs) in enumerate(zip(owner, lists)):
        pair = [len(recs), sum(v for v, _ in recs)]
        want["V"] += pair if m >= 0 else [-7, -7]
        if m >= 0:
            want["P"].setdefault(m, []).extend(pair)
        for v, side in served[i]:
            want["L"].append(v)
            want["K"].append(i)
            want["S"].append(len(want["D"]))
            want["D"] += side
        want["O"].append(len(want["L"]))
    want["T"] = [len(want["L"]), len(want["D"])]
    want["M"] = want["O"] + want["L"]
    assert len(want["O"]) == n + 1
    return want


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("group_gather") / "group_gather_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", out, os.path.join(ROOT, "tests", "group_gather_host_check.cpp")])
    return out


def test_gathered_arrays_equal_the_restatement(exe, tmp_path):
    cs = cases()
    assert {w for w, _, _ in cs} == set(MEMBERS)
    assert any(len(l) == 0 for _, _, l in cs) and any(len(l) == 1 for _, _, l in cs) and any(0 < len(l) < w for w, _, l in cs)
    path = tmp_path / "cases.txt"
    path.write_text(dump(cs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-400:], r.stderr[-2000:])      # a clean sanitizer exit
    got, cur = [], None
    for ln in r.stdout.splitlines():
        f = ln.split()
        assert f[0] != "FAILED", ln
        if f[0] == "CASE":
            cur = {"P": {}, "head": (int(f[1]), int(f[2]))}
            got.append(cur)
        elif f[0] == "P":
            cur["P"][int(f[1])] = [int(x) for x in f[2:]]
        else:
            cur[f[0]] = [int(x) for x in f[1:]]
    assert len(got) == len(cs)
    n_rec = n_side = 0
    for (w, owner, lists), g in zip(cs, got):
        want = restated(w, owner, lists)
        assert g["head"] == (w, len(lists))
        for key in ("V", "T", "O", "L", "K", "S", "D", "M", "P"):
            assert g[key] == want[key], (w, len(lists), key, owner, g[key], want[key])
        n_rec += want["T"][0]
        n_side += want["T"][1]
    assert n_rec > 500 and n_side > 500                  # (the cases are not all empty ones)
