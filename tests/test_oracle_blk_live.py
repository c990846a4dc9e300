"""The block-search restatement (oracle/spdp_oracle_blk.c) against the compiled reference itself, run here, on what no recorded
fixture can hold: a repetitive genome of 24 chromosomes whose index -- formatted by the reference's own `spaln -W -KD -XC5 -Xb256` --
has posting lists past 128 entries (two of them are merged by the oracle's restatement of Qwords::next_mrglist), with copies of
the repeat, queries longer than 2048 residues, fragments and noise.  Every query runs in a reference process of its own (a fresh
worker: grown tables do not carry over) with the recorder of oracle/ref_build/blk_tap.cc; the oracle has to equal every recorded
TestOutput call.  A recorded fixture of this kind does not fit the repository: a call's record lists every block that scored, some
20 000 ints on such an index, and an index small enough for short records has no long lists (the builder drops words that are in
too many of few blocks).  Needs oracle/_ref (built where the reference's sources are); skipped elsewhere.

What this cannot pin: growth of the run hash.  The reference sizes that table from its longest list (here 409 slots for lists
of 169 at the most), so that with its own geometry no scan fills it; tests/vote_cases.py shrinks the table by hand."""
import os
import subprocess

import numpy as np
import pytest

from oracle import blk
from tests import spdg, vote_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
DEC = {2: "A", 3: "C", 5: "G", 9: "T"}


def letters(a):
    return "".join(DEC[int(x)] for x in a)


@pytest.mark.skipif(not (os.path.exists(os.path.join(REF, "spaln")) and os.path.exists(os.path.join(REF, "spaln_blktap"))),
                    reason="the compiled reference (oracle/_ref) is not on this machine")
def test_oracle_equals_the_reference_on_a_repetitive_genome(tmp_path):
    rng = np.random.default_rng(20270)
    element = vc.random_dna(rng, 900)
    codes, off = vc.make_genome(rng, [18000 + 900 * i for i in range(24)], element, 1000, 0.03)
    qs = [vc.mutate(rng, element, 0.03)[int(rng.integers(0, 100)):int(rng.integers(400, 900))] for _ in range(50)]
    qs += [vc.fragment(rng, codes, 60, 800) for _ in range(40)]
    qs += [np.concatenate([vc.fragment(rng, codes, 500, 900) for _ in range(4)])[:int(rng.integers(2100, 3000))] for _ in range(20)]
    qs += [vc.random_dna(rng, int(rng.integers(100, 900))) for _ in range(30)]
    td = str(tmp_path)
    env = dict(os.environ, ALN_TAB=os.path.join(REF, "table"), ALN_DBS=td)
    with open(os.path.join(td, "gnm.mfa"), "w") as f:
        for c in range(24):
            t = letters(codes[off[c]:off[c + 1]])
            f.write(f">chr{c + 1}\n")
            f.writelines(t[i:i + 60] + "\n" for i in range(0, len(t), 60))
    subprocess.run([os.path.join(REF, "spaln"), "-W", "-KD", "-XC5", "-Xb256", "gnm.mfa"], cwd=td, env=env, check=True, capture_output=True)
    fx, ix, n_calls, n_long, lane_merges = None, None, 0, 0, 0
    for i, q in enumerate(qs):
        with open(os.path.join(td, "one.fa"), "w") as f:
            f.write(f">q{i}\n{letters(q)}\n")
        log = os.path.join(td, f"one{i}.spdg")
        subprocess.run([os.path.join(REF, "spaln_blktap"), "-Q7", "-O4", "-t1", "-dgnm", "one.fa"], cwd=td, env=dict(env, SPDP_BLK_LOG=log),
                       check=True, capture_output=True)
        got = spdg.load(log)
        if fx is None:
            fx = got
            fx["blk_convtab"][:2] = 255
            ix, _keep = blk.index_of(fx)
            lens = vc.list_lengths(fx)
            assert ix.n_chr == 24 and ix.kk == 3 and (lens > 128).sum() >= 20
            assert ix.hh_size1 > 2 * int(lens.max())                 # (why the run hash never grows under the reference's own geometry)
        for rec in blk.parse_log(dict(q_log=got["q_log"], blk_prm=fx["blk_prm"])):
            n_long += len(rec["codes"]) > 2048
            for ci, (want_vote, want_pairs) in enumerate(rec["calls"]):
                mine = blk.vote(ix, rec["codes"], rec["left"], rec["right"], ci)
                assert mine is not None and np.array_equal(mine[0], want_vote), (i, ci)
                if want_pairs is not None:
                    k = int(mine[1][1])
                    assert k >= 1 and np.array_equal(mine[1][2:2 + 9 * k], want_pairs[2:2 + 9 * k]), (i, ci)
                lane_merges += blk.last_paths()["lane_merges"]
                n_calls += 1
    assert n_calls >= 200 and n_long >= 15 and lane_merges > 0, (n_calls, n_long, lane_merges)
