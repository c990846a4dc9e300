"""The group forms of the map + align entries with the preparation in front and of the dispersed ones (spdp_group_map_align_s_prep,
_s_multi_prep, _s_dispersed, _h_dispersed): three contexts on ONE card against the single-context entry.  The inputs are those of
tests/test_gpu_e2e_dispersed.py (its `small` set-up on blk_k1) and tests/test_gpu_map_multi.py (its Case on the paralog and the
protein genome), with what the end-to-end tools plant added by hand: poly-A tails, antisense reads with poly-T heads, and queries
joined from two transcripts.  Genes, exons, part, covered and tails must be identical."""
import numpy as np
import pytest

from spaln_amd import blocks, engine
from tests.test_gpu_e2e_dispersed import small  # noqa: F401  (a module-scoped fixture: one context, blk_k1, eight queries)
from tests.test_gpu_map_multi import Case

pytestmark = pytest.mark.gpu

COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ((2, 9), (9, 2), (3, 5), (5, 3)):
    COMP[_a] = _b


@pytest.fixture(scope="module")
def grp():
    g = engine.Group([0, 0, 0])
    yield g
    g.close()


def tailed(queries):
    """a third as they are, a third with a poly-A tail, a third as antisense reads with a poly-T head"""
    tail = np.full(25, 2, dtype=np.uint8)
    out = []
    for i, q in enumerate(queries):
        t = np.concatenate([q, tail]) if i % 3 else q
        out.append(np.ascontiguousarray(COMP[t[::-1]]) if i % 3 == 2 else np.ascontiguousarray(t))
    return out


def joined(queries):
    """the queries, and between them transcripts joined from two of them: whole + whole, whole + first third, last quarter + whole"""
    out = []
    for i, q in enumerate(queries):
        o = queries[(i + 3) % len(queries)]
        out.append(q)
        out.append(np.ascontiguousarray(np.concatenate([(q, o), (q, o[:len(o) // 3]), (q[-(len(q) // 4):], o)][i % 3])))
    return out


def plain(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    return x


def test_prep_twins(small, grp):  # noqa: F811
    s = small
    queries = tailed(joined(s["queries"])[:12] + s["queries"])
    args = (s["gen"], s["off"], s["sc"], s["sp"], s["sig"], s["prm"], s["rescore"], queries)
    gix = blocks.GroupIndex(grp, fixture_of("blk_k1"))
    try:
        for q_mns in (1, 3):
            want = blocks.map_align_prep(s["dix"], *args, q_mns=q_mns)
            got = blocks.group_map_align_prep(gix, *args, q_mns=q_mns)
            assert plain(got[0]) == plain(want[0]) and got[2] == want[2] and got[3].tolist() == want[3].tolist(), q_mns
            assert set(grp.shards(len(queries)).tolist()) == {0, 1, 2}
            assert sum(1 for g in want[0] if g is not None) >= len(queries) // 2
            pols = {int(p) for p in want[3][:, 0]}
            assert 1 in pols and (2 in pols) == (q_mns == 3)            # A tails, and T heads where they are looked for
            assert max(got[1]) > 0
            wantm = blocks.map_align_multi_prep(s["dix"], *args, q_mns=q_mns)
            gotm = blocks.group_map_align_multi_prep(gix, *args, q_mns=q_mns)
            assert plain(gotm[0]) == plain(wantm[0]) and gotm[2] == wantm[2] and gotm[3].tolist() == wantm[3].tolist(), q_mns
    finally:
        gix.free()


def fixture_of(name):
    from tests import spdg
    from tests.conftest import golden_files
    return spdg.load([f for f in golden_files("blk_") if f.endswith(name + ".spdg")][0])


@pytest.mark.parametrize("prep", [None, (3, 12)], ids=["ori", "prep"])
def test_dispersed_twin(small, grp, prep):  # noqa: F811
    s = small
    queries = joined(s["queries"])
    if prep is not None:
        queries = tailed(queries)
    args = (s["gen"], s["off"], s["sc"], s["sp"], s["sig"], s["prm"], s["rescore"], queries)
    gix = blocks.GroupIndex(grp, fixture_of("blk_k1"))
    try:
        for ori in ((1, 3) if prep is None else (1,)):
            want = blocks.map_align_dispersed(s["dix"], *args, min_seg_len=21, ori=ori, prep=prep)
            got = blocks.group_map_align_dispersed(gix, *args, min_seg_len=21, ori=ori, prep=prep)
            lists, covered, sec, rc, rec = got
            assert plain(lists) == plain(want[0]), ori                  # genes, exons and every gene's part, in the caller's order
            assert covered.tolist() == want[1].tolist() and rc == want[3]
            assert (rec is None and want[4] is None) if prep is None else rec.tolist() == want[4].tolist()
            assert set(grp.shards(len(queries)).tolist()) == {0, 1, 2}
            parts = [g["part"] for lst in lists for g in lst]
            assert max(len(lst) for lst in lists) >= 2 and {1, 2} & set(parts), parts   # the joined queries: records of a rest
            assert max(sec) > 0
    finally:
        gix.free()


def test_protein_dispersed_twin(grp):
    eng = engine.Engine(0)
    try:
        c = Case(eng, "map_multi_p1", max_out=1)
        gix = None
        try:
            gix = blocks.GroupIndex(grp, c.fx)
            queries = joined(c.queries[:12])
            args = (c.gen, c.off, c.sc, c.sp, c.sigmodel, c.prm, c.rescore, queries, 12)
            want = blocks.map_align_h_dispersed(c.ix, *args)
            got = blocks.group_map_align_h_dispersed(gix, *args)
            assert plain(got[0]) == plain(want[0]) and got[1].tolist() == want[1].tolist() and got[3] == want[3]
            assert set(grp.shards(len(queries)).tolist()) == {0, 1, 2}
            assert sum(len(lst) for lst in want[0]) >= len(queries) // 2 and max(len(lst) for lst in want[0]) >= 2
        finally:
            if gix is not None:
                gix.free()
            c.free()
    finally:
        eng.close()
