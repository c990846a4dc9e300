"""spdp_hsp_search on the device against the host form of the same search, task by task and record by record: every call of
tests/hsp_cases.py through spdp_hsp_tasks and spdp_hsp_tasks_host.  The flags are the ones arithmetic on the host form's counts
and the plan predicts (tests/test_hsp_cases.py holds the generator to that without a GPU: exactly the intended flag on the cap
cases, none anywhere else -- so nothing here passes on a task handed back); an unflagged task has the host form's records, all
seven ints of each; of a flagged task only the flags are compared."""
import pytest

from spaln_amd import blocks
from tests import hsp_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from spaln_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host(eng):
    """per call the host form's (records, counts): computed once, shared"""
    return [blocks.hsp_tasks_host(eng.lib, rq["model"], rq["genome"], rq["chr_off"], rq["queries"], rq["tasks"], rq["ranges"], rq["tlen"], rq["exg"])
            for rq in hc.requests()]


def device(eng, rq, tasks=None, **plan):
    return blocks.hsp_tasks(eng, rq["model"], rq["genome"], rq["chr_off"], rq["queries"], rq["tasks"] if tasks is None else tasks, rq["ranges"],
                            rq["tlen"], rq["exg"], **dict(rq["plan"], **plan))


def check(rq, want, got, flags, plan, order=None):
    """got / flags of the tasks in `order` (default: the call's own) against the host form's records and the predicted flags"""
    recs, counts = want
    n_served = n_rec = 0
    for at, k in enumerate(range(len(rq["tasks"])) if order is None else order):
        where = (rq["name"], k, rq["cases"][k].recipe, rq["cases"][k].effect)
        f = hc.flags_of(rq, rq["tasks"][k], *[int(x) for x in counts[k]], plan)
        assert int(flags[at]) == f, where + (int(flags[at]), f, counts[k].tolist())
        if f:
            continue
        assert len(got[at]) == len(recs[k]), where + (got[at].tolist(), recs[k].tolist())
        assert got[at].tolist() == recs[k].tolist(), where
        n_served += 1
        n_rec += len(recs[k])
    return n_served, n_rec


def test_every_call_equals_the_host_form(eng, host):
    served = n_rec = flagged = 0
    for rq, want in zip(hc.requests(), host):
        got, flags, plan = device(eng, rq)
        for k, v in rq["plan"].items():
            assert plan[k] == v, (rq["name"], plan)
        s, r = check(rq, want, got, flags, plan)
        served, n_rec, flagged = served + s, n_rec + r, flagged + int((flags != 0).sum())
    assert served >= 1300 and n_rec >= 1200 and 20 <= flagged <= 40, (served, n_rec, flagged)


def test_task_order_and_wave_count_do_not_matter(eng, host):
    """the same tasks reversed, and on 1 and 3 waves: a wave's LDS is reused by every task of its stride"""
    for rq, want in zip(hc.requests(), host):
        n = len(rq["tasks"])
        order = list(range(n))[::-1]
        got, flags, plan = device(eng, rq, tasks=[rq["tasks"][k] for k in order])
        check(rq, want, got, flags, plan, order)
        for n_waves in (1, 3):
            got, flags, plan = device(eng, rq, n_waves=n_waves)
            assert plan["n_waves"] == n_waves
            check(rq, want, got, flags, plan)


def test_reuse_tasks_on_the_default_launch_give_equal_records(eng, host):
    n = 0
    for rq, want in zip(hc.requests(), host):
        if rq["plan"].get("n_waves") != 3:
            continue
        three = device(eng, rq)
        free = blocks.hsp_tasks(eng, rq["model"], rq["genome"], rq["chr_off"], rq["queries"], rq["tasks"], rq["ranges"], rq["tlen"], rq["exg"])
        assert three[2]["n_waves"] == 3 and free[2]["n_waves"] == len(rq["tasks"])
        assert all(a.tolist() == b.tolist() for a, b in zip(three[0], free[0])) and three[1].tolist() == free[1].tolist()
        check(rq, want, free[0], free[1], free[2])
        n += len(rq["tasks"])
    assert n >= 300


def test_refusals_by_name(eng):
    rq = next(r for r in hc.requests() if r["name"] == "nt/exg00/default")
    few = dict(model=rq["model"], genome_codes=rq["genome"], chr_off=rq["chr_off"], queries=rq["queries"][:2], tasks=rq["tasks"][:2], ranges=rq["ranges"][:2])

    def refused(why, **change):
        with pytest.raises(RuntimeError, match=why):
            blocks.hsp_tasks(eng, **dict(few, **change))
    blocks.hsp_tasks(eng, **few)
    refused("hash_slots is not a power of two", hash_slots=1000)
    refused("hit_cap is not a power of two", hit_cap=3000)
    refused("LDS exceeds", hit_cap=1 << 16)
    t = rq["tasks"][0]
    refused("outside its chromosome", tasks=[(0, t[1], int(rq["chr_off"][t[1] + 1] - rq["chr_off"][t[1]]) - 10, 11, 0)])
    refused("left / right / tlen outside the query", ranges=[(0, len(rq["queries"][0]) + 1), rq["ranges"][1]])
    refused("left / right / tlen outside the query", tlen=[len(rq["queries"][0]) + 1, 5])
    bad = rq["queries"][0].copy()
    bad[-1] = rq["model"].mtx_rows
    refused("a query code at or above mtx_rows", queries=[bad, rq["queries"][1]])
    from spaln_amd import abi
    odd = abi.WilipModel.from_buffer_copy(rq["model"])
    odd.level[0].bitpat_len = odd.level[0].width + 1
    refused("pattern's length differs from width", model=odd)
