"""The restatement of SrchBlk::finds (tests/finds_restate.py) held to the program: for every query of every -pw run of the fixtures
(-M4 -pw, -LS -M2 -pw: with -pw the program prints a record for every candidate finds returned) the restatement's candidate set
is the set of database names the program printed.  This is what makes the restatement a checker."""
import pytest

from tests import aa_fixture as af
from tests import finds_restate as fr


@pytest.mark.parametrize("name", af.SETS)
@pytest.mark.parametrize("run", list(af.PW_RUNS))
def test_candidate_sets_are_the_programs(name, run):
    doc = af.search(name)
    max_out, local = af.PW_RUNS[run]
    ix = af.index(name, max_out, local)
    names = [d["name"] for d in doc["db"]]
    printed = doc["runs"][run]["o4"]
    # the program refuses a query below MinQuery = 2 Ktuple + Nshift before it calls finds (src/spaln.cc:1087, 1104)
    min_query = 2 * ix.patterns[0][0] + ix.nshift
    assert set(doc["refused"]) == {q["name"] for q in doc["queries"] if len(q["seq"]) < min_query}
    n_searched = 0
    for q in doc["queries"]:
        r = fr.finds(ix, af.encode(q["seq"]))
        if len(q["seq"]) - (ix.nshift + ix.patterns[0][1]) < 1:
            assert r["ret"] == fr.ERROR and r["flags"] == fr.SHORT and q["name"] in doc["refused"], q
        if q["name"] in doc["refused"]:
            assert q["name"] not in printed
            continue
        got = {names[c] for c in r["cands"]}
        want = {rec["b"] for rec in printed.get(q["name"], [])}
        assert got == want and len(r["cands"]) == len(printed.get(q["name"], [])), (q["name"], q["cls"], sorted(got), sorted(want))
        assert all(c >= 0 for c in r["cands"])
        n_searched += 1
    assert n_searched >= 30


@pytest.mark.parametrize("name", af.SETS)
def test_planted_sources_come_first(name):
    """the block of the planted source has the highest score of the m15 / frag / xx queries, as the program's first record says"""
    doc = af.search(name)
    ix = af.index(name, 1)
    first = doc["runs"]["default"]["o4"]
    for q in doc["queries"]:
        if q["cls"] in ("m15", "frag", "xx") and q["name"] in first:
            r = fr.finds(ix, af.encode(q["seq"]))
            assert doc["db"][r["cands"][0]]["name"] == first[q["name"]][0]["b"], q["name"]
