"""Map and align end to end on queries as a FASTA file of mRNAs and ESTs holds them (tools/e2e_q7.py --tails): poly-A tails on a
third of the queries, antisense reads with poly-T heads on another third, A's planted in the genome behind the last exon of every
third gene.  `spaln -Q7 -O4` of the compiled reference (oracle/_ref/spaln: test infrastructure, prebuilt) does what it does to
every cDNA first, PolyA::rmpolyA; the library goes through spdp_map_align_s_prep / _multi_prep.  The exon tables must be the
program's, the records of the device scan those of spdp_polya_scan_host, and the data must be able to tell a trimmed run from
an untrimmed one: the entry without the preparation differs from the program on at least one tailed query."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [["--ori", "1"], ["--ori", "3"], ["--max-out", "4", "--paralogs"]],
                         ids=["ori1", "ori3", "M4-paralogs"])
def test_tailed_queries_give_the_programs_exon_tables(extra):
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "spaln")):
        pytest.skip("oracle/_ref/spaln is not built")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e_q7.py"), "--tails", "--queries", "300", "--genes", "60"] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-400:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps({k: d.get(k) for k in ("reference_aligned", "library_aligned", "identical_exon_tables", "tails", "tail_records_equal_host",
                                            "untrimmed_differs")}))
    assert d["reference_aligned"] == 300 and d["library_aligned"] == 300, d
    assert d["identical_exon_tables"] == 300, (d, r.stderr[-600:])
    assert d["tail_records_equal_host"] is True
    assert d["untrimmed_differs"] >= 1
    assert d["tails"]["none"] == 100 and d["tails"]["a_tail"] + d["tails"]["t_head"] == 200
    assert d["tails"]["t_head"] == (100 if extra == ["--ori", "3"] else 0)
