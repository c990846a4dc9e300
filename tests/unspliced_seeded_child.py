"""One seeded call on one option set of the fixtures in a process of its own (tests/test_gpu_unspliced_seeded.py starts it with
and without SPDP_B_THIN=0: the library reads the switch from the environment).  Prints one JSON line: per pair score and
corners, and the call's counters.

    python -m tests.unspliced_seeded_child <fixture file> <run index>
"""
import json
import sys

from spaln_amd import defaults, engine
from tests import unspliced_seeded_cases as usc


def main() -> int:
    name, k = sys.argv[1], int(sys.argv[2])
    sc, up, sp, ps, recs, opts = usc.problems(name, k)
    eng = engine.Engine(0)
    alns = eng.align_b_seeded(sc, up, sp, ps, model=defaults.wilip_model_b())
    stats = eng.seeded_stats_b()
    eng.close()
    print(json.dumps(dict(alignments=[[s, skl.tolist()] for s, skl in alns], stats=stats)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
