"""One process of tests/test_gpu_vote_edges.py's launch-path checks (the engine reads its switches once per process): the stash,
chunk, trip, geometry, sub-read cap and tier inputs of tests/vote_inputs.py end to end against the oracle.
usage: python tests/vote_child.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ["TELR_DEBUG"] = "1"

import torch  # noqa: E402,F401  (its HIP runtime first, as in tests/conftest.py)

from telr_amd.aligner import Engine  # noqa: E402
import vote_inputs as I  # noqa: E402
from test_gpu_vote_edges import run_case  # noqa: E402

CASES = ("stash", "stash_chunks", "chunk127", "chunk128", "chunk129", "chunk300", "trip", "geometry", "subcap",
         "tiers_plain", "tiers_voted", "tiers_plain_fit", "tiers_voted_fit")


def main():
    eng = Engine(0)
    # (several ranges: the stage captures hold the last range only -- records, CIGARs and counters are compared)
    ranges = "TELR_BATCH_KBP" in os.environ
    cases = I.all_cases()
    for name in CASES:
        c = cases[name]()
        if ranges:
            plan = Engine.map_plan([len(q) for q in c.queries], vote=c.mo.vote_len > 0, debug=1)
            assert len(plan[2]) > 1, (name, plan)
        run_case(eng, c, stages=not ranges)
    print("vote child ok")


if __name__ == "__main__":
    main()
