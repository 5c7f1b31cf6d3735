"""One process of tests/test_gpu_seed_rescue.py's launch-path checks (the engine reads its switches once per process):
TELR_MF_SEED_RESCUE end to end against the oracle on the two-family queries plus the over-size query (tests/seed_rescue_inputs.py)
with map-ont and ngmlr-ont, and on the edge inputs.  usage: python tests/seed_rescue_child.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ["TELR_DEBUG"] = "1"

import torch  # noqa: E402,F401  (its HIP runtime first, as in tests/conftest.py)

from telr_amd.aligner import Engine  # noqa: E402
from telr_amd.presets import preset  # noqa: E402
from telr_amd._abi import MF_SEED_RESCUE  # noqa: E402
import seed_rescue_inputs as I  # noqa: E402
from test_gpu_parity import compare_all  # noqa: E402


def main():
    eng = Engine(0)
    # (several ranges: the stage captures hold the last range only -- records, CIGARs and counters are compared)
    stages = "TELR_BATCH_KBP" not in os.environ
    targets, queries = I.two_family()
    queries = list(queries) + [I.over_query()]          # the last query holds more than SEGSORT_CAP anchors with map-ont
    for pname in ("map-ont", "ngmlr-ont"):
        io, mo = preset(pname, seed_rescue=True)
        _, oref = compare_all(eng, targets, queries, io, mo, stages=stages)
        if pname == "map-ont":
            assert oref["anchor_off"][-1] - oref["anchor_off"][-2] > 20480
            assert eng.counters()["over_queries"] > 0
    targets, io, mo, _, cases = I.edge_cases()
    mo = mo.copy(); mo.flags |= MF_SEED_RESCUE
    compare_all(eng, targets, [c["query"] for c in cases], io, mo, stages=stages)
    print("seed rescue child ok")


if __name__ == "__main__":
    main()
