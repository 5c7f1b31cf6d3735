"""One process of tests/test_gpu_seed_batch.py's launch-path checks (the engine reads its switches once per process): the round-edge,
tile-edge and list-length inputs of tests/seed_batch_inputs.py end to end against the oracle.  usage: python tests/seed_batch_child.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ["TELR_DEBUG"] = "1"

import torch  # noqa: E402,F401  (its HIP runtime first, as in tests/conftest.py)

from telr_amd.aligner import Engine  # noqa: E402
from telr_amd.presets import preset  # noqa: E402
import seed_batch_inputs as I  # noqa: E402
from test_gpu_parity import compare_all  # noqa: E402


def main():
    eng = Engine(0)
    # (several ranges: the stage captures hold the last range only -- records, CIGARs and counters are compared)
    stages = "TELR_BATCH_KBP" not in os.environ
    io, mo = preset("map-ont")
    targets, queries, counts = I.count_queries()
    assert counts[:-1] == list(I.COUNTS)
    _, oref = compare_all(eng, targets, queries, io, mo, stages=stages)
    assert oref["counters"]["minimizers"] == sum(counts)
    targets, queries, _ = I.tile_queries()
    compare_all(eng, targets, queries, io, mo, stages=stages)
    targets, queries, _ = I.family_case()
    io, mo = I.family_opts(7)
    compare_all(eng, ["".join(targets)], queries, io, mo, stages=stages)
    print("seed batch child ok")


if __name__ == "__main__":
    main()
