"""One process of tests/test_gpu_chain_skip.py's launch-path checks (the engine reads its switches once per process): minimap2's
chaining scan (TELR_MF_CHAIN_SKIP) end to end against the oracle on hard-genome reads, and telr_debug_chain on every hand-built
anchor list against the restatement.  usage: python tests/chain_skip_child.py [n_reads]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ["TELR_DEBUG"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (its HIP runtime first, as in tests/conftest.py)

from telr_amd.aligner import Engine  # noqa: E402
from telr_amd.presets import preset  # noqa: E402
import chain_scan_ref as R  # noqa: E402
import chain_skip_inputs as I  # noqa: E402
from test_gpu_parity import compare_all  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    eng = Engine(0)
    io, mo = preset("map-ont", chain_skip=True)
    ref = [bytes(c).decode() for c in I.hard_genome()["ref"]]
    # (several ranges: the stage captures hold the last range only -- records, CIGARs and counters are compared)
    compare_all(eng, ref, I.hard_ont_reads()[:n], io, mo, stages="TELR_BATCH_KBP" not in os.environ)
    hm = R.hand_opts()
    for name, lists, _ in R.hand_cases():
        keys, off = R.concat_lists(lists)
        f, p = eng.debug_chain(keys, off, hm)
        ef, ep = R.chain_scan_all(keys, off, hm)
        assert np.array_equal(f, ef) and np.array_equal(p, ep), name
    print("chain skip child ok")


if __name__ == "__main__":
    main()
