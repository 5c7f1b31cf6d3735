"""One process of tests/test_gpu_sketch_edges.py's switch checks (the engine reads TELR_AB once per process): the index comparison
of every case of tests/sketch_edges.py against the plain reference, one line per case.
usage: TELR_AB=sketch64 | index_sort_lib python tests/sketch_child.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ["TELR_DEBUG"] = "1"

import torch  # noqa: E402,F401  (its HIP runtime first, as in tests/conftest.py)

from telr_amd.aligner import Engine  # noqa: E402
import sketch_edges as se  # noqa: E402


def main():
    eng = Engine(0)
    n = 0
    for case in se.cases():
        n_mz, n_ent = se.check_index(eng, case, se.reference(case))
        print("%s: %d minimizers, %d entries ok" % (case[0], n_mz, n_ent), flush=True)
        n += 1
    print("sketch edges ok: %d cases" % n)


if __name__ == "__main__":
    main()
