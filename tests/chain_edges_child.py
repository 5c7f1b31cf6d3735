"""One process of tests/test_gpu_chain_edges.py's launch-path checks (the engine reads TELR_AB and TELR_CHAIN_DENSE once per process):
telr_debug_chain on every case of tests/chain_edges.py except mw_default, as built (the island launch unless TELR_AB=no_islands) and
padded with empty queries to CHAIN_ISL_NQ + 1 (one wave per query, k_chain_mw beside it under small thresholds), against the
oracle's tap, exactly.  Before each call a call of the same shape with an answer that differs at every anchor goes through the tap
(chain_edges.poison_input: the tap's device buffers outlive a call).  Every case is run; the ones that differ are listed before
the process fails.
usage: python tests/chain_edges_child.py [--mw-default]       (with the two mw_default cases)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (its HIP runtime first, as in tests/conftest.py)

from telr_amd.aligner import Engine  # noqa: E402
import chain_edges as E  # noqa: E402


def main():
    eng = Engine(0)
    bad, n = [], 0
    for case in E.cases():
        if case["name"].startswith("mw_default") and "--mw-default" not in sys.argv[1:]:
            continue
        ef, ep = E.oracle_out(case)
        for nq in (None, E.CHAIN_ISL_NQ + 1):
            keys, off = E.call_input(case, nq)
            pk, s = E.poison_input(case, off)
            f, p = eng.debug_chain(pk, off, case["mo"])
            if not (np.all(f == s) and np.all(p == -1)):
                bad.append("%s (nq %d): the poisoning call" % (case["name"], len(off) - 1))
            f, p = eng.debug_chain(keys, off, case["mo"])
            n += 1
            if not (f.dtype == ef.dtype and p.dtype == ep.dtype and np.array_equal(f, ef) and np.array_equal(p, ep)):
                w = np.flatnonzero((f != ef) | (p != ep))
                bad.append("%s (nq %d): %d anchors differ, the first at %d: f %d p %d, oracle f %d p %d"
                           % (case["name"], len(off) - 1, len(w), w[0], f[w[0]], p[w[0]], ef[w[0]], ep[w[0]]))
    if bad:
        print("\n".join(bad))
        print("chain edges child: %d of %d calls differ" % (len(bad), n))
        sys.exit(3)
    print("chain edges child ok (%d calls)" % n)


if __name__ == "__main__":
    main()
