"""The two consensus kernels at their caps and edges (tests/consensus_edges.py): every hand-built case through telr_poa_build
(k_poa_window) and telr_consensus_build (k_pile_count / k_pile_call) against the oracle's tor_poa / tor_consensus, string for
string, at min_depth 1, 3 and the case's own boundary; every POA case must reach the edge it is aimed at (tor_poa_stats).
The one switch that changes the consensus path -- TELR_AB=scan_lib, the library scan of the pile-up's output offsets -- runs the
same set in a process of its own (switches are read once per process).  Malformed records never reach a kernel here: the
host check both builds run first is tested in tests/test_consensus_reference.py."""
import os
import subprocess
import sys

import pytest

import consensus_edges as ce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ce.cases()


def test_kernels_equal_the_oracle_at_their_edges(engine, cases):
    # (a comparison only means something where the case reaches its edge: the cases are checked first, on the same set)
    missed = [(c["name"], c["reach"](ce.oracle_stats(c), c)) for c in cases if c["poa"] and c["reach"]]
    assert not [m for m in missed if m[1]], missed
    n, bad = ce.run_all(engine, cases)
    assert n > 100
    assert not bad, "%d of %d comparisons differ:\n%s" % (len(bad), n, "\n".join(bad[:40]))


@pytest.mark.parametrize("ab", ["scan_lib"])
def test_switches_keep_the_edges(ab):
    env = dict(os.environ, TELR_AB=ab)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "consensus_edges.py"), "--engine"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "consensus edges ok" in p.stdout
