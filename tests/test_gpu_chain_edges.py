"""The default chaining stage on the device -- chain_dispatch: the push loop d_chain_run<R>, the lazy far look-back
d_chain_run_lazy<R>, the R-wave ring d_chain_run_mw<R> and the island launch (k_isl_heads, k_isl_fill, k_chain_isl), each for R = 1, 2,
4 and SKIP on and off -- through the engine's tap telr_debug_chain on the hand-built lists of tests/chain_edges.py.  Every comparison
is exact (int32 arrays, no tolerance) against the oracle's tap tor_debug_chain; tests/test_chain_edges_ref.py checks on the CPU that
the oracle's tap is right and that each case reaches the edge it is built for.  Before every call under test a call of the same
shape whose answer differs at every anchor (chain_edges.poison_input) goes through the tap, whose device buffers outlive a call: an
anchor that a launch leaves unwritten, or a copy that does not wait for the second stream, cannot come back right.  In process every
case runs in two layouts: as built (at most CHAIN_ISL_NQ queries: the island launch) and padded with empty queries to
CHAIN_ISL_NQ + 1 (one wave per query, with mw_default k_chain_mw beside it).  The loops that the dispatch would not choose by itself run in child processes, one per setting of
the switches (tests/chain_edges_child.py)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import chain_edges as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in E.cases()]


def _same(engine, case, nq, what):
    keys, off = E.call_input(case, nq)
    ef, ep = E.oracle_out(case)
    # the tap's device buffers outlive a call: fill them with an answer that is wrong at every anchor first
    pk, s = E.poison_input(case, off)
    f, p = engine.debug_chain(pk, off, case["mo"])
    assert np.all(f == s) and np.all(p == -1), "%s: the poisoning call, %s" % (case["name"], what)
    t0 = time.perf_counter()
    f, p = engine.debug_chain(keys, off, case["mo"])
    dt = time.perf_counter() - t0
    assert f.dtype == np.int32 and p.dtype == np.int32
    np.testing.assert_array_equal(f, ef, err_msg="%s: f, %s" % (case["name"], what))
    np.testing.assert_array_equal(p, ep, err_msg="%s: p, %s" % (case["name"], what))
    return dt


@pytest.mark.parametrize("name", NAMES)
def test_engine_tap_equals_oracle_tap(engine, name):
    case = E.case_named(name)
    assert len(case["lists"]) <= E.CHAIN_ISL_NQ
    a = _same(engine, case, None, "as built")
    b = _same(engine, case, E.CHAIN_ISL_NQ + 1, "padded to %d queries" % (E.CHAIN_ISL_NQ + 1))
    if name.startswith("mw_default"):
        print("%s: %.3f s as built, %.3f s padded (copies included)" % (name, a, b))


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("mixed_queries")])
def test_island_launch_threshold(engine, name):
    """nq == CHAIN_ISL_NQ: still island by island; one more: one wave per query"""
    case = E.case_named(name)
    _same(engine, case, E.CHAIN_ISL_NQ, "padded to %d queries" % E.CHAIN_ISL_NQ)
    _same(engine, case, E.CHAIN_ISL_NQ + 1, "padded to %d queries" % (E.CHAIN_ISL_NQ + 1))


# one loop everywhere, no second kernel, no islands, and small thresholds for d_chain_dense / k_chain_mw (every dense run of 128
# anchors and more: the push loop on the island path, the R-wave ring where the call has more than CHAIN_ISL_NQ queries)
PATHS = [
    {"TELR_AB": "chain_push"},
    {"TELR_AB": "chain_lazy"},
    {"TELR_AB": "chain_no_mw", "--mw-default": ""},                   # (with mw_default: the one run that k_chain_mw takes by default)
    {"TELR_AB": "chain_no_mw", "TELR_CHAIN_DENSE": "128,300,128"},    # k_chain takes the dense runs of 128 anchors and more itself
    {"TELR_AB": "no_islands"},
    {"TELR_CHAIN_DENSE": "128,300,128"},
    {"TELR_AB": "no_islands", "TELR_CHAIN_DENSE": "128,300,128"},
]


@pytest.mark.parametrize("env", PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()).rstrip("="))
def test_launch_paths(env):
    e = dict(os.environ)
    e.pop("TELR_AB", None); e.pop("TELR_CHAIN_DENSE", None)
    e.update((k, v) for k, v in env.items() if not k.startswith("--"))
    args = [k for k in env if k.startswith("--")]           # (the child's own arguments)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_edges_child.py")] + args, cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "chain edges child ok" in out, out[-6000:]
