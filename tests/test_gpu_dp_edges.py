"""The engine's DP classes at their routing edges, problem by problem against the oracle's banded DP (tests/dp_edges.py):
score, end cell, CIGAR, retry flag, matching bases and the trace-back offset of every problem, the class every problem takes
against a restatement of the routing (d_dp_class, the N rule, the nibble cell's move to class 14), and every class 0-24
reached at its widest band and at its step bound.  The switches that change the trace-back format or the wave split run the
same set in a process of their own (they are read once per process)."""
import os
import subprocess
import sys

import pytest

import dp_edges as de
from telr_amd import _lib
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def edge_run(engine):
    return de.run_all(engine)


def test_engine_equals_oracle_at_class_edges(edge_run):
    total, bad, _, per_set = edge_run
    for name, (n, cls) in per_set.items():
        print("%-16s %6d problems, classes %s" % (name, n, " ".join(map(str, cls))))
    assert total > 40000
    assert not bad, "%d of %d problems differ:\n%s" % (len(bad), total, "\n".join(bad[:40]))


def test_every_class_reached_at_its_edges(edge_run):
    _, _, cov, _ = edge_run
    at_d = {(c, D) for _, c, D, _, _ in cov}
    for c, D in de.UPPER_D.items():
        assert (c, D) in at_d, "class %d never ran a band of %d diagonals" % (c, D)
    at_l = {(c, tag) for _, c, _, _, tag in cov}
    for c, lim in de.STEP_LIMIT.items():
        assert (c, "L:%s:0" % lim) in at_l, "class %d never ran a problem of exactly %s steps" % (c, lim)
    # the nibble cell's move, and a packed class left for an N, both happened
    assert any(c == 14 and tag.startswith("L:tb4_steps:1") for _, c, _, _, tag in cov)
    assert any(c in (5, 6, 7, 8, 9) and tag == "N" and D <= 128 for _, c, D, _, tag in cov)


def test_tap_refuses_what_the_map_path_cannot_produce(engine):
    mo = preset("map-ont")[1]
    q = engine.seqset([b"ACGT" * 50])
    t = engine.seqset([b"ACGT" * 50])
    good = (0, 0, 0, 0, 100, 100, -4, 4, 0, 1, 1, 0)
    r = engine.debug_dp(q, t, mo, [good])
    assert r["score"][0] == 200 and r["cls"][0] == 17
    for bad in ((0, 0, 0, 0, 100, 100, -3, 4, 0, 1, 1, 0),       # odd dlo
                (0, 150, 0, 0, 100, 100, -4, 4, 0, 1, 1, 0),     # window past the end
                (0, 50, 0, 0, 100, 100, -4, 4, 0, -1, 1, 0),     # reverse window before the start
                (0, 0, 0, 0, 100, 100, -6, 4, 0, 1, 1, 0),       # lopsided fill band
                (0, 0, 0, 0, 100, 100, -4, 4, 4, 1, 1, 0),       # kind 4
                (0, 0, 0, 0, 100, 100, -4, 4, 3, 1, 1, 0),       # kind 3 with a band kind 0 takes
                (0, 0, 0, 0, 100, 100, -4, 4, 1, 1, 1, 0),       # extension with a fill band
                (0, 0, 0, 0, 100, 100, -32, 31, 5, 1, 1, 0)):    # long-gap fill of a short gap
        with pytest.raises(_lib.TelrError) as ei:
            engine.debug_dp(q, t, mo, [good, bad])
        assert "invalid argument" in str(ei.value) and "problem 1" in str(ei.value), bad
    m2 = mo.copy()
    m2.q2 = mo.q - 1            # the option checks of telr_map
    with pytest.raises(_lib.TelrError):
        engine.debug_dp(q, t, m2, [good])


@pytest.mark.parametrize("ab", ["tb8", "no_tag8", "tb_one_launch", "dp_one_wave"])
def test_switch_keeps_dp_edges(ab):
    e = dict(os.environ)
    e["TELR_AB"] = ab
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dp_edges.py")], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0 and "dp edges ok" in out, out[-4000:]
