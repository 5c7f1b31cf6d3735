"""The three trace-back walks at their path-shaped edges (tests/tb_paths.py): planted paths through the engine's DP pass against
the oracle's banded DP, problem by problem -- score, end cell, CIGAR, retry flag, mlen against the CIGAR, spans, tb_off
alignment and the class taken.  One engine run of all groups, one test per family; the switches that change the trace-back
format run the same groups in a process of their own."""
import os
import subprocess
import sys
from collections import Counter

import pytest

import tb_paths as tp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def path_run(engine):
    res = tp.run_all(engine)
    print("\n".join(tp.summary(res)))
    return res


def _clean(res, fam, least):
    n, bad, cov = res[fam]
    print("\n".join(tp.summary({fam: res[fam]})))
    assert n >= least, n
    assert not bad, "%d of %d problems differ:\n%s" % (len(bad), n, "\n".join(bad[:40]))
    return cov


def test_packed_fills_walk_planted_paths(path_run):
    cov = _clean(path_run, "A", 12000)
    b = tp.build()
    assert {c for _, _, c, _, _, _ in cov} == set(tp.A_CLASSES)
    # the encoding every wave took, by the library's own limits: nibble, tagged and plain-flag waves all ran, and the convex cell
    encs = {}
    for g in b.groups:
        if g.fam == "A":
            cs = [(c, st) for s, name, c, _, st, _ in cov if s == g.set and name == g.name]
            for c, e in tp.wave_cells(b.sets[g.set], b.lims[g.set], cs).items():
                encs.setdefault(c, set()).update(e)
    print("encodings per class:", {c: sorted(e) for c, e in sorted(encs.items())})
    for c in tp.A_CLASSES:
        assert encs[c] == ({"nibble", "cx"} if c in tp.NIBBLE_BIT else {"tag8", "plain", "cx"}), (c, encs[c])


def test_wave_walk_takes_planted_paths(path_run):
    cov = _clean(path_run, "B", 200)
    assert {c for _, _, c, _, _, _ in cov} == {19, 20, 21, 7, 8, 9, 1, 2, 4}


def test_lane_walk_takes_planted_paths(path_run):
    cov = _clean(path_run, "C", 600)
    assert {c for _, _, c, _, _, _ in cov} == {18, 23, 24, 0, 5, 6}


def test_tail_class_lists_on_both_sides_of_the_lane_walk_switch(path_run):
    cov = _clean(path_run, "D", 6 * tp.TBW_MAX + 3)
    per = Counter((name, c) for _, name, c, _, _, _ in cov)
    print(dict(per))
    for c in (19, 7, 1):
        for n in (tp.TBW_MAX, tp.TBW_MAX + 1):
            assert per[("%d of class %d" % (n, c), c)] == n, (c, n)


@pytest.mark.parametrize("ab", ["tb8", "no_tag8", "tb_one_launch"])
def test_switch_keeps_planted_paths(ab):
    e = dict(os.environ)
    e["TELR_AB"] = ab
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tb_paths_child.py")], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    print(out[-2000:])
    assert p.returncode == 0 and "tb paths ok" in out, out[-4000:]
