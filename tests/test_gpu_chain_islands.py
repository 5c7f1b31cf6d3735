"""The island walk of k_chain (kernels.hip.h: THE ISLAND WALK) on the hand-built lists of tests/chain_island_cases.py: windows of
small islands chained side by side, islands that do not fit a window handed to the loops for whole runs.  Every comparison is exact
(int32 arrays, no tolerance) of f and p for every anchor, telr_debug_chain against the oracle's tap tor_debug_chain.

The cases have a few queries each, for which the dispatch would choose the island launch, so the kernel with one wave per query runs
in child processes under TELR_AB=no_islands (the engine reads its switches once per process): the walk itself, the walk with small
thresholds for d_chain_dense (a dense serial island takes the push loop between two packed windows), and TELR_AB=chain_no_pack, which
pins the loops for whole lists at the same island edges.  One more test maps the bundled 38-kb fixture with and without the walk and
compares records and CIGARs bit for bit.

The first tests need no GPU: each case has the island sizes and takes the walk its name claims (numpy on the keys), the oracle's
tap equals the restatement in Python of tests/chain_edges.py on every case, and island by island the tap gives what it gives on
whole lists."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_edges as E
import chain_island_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in C.cases()]
BY = {c["name"]: c for c in C.cases()}
H64 = [n for n in NAMES if n.endswith("_h64_s0")]


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU


@pytest.mark.parametrize("name", NAMES)
def test_case_has_the_islands_it_claims(name):
    case = BY[name]
    assert case["mo"].max_gap == C.MAX_GAP
    assert 1 <= len(case["lists"]) <= 3 and all(len(L) <= 420 for L in case["lists"])
    assert len(case["sizes"]) == len(case["walk"]) == len(case["lists"])
    for L, sizes, walk in zip(case["lists"], case["sizes"], case["walk"]):
        assert C.sizes_of(L, case["mo"].max_gap) == sizes, name
        assert C.walk_of(sizes) == walk, name
        # the walk covers the list once, every packed window holds whole islands of at most 64 anchors (63 where the list goes
        # on), and a serial island is one island that fills a window
        starts = set(np.concatenate(([0], np.cumsum(sizes))).tolist())
        pos = 0
        for kind, at, n in walk:
            assert at == pos and at in starts and at + n in starts and n >= 1
            inside = [s for s, b in zip(sizes, np.cumsum(sizes)) if at < b <= at + n]
            if kind == "packed":
                assert n <= 64 and sum(inside) == n and (n <= 63 or at + n == len(L))
            else:
                assert inside == [n] and n >= 64 and at + n <= len(L)
            pos += n
        assert pos == len(L)


def test_the_named_shapes_are_there():
    """what the case names say, on the h64_s0 instances (the lists are the same under every setting)"""
    by = {c["name"][:-len("_h64_s0")]: c for c in C.cases() if c["name"].endswith("_h64_s0")}
    every = set(s for c in by.values() for sizes in c["sizes"] for s in sizes)
    assert {1, 2, 16, 17, 63, 64, 65} <= every
    assert by["singletons_64"]["sizes"] == [[1] * 64] and by["singletons_64"]["walk"] == [[("packed", 0, 64)]]
    # a head at lane 63 of a window that is not the list's last
    for n in ("size_63_head_at_lane_63", "singletons_head_at_lane_63"):
        assert by[n]["walk"][0][0] == ("packed", 0, 63) and len(by[n]["lists"][0]) > 64
    # the list ends at lanes 1, 63 and 64 of its last window
    ends = {}
    for name, c in by.items():
        for w in c["walk"]:
            if w and w[-1][0] == "packed":
                ends.setdefault(w[-1][2], []).append(name)
    assert {1, 63, 64} <= set(ends)
    # an island across a window boundary: below 64 anchors packed in the next window, above it serial
    assert by["straddle_below_64"]["walk"] == [[("packed", 0, 40), ("packed", 40, 43)]] and by["straddle_below_64"]["sizes"][0][1] == 40
    assert ("serial", 40, 70) in by["straddle_above_64"]["walk"][0]
    # packed directly before and directly after serial, and serial directly before and after packed
    kinds = lambda n: [w[0] for w in by[n]["walk"][0]]
    assert kinds("packed_serial_packed") == ["packed", "serial", "packed"]
    assert kinds("serial_packed_serial") == ["serial", "packed", "serial", "serial", "packed"]
    assert kinds("dense_serial_island") == ["packed", "serial", "packed"]
    # an empty query and one of a single anchor
    assert [len(L) for L in by["empty_and_single_anchor"]["lists"]] == [0, 82, 1]
    # the ties sit inside packed windows, once in a list's third window
    assert by["tie_in_packed_island_late"]["walk"][0][-1] == ("packed", 83, 54)
    # the random lists take both paths
    k = set(w[0] for walk in by["random_islands"]["walk"] for w in walk)
    assert k == {"packed", "serial"}
    for H, skip in E.SETTINGS:
        assert sum(n.endswith("_h%d_s%d" % (H, skip)) for n in NAMES) == len(by)


@pytest.mark.parametrize("name", H64 + [n for n in NAMES if n.startswith(("tie_", "random_", "dense_")) and n not in H64])
def test_oracle_tap_on_the_cases(name):
    """the reference of the GPU tests: equal to the restatement, the case's edge reached, and the same island by island (p shifted
    by the island's start) as on whole lists"""
    from oracle import binding as ob
    case = BY[name]
    keys, off = E.call_input(case)
    f, p = E.oracle_out(case)
    rf, rp = E.chain_default_all(keys, off, case["mo"])
    np.testing.assert_array_equal(f, rf)
    np.testing.assert_array_equal(p, rp)
    case["reach"](*E.split(f, p, off))
    # island by island: every island a query of its own
    ioff, start = [0], []
    for q, sizes in enumerate(case["sizes"]):
        at = 0
        for s in sizes:
            start.append(at)
            ioff.append(ioff[-1] + s)
            at += s
    assert ioff[-1] == len(keys)
    fi, pi = ob.debug_chain(keys, np.asarray(ioff, np.int32), case["mo"])
    shift = np.repeat(np.asarray(start, np.int32), np.diff(ioff))
    np.testing.assert_array_equal(fi, f)
    np.testing.assert_array_equal(np.where(pi >= 0, pi + shift, -1), p)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU


def _start(env, args):
    e = dict(os.environ)
    e.pop("TELR_AB", None); e.pop("TELR_CHAIN_DENSE", None)
    e.update(env)
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "chain_island_cases.py")] + args, cwd=ROOT, env=e,
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def _finish(p):
    try:
        out = p.communicate(timeout=600)[0]
    except subprocess.TimeoutExpired:
        p.kill()
        out = p.communicate()[0]
    return p.returncode, out.decode()


def _child(env, args):
    return _finish(_start(env, args))


PATHS = [
    {"TELR_AB": "no_islands"},                                                      # the walk
    {"TELR_AB": "no_islands,chain_no_mw", "TELR_CHAIN_DENSE": "128,300,128"},       # the walk; dense serial islands take the push loop
    {"TELR_AB": "no_islands", "TELR_CHAIN_DENSE": "128,300,128"},                   # k_chain_mw beside it for the lists dense as a whole
    {"TELR_AB": "no_islands,chain_no_pack"},                                        # whole lists: the loops from before the walk
    {},                                                                             # the island launch (k_chain_isl)
]


@pytest.mark.gpu
@pytest.mark.parametrize("env", PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_walk_equals_oracle_tap(env):
    rc, out = _child(env, [])
    assert rc == 0 and "chain islands child ok (%d calls)" % len(NAMES) in out, out[-6000:]


@pytest.mark.gpu
def test_fixture_maps_the_same_with_and_without_the_walk(tmp_path):
    """the 38-kb fixture reads under map-ont and ngmlr-ont: one wave per query with the walk, without it, and the default dispatch"""
    arms = (("walk", {"TELR_AB": "no_islands"}), ("no_pack", {"TELR_AB": "no_islands,chain_no_pack"}),
            ("default", {}), ("default_no_pack", {"TELR_AB": "chain_no_pack"}))
    procs = [(tag, str(tmp_path / (tag + ".npz")), _start(env, ["--map", str(tmp_path / (tag + ".npz"))])) for tag, env in arms]      # (side by side)
    outs = {}
    for tag, path, p in procs:
        rc, out = _finish(p)
        assert rc == 0 and "chain islands map ok" in out, out[-6000:]
        outs[tag] = np.load(path)
    ref = outs["no_pack"]
    assert len(ref["map-ont_alns"]) > 0 and len(ref["ngmlr-ont_alns"]) > 0
    for tag in ("walk", "default", "default_no_pack"):
        for k in ref.files:
            assert outs[tag][k].dtype == ref[k].dtype and np.array_equal(outs[tag][k], ref[k]), "%s: %s" % (tag, k)
