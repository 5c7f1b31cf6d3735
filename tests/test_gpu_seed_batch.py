"""The seeding routine with several loads in flight per thread (d_seed_query<1>, the key writer of k_seed<1> and of the fused sort:
SEED_PROBE_BATCH minimizers per thread and round, an occurrence list read four occurrences at a time): engine == oracle bit for bit
end to end (q_aoff, the sorted keys, f, p, chains, every record field, every CIGAR, the counters: compare_all of
tests/test_gpu_parity.py) on inputs that sit on the edges of the groups (tests/seed_batch_inputs.py).  The probes (d_seed_query<0>)
take one minimizer a round; the same inputs hold them to the oracle.  Every test first asserts on the CPU that its input is what it claims."""
import os
import subprocess
import sys

import numpy as np
import pytest

from telr_amd.presets import preset
from telr_amd._abi import MF_PER_TARGET, MF_SEED_RESCUE
import seed_batch_inputs as I
import sketch_edges as SE
from test_gpu_parity import compare_all

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_edges(engine):
    """minimizer counts 0, 1, 255, 256, 257, 256U - 1, 256U, 256U + 1, 512U + 3 (U = 4) and a query of the 1,024-thread sort tier"""
    targets, queries, counts = I.count_queries()
    assert [I.n_minimizers(q) for q in queries[:-1]] == list(I.COUNTS) == counts[:-1]
    io, mo = preset("map-ont")
    assert (io.k, io.w) == (I.K, I.W)
    _, oref = compare_all(engine, targets, queries, io, mo)
    assert oref["counters"]["minimizers"] == sum(counts)
    na = np.diff(oref["anchor_off"])
    assert 4096 < na[-1] <= 20480, na[-1]          # k_segsort<1024, 8 | 20>


@pytest.mark.parametrize("w", [I.W, 1])
def test_tile_edges(engine, w):
    """a thread's indices of one round in 1, 2, 3 and more sketch tiles, across an empty tile, and across more empty tiles than a
    round reads ahead.  w = 1 (every k-mer a minimizer) puts all four indices of a thread into one tile."""
    targets, queries, tiles = I.tile_queries(w)
    assert 2 not in tiles[1] and {1, 3} <= set(tiles[1].tolist())
    assert np.diff(np.unique(tiles[2])).max() - 1 > I.TILE_WIN
    seen = set().union(*[I.round_tile_counts(t) for t in tiles])
    assert ({(1, 1), (2, 2), (3, 3)} <= seen) if w == I.W else ({(4, 1), (4, 2)} <= seen)
    io, mo = preset("map-ont")
    io.w = w
    compare_all(engine, targets, queries, io, mo)


def _family_oracle(targets, queries, io, mo, qtarget=None):
    from oracle import binding as ob
    oix = ob.OracleIndex(list(targets), io)
    return oix, oix.map(list(queries), mo, qtarget=qtarget, debug=True)


@pytest.mark.parametrize("cutoff", [4, 7, 9])
def test_list_lengths(engine, cutoff):
    """occurrence lists of 1, 2, 3, 4, 5, 7, 8, 9 entries against a cut-off inside that range"""
    targets, queries, _ = I.family_case()
    targets = ["".join(targets)]
    io, mo = I.family_opts(cutoff)
    oix, o = _family_oracle(targets, queries, io, mo)
    assert oix.mid_occ(mo) == cutoff
    oh, _ = oix.dump()
    occ = [I.query_occurrences(oh, q) for q in queries]
    assert set(I.FAMILY_COPIES) <= set(np.concatenate(occ).tolist())
    # a query's anchors are the occurrences of its minimizers at or below the cut-off: the lists one above it yield none
    above = [n for n in I.FAMILY_COPIES if n > cutoff]
    for q, c in enumerate(occ):
        assert o["anchor_off"][q + 1] - o["anchor_off"][q] == int(c[c <= cutoff].sum())
    if above:
        assert any((c == above[0]).any() for c in occ)
    compare_all(engine, targets, queries, io, mo)


def test_probe_collisions(engine):
    """entries that share a home slot of the probe table: the second one is found by linear probing"""
    targets, queries, _ = I.count_queries()
    io, mo = preset("map-ont")
    gix = engine.index(targets, io)
    eh, _, _ = gix.debug_dump()
    home = I.home_slots(eh)
    slots, n = np.unique(home, return_counts=True)
    shared = set(slots[n >= 2].tolist())
    assert len(shared) >= 1
    collide = set(np.asarray(eh)[np.isin(home, list(shared))].tolist())
    qh = {x >> 8 for q in queries[2:6] for x, _ in SE.brute_minimizers(q, io.k, io.w)}
    assert len(qh & collide) >= 2
    compare_all(engine, targets, queries, io, mo)


def test_query_targets(engine):
    """per-query targets with -1 entries: the target's piece of a list by bisection, then the same expansion"""
    targets, queries, _ = I.family_case()
    io, mo = I.family_opts(7)
    qt = np.array([0, -1, 1, 2, -1, 0, 1, 2], np.int32)
    _, o = _family_oracle(targets, queries, io, mo, qtarget=qt)
    _, o0 = _family_oracle(targets, queries, io, mo)
    na, na0 = np.diff(o["anchor_off"]), np.diff(o0["anchor_off"])
    assert (na[qt < 0] == na0[qt < 0]).all() and (na[qt >= 0] < na0[qt >= 0]).any() and (na[qt >= 0] > 0).any()
    compare_all(engine, targets, queries, io, mo, qtarget=qt)


def test_per_target(engine):
    targets, queries, _ = I.family_case()
    io, mo = I.family_opts(4)
    on = mo.copy(); on.flags |= MF_PER_TARGET
    _, o = _family_oracle(targets, queries, io, on)
    _, o0 = _family_oracle(targets, queries, io, mo)
    # a list above the pooled cut-off whose pieces inside the targets are not: the per-target count keeps it
    assert (np.diff(o["anchor_off"]) > np.diff(o0["anchor_off"])).any()
    compare_all(engine, targets, queries, io, on)


def test_seed_rescue(engine):
    targets, queries, _ = I.family_case()
    targets = ["".join(targets)]
    io, mo = I.family_opts(4)
    on = mo.copy(); on.flags |= MF_SEED_RESCUE
    _, o = _family_oracle(targets, queries, io, on)
    _, o0 = _family_oracle(targets, queries, io, mo)
    assert (np.diff(o["anchor_off"]) > np.diff(o0["anchor_off"])).any()
    compare_all(engine, targets, queries, io, on)


# the launch paths that are read once per process: the two-step seeding (k_seed<1> writes the keys to memory), compacted
# minimizer arrays (no tile walk), and several ranges, also pipelined
PATHS = [
    {"TELR_AB": "seed_unfused"},
    {"TELR_AB": "mz_compact"},
    {"TELR_BATCH_KBP": "40"},
    {"TELR_BATCH_KBP": "40", "TELR_PIPELINE": "force"},
]


@pytest.mark.parametrize("env", PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_launch_paths(env):
    e = dict(os.environ); e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seed_batch_child.py")], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "seed batch child ok" in out, out[-3000:]
