"""Sub-read voting (k_vote_lookup, k_vote_qhits, k_seed_vote<T16>, k_vote_compact) and the anchor sort (segsort.hip.h) at their fixed
caps and alternative paths: engine == oracle bit for bit end to end (q_aoff, the sorted keys, f, p, chains, every record field, every
CIGAR, the counters: compare_all of tests/test_gpu_parity.py) on the inputs of tests/vote_inputs.py.  Every test first builds its
input, which asserts on the CPU that it reaches the edge it names (tests/test_vote_ref.py proves the same without a device and holds
the oracle to tests/vote_ref.py), then asserts that the case is not vacuous: voting removed hits and kept hits.

Which test stands on which side of a constant:
  VOTE_HCAP = 768         test_stash_cap: 767, 768 | 769, 4,138 hits in one sub-read; test_stash_cap_two_chunks beyond it in two chunks;
                          test_trips: 513 | 1,316
  VOTE_MZ = 128           test_chunk_cap[127], [128] | [129] (a second chunk of ONE minimizer), [300] (three chunks)
  the 512-hit trip        test_trips: chunks of 511, 512 | 513, 1,316 hits; list starts on hits 31, 32, 63, 64
  VOTE_SUBCAP = 512       test_sub_read_cap: 511, 512 | 513, 1,025 sub-reads
  VOTE_WAVES = 3          test_geometry: 1, 2, 3 | 4, 7 sub-reads (4: the first wave's prefetched second sub-read), empty sub-reads
  65,535 staged hits      test_counter_width: 65,535 | 65,536, all of them votes of one bin; test_wide_bin: one bin of 118,400 votes
  the 1,024-bin fold      test_threshold: bins 1023 and 0 as neighbours, two loci 32,768 bases apart in one bin
  segsort_tier_of         test_sort_tiers: 128 | 129, 512 | 513, 1,024 | 1,025, 2,048 | 2,049, 4,096 | 4,097, 8,192 | 8,193,
                          20,480 (SEGSORT_CAP) | 20,481, with 0, 1, 2, 3"""
import os
import subprocess
import sys

import numpy as np
import pytest

import vote_inputs as I
from test_gpu_parity import compare_all

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(engine, c, stages=True):
    """compare_all, then: voting removed at least one hit and kept at least one (the hits before voting by brute force on the CPU)"""
    _, oref = compare_all(engine, c.targets, c.queries, c.io, c.mo, stages=stages)
    if c.mo.vote_len > 0:
        ix = I.Index(c.targets, c.io)
        hits = sum(ix.hits(q) for q in c.queries)
        assert 0 < oref["counters"]["anchors"] < hits, (oref["counters"]["anchors"], hits)
    return oref


def test_stash_cap(engine):
    c = I.stash_case()
    assert c.facts["hits"][:6] == [767, 767, 768, 768, 769, 769] and c.facts["hits"][6] > 2000
    assert all(0 < k < h for k, h in zip(c.facts["kept"], c.facts["hits"]))
    oref = run_case(engine, c)
    assert np.diff(oref["anchor_off"]).tolist() == c.facts["kept"]


def test_stash_cap_two_chunks(engine):
    c = I.stash_chunks_case()
    assert min(c.facts["nmz"]) > I.VOTE_MZ and min(c.facts["hits"]) > I.VOTE_HCAP
    oref = run_case(engine, c)
    assert np.diff(oref["anchor_off"]).tolist() == c.facts["kept"]


@pytest.mark.parametrize("vote_len", I.CHUNK_LENS)
def test_chunk_cap(engine, vote_len):
    c = I.chunk_case(vote_len)
    assert (c.facts["multi"] > 0) == (vote_len > I.VOTE_MZ)
    run_case(engine, c)


def test_trips(engine):
    c = I.trip_case()
    assert c.facts["chunk_hits"] == (274, 511, 512, 513, 1316)
    assert [int(p[-1]) for p in c.facts["prefix"]] == [274, 511, 512, 513, 1316]
    run_case(engine, c)


def test_geometry(engine):
    c = I.geometry_case()
    assert {1, 2, 3, 4, 7} <= set(c.facts["nsub"]) and [len(q) for q in c.queries[:8:2]] == [255, 256, 257, 300]
    run_case(engine, c)


def test_sub_read_cap(engine):
    c = I.subcap_case()
    assert c.facts["nsub"][::2] == [511, 512, 513, 1025]
    run_case(engine, c)


@pytest.mark.parametrize("o", range(len(I.THR_OPTS)))
def test_threshold(engine, o):
    c = I.threshold_case(o)
    oref = run_case(engine, c)
    off = oref["anchor_off"]
    kept = set(oref["anchors"][off[0]:off[1]].tolist())          # (compare_all: the engine's sorted keys are these)
    fate = c.facts["fate"]
    assert any(s for _, _, s in fate) and not all(s for _, _, s in fate)
    for _, key, stays in fate:
        assert (key in kept) == stays, hex(key)


def test_counter_width(engine):
    c = I.width_case()
    assert c.facts["hits"][:4] == [65535, 65535, 65536, 65536] == c.facts["vmax"][:4]          # all of them votes of ONE bin
    oref = run_case(engine, c)
    assert np.diff(oref["anchor_off"]).tolist()[:4] == c.facts["hits"][:4]                     # and all of them stay


def test_wide_bin(engine):
    c = I.wide_bin_case()
    assert min(c.facts["vmax"]) > 65535
    run_case(engine, c)


@pytest.mark.parametrize("voted", [False, True], ids=["plain", "voted"])
@pytest.mark.parametrize("over", [True, False], ids=["with_over", "fit"])
def test_sort_tiers(engine, voted, over):
    """one query per tier edge.  with_over: the 20,481 query in the same range sends the range through the two-step form with the
    fall-back beside k_segsort with LoadKeys; fit: the fused producer (plain) or the staging pieces in place (voted)"""
    c = I.tier_case(voted)
    assert tuple(c.facts["counts"]) == I.TIER_COUNTS
    if not over:
        c = I.without_over(c)
    oref = run_case(engine, c)
    assert np.diff(oref["anchor_off"]).tolist() == c.facts["counts"]
    ctr = engine.counters()
    assert (ctr["over_queries"], ctr["over_ranges"]) == ((1, 1) if over else (0, 0))


# the launch paths that are read once per process
PATHS = [
    {"TELR_AB": "vote_filter"},
    {"TELR_AB": "sort64"},
    {"TELR_AB": "seed_unfused"},
    {"TELR_BATCH_KBP": "1"},
    {"TELR_BATCH_KBP": "1", "TELR_PIPELINE": "force"},
]


@pytest.mark.parametrize("env", PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_launch_paths(env):
    e = dict(os.environ); e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vote_child.py")], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "vote child ok" in out, out[-3000:]
