"""minimap2's chaining scan on the device (TELR_MF_CHAIN_SKIP = the oracle's 0x1000): engine == oracle bit for bit end to end
(anchors, f, p, chains, every record field, every CIGAR, the counters: compare_all of tests/test_gpu_parity.py), every launch path
of the chaining stage, and telr_debug_chain on the hand-built edges of the scan against the restatement (tests/chain_scan_ref.py).
Each end-to-end input except the bundled fixture asserts first that the oracle's f / p with the bit differ from those without it,
so that none of these tests can pass on an engine that ignores the bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from telr_amd.fasta import read_fasta
from telr_amd.presets import preset
from telr_amd._abi import MF_PER_TARGET
import chain_scan_ref as R
import chain_skip_inputs as I
from test_gpu_parity import compare_all

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strs(xs):
    return [bytes(x).decode() if not isinstance(x, str) else x for x in xs]


def _oracle_pair(targets, queries, pname, flags=0, qtarget=None):
    """the oracle's debug output with and without the bit"""
    from oracle import binding as ob
    io, mo = preset(pname, chain_skip=True)
    _, mo0 = preset(pname)
    mo.flags |= flags; mo0.flags |= flags
    oix = ob.OracleIndex(_strs(targets), io)
    q = _strs(queries)
    return io, mo, oix.map(q, mo, qtarget=qtarget, debug=True), oix.map(q, mo0, qtarget=qtarget, debug=True)


def _fp_differ(o, o0):
    assert np.array_equal(o["anchors"], o0["anchors"])
    return not (np.array_equal(o["f"], o0["f"]) and np.array_equal(o["p"], o0["p"]))


def _max_link(o):
    off, p = o["anchor_off"], o["p"]
    idx = np.concatenate([np.arange(off[q + 1] - off[q]) for q in range(len(off) - 1)])
    return int((idx - p)[p >= 0].max())


def test_fixture_map_ont(engine, data_dir):
    """(on the fixture the scan and the fixed look-back give the same f / p: a no-drift check of the mode, not a precondition)"""
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-ont", chain_skip=True)
    res, _ = compare_all(engine, ts, qs, io, mo)
    assert len(res.alns) >= 18


def test_hard_clr_map_pb(engine):
    ref = [bytes(c).decode() for c in I.hard_genome()["ref"]]
    reads = I.hard_clr_reads()
    io, mo, o, o0 = _oracle_pair(ref, reads, "map-pb")
    assert _fp_differ(o, o0)
    compare_all(engine, ref, reads, io, mo)


def test_asm10_per_target(engine):
    ref = [bytes(c).decode() for c in I.hard_genome()["ref"]]
    reads = I.hard_ont_reads()[:100]
    io, mo, o, o0 = _oracle_pair(ref, reads, "asm10", flags=MF_PER_TARGET)
    assert _fp_differ(o, o0)
    compare_all(engine, ref, reads, io, mo)


def test_ngmlr_ont(engine):
    ref = [bytes(c).decode() for c in I.hard_genome()["ref"]]
    reads = I.hard_ont_reads()[:150]
    io, mo, o, o0 = _oracle_pair(ref, reads, "ngmlr-ont")
    assert _fp_differ(o, o0)
    compare_all(engine, ref, reads, io, mo)


def test_hard_genome_map_ont_2000_reads(engine):
    ref = [bytes(c).decode() for c in I.hard_genome()["ref"]]
    reads = I.hard_ont_reads(2000)
    assert len(reads) == 2000
    io, mo, o, o0 = _oracle_pair(ref, reads, "map-ont")
    assert _fp_differ(o, o0)
    # records change, links reach past the back-tracking ring of the fixed look-back (BT_RING = 512), and the scans that the
    # 25-skip rule ends are there (restatement on the first 60 reads)
    a, b = o["alns"], o0["alns"]
    assert len(a) != len(b) or any(x.tobytes() != y.tobytes() for x, y in zip(a, b))
    assert _max_link(o) > 512
    st = {}
    off = o["anchor_off"]
    R.chain_scan_all(o["anchors"][:off[60]], off[:61], mo, st)
    assert st["breaks"] > 0
    compare_all(engine, ref, reads, io, mo)


def test_debug_chain_hand_built_edges(engine):
    mo = R.hand_opts()
    for name, lists, checks in R.hand_cases():
        keys, off = R.concat_lists(lists)
        f, p = engine.debug_chain(keys, off, mo)
        ef, ep = R.chain_scan_all(keys, off, mo)
        np.testing.assert_array_equal(f, ef, err_msg=name)
        np.testing.assert_array_equal(p, ep, err_msg=name)
        for q, exp in checks.items():
            for i, want in exp.items():
                assert p[off[q] + i] == want, (name, q, i)


def test_debug_chain_random_lists(engine):
    mo = R.hand_opts()
    for seed in (1, 2):
        keys, off = R.concat_lists(R.random_lists(seed))
        f, p = engine.debug_chain(keys, off, mo)
        ef, ep = R.chain_scan_all(keys, off, mo)
        np.testing.assert_array_equal(f, ef)
        np.testing.assert_array_equal(p, ep)


def test_debug_chain_on_oracle_anchor_lists_both_modes(engine):
    """the oracle's own anchor lists of hard-genome reads through telr_debug_chain: with the bit the oracle's f / p under 0x1000,
    without it the oracle's default chain_dp (the same entry runs the default dispatch unchanged)"""
    ref = [bytes(c).decode() for c in I.hard_genome()["ref"]]
    reads = I.hard_ont_reads()[:200]
    _, mo, o, o0 = _oracle_pair(ref, reads, "map-ont")
    _, mo0 = preset("map-ont")
    off = o["anchor_off"].astype(np.int32)
    f, p = engine.debug_chain(o["anchors"], off, mo)
    np.testing.assert_array_equal(f, o["f"]); np.testing.assert_array_equal(p, o["p"])
    f0, p0 = engine.debug_chain(o0["anchors"], off, mo0)
    np.testing.assert_array_equal(f0, o0["f"]); np.testing.assert_array_equal(p0, o0["p"])


def test_debug_chain_refuses_bad_input(engine):
    from telr_amd._lib import TelrError
    mo = R.hand_opts()
    keys = np.array([R.key(200, 200), R.key(100, 100)], np.uint64)
    with pytest.raises(TelrError):            # not sorted
        engine.debug_chain(keys, np.array([0, 2], np.int32), mo)
    bad = mo.copy(); bad.chain_lookback = 100
    with pytest.raises(TelrError):            # fails check_map_opt
        engine.debug_chain(keys[::-1].copy(), np.array([0, 2], np.int32), bad)


# the other launch paths, each in a process of its own (the switches are read once per process): one wave per query (no islands),
# several pipelined ranges, and small k_chain_mw thresholds (the multi-wave loop must leave the scan's runs alone)
PATHS = [
    {"TELR_AB": "no_islands"},
    {"TELR_BATCH_KBP": "400"},
    {"TELR_CHAIN_DENSE": "128,300,128"},
    {"TELR_AB": "no_islands", "TELR_CHAIN_DENSE": "128,300,128"},
]


@pytest.mark.parametrize("env", PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_launch_paths(env):
    e = dict(os.environ); e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_skip_child.py"), "300"], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "chain skip child ok" in out, out[-3000:]
