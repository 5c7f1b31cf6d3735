"""minimap2's high-occurrence seed rescue and its MAPQ on the device (TELR_MF_SEED_RESCUE = the oracle's 0x2000, TELR_MF_MM2_MAPQ = its
0x20000): engine == oracle bit for bit end to end (anchors, f, p, chains, every record field, every CIGAR, the counters: compare_all
of tests/test_gpu_parity.py) on every seeding path.  Each test except the bundled fixture first asserts its precondition on the
oracle alone -- the bit changes the oracle's output (or, where the rule does not apply, leaves it alone) -- so that none of them can
pass on an engine that ignores the bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from telr_amd.fasta import read_fasta
from telr_amd.presets import preset
from telr_amd._abi import MF_PER_TARGET, MF_SEED_RESCUE, MF_MM2_MAPQ, MF_CHAIN_SKIP
import chain_skip_inputs as CI
import seed_rescue_inputs as I
from test_gpu_parity import compare_all, ALN_FIELDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_pair(targets, queries, io, mo, bit, qtarget=None):
    """the oracle's debug output with `bit` set in mo.flags and without it"""
    from oracle import binding as ob
    on = mo.copy(); on.flags |= bit
    off = mo.copy(); off.flags &= ~bit
    oix = ob.OracleIndex(list(targets), io)
    return on, oix.map(list(queries), on, qtarget=qtarget, debug=True), oix.map(list(queries), off, qtarget=qtarget, debug=True)


def _gainers(o, o0):
    return int((np.diff(o["anchor_off"]) > np.diff(o0["anchor_off"])).sum())


def _records_differ(o, o0):
    a, b = o["alns"], o0["alns"]
    return len(a) != len(b) or any(x.tobytes() != y.tobytes() for x, y in zip(a, b)) or not np.array_equal(o["cigars"], o0["cigars"])


def _same_output(o, o0):
    return all(np.array_equal(o[k], o0[k]) for k in ("anchors", "anchor_off", "f", "p", "chains", "cigars")) and o["alns"].tobytes() == o0["alns"].tobytes()


@pytest.mark.parametrize("pname", ["map-ont", "asm10"])
def test_two_family(engine, pname):
    targets, queries = I.two_family()
    io, mo = preset(pname)
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE)
    assert _gainers(o, o0) >= len(queries) // 2 and _records_differ(o, o0)
    compare_all(engine, targets, queries, io, on)


def test_two_family_ngmlr_ont(engine):
    targets, queries = I.two_family()
    io, mo = preset("ngmlr-ont")
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE)
    assert _gainers(o, o0) >= 1 and _records_differ(o, o0)
    compare_all(engine, targets, queries, io, on)


@pytest.mark.parametrize("pname", ["map-ont", "asm10", "ngmlr-ont"])
def test_two_family_with_chain_skip(engine, pname):
    targets, queries = I.two_family()
    io, mo = preset(pname, chain_skip=True)
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE)
    assert on.flags & MF_CHAIN_SKIP and _gainers(o, o0) >= 1 and _records_differ(o, o0)
    compare_all(engine, targets, queries, io, on)


def test_over_size_query(engine):
    """the last query (seed_rescue_inputs.over_query: 70 pieces across A copies) holds more anchors than one workgroup sorts in LDS
    only BECAUSE of the rescue; its range takes the two-step seeding"""
    targets, queries = I.two_family()
    queries = list(queries) + [I.over_query()]
    io, mo = preset("map-ont")
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE)
    assert o["anchor_off"][-1] - o["anchor_off"][-2] > 20480 >= o0["anchor_off"][-1] - o0["anchor_off"][-2]
    compare_all(engine, targets, queries, io, on)
    assert engine.counters()["over_queries"] > 0


@pytest.mark.parametrize("pname", ["map-ont", "asm10", "ngmlr-ont"])
def test_small_clamped_case(engine, pname):
    targets, queries = I.small_case()
    io, mo = I.clamp_opts(pname)
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE)
    assert _gainers(o, o0) == 1
    compare_all(engine, targets, queries, io, on)


@pytest.mark.parametrize("pname", ["map-ont", "ngmlr-ont"])
def test_edges(engine, pname):
    """every named edge of the rule (seed_rescue_inputs.EDGE_NAMES) in one call, all stages compared; the voting preset takes the
    same queries through k_vote_rescue"""
    targets, io, mo, _, cases = I.edge_cases()
    if pname != I.EDGE_PRESET:
        io, mo = I.clamp_opts(pname)
    queries = [c["query"] for c in cases]
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE)
    gain = np.diff(o["anchor_off"]) - np.diff(o0["anchor_off"])
    if pname == I.EDGE_PRESET:
        # the anchors a query gains are the occurrences of the minimizers the restatement expects
        for q, c in enumerate(cases):
            assert gain[q] == sum(int(c["occ"][i]) for i in c["rescued"]), c["name"]
    assert (gain > 0).any()
    compare_all(engine, targets, queries, io, on)


def test_per_target_call_is_left_alone(engine):
    targets, queries = I.two_family()
    extra, _ = I.small_case()
    targets = list(targets) + list(extra)
    io, mo = preset("asm10")
    mo.flags |= MF_PER_TARGET
    on, o, o0 = _oracle_pair(targets, queries[:12], io, mo, MF_SEED_RESCUE)
    assert _same_output(o, o0)
    compare_all(engine, targets, queries[:12], io, on)


def test_qtarget_call_is_left_alone(engine):
    targets, queries = I.two_family()
    extra, _ = I.small_case()
    targets = list(targets) + list(extra)
    qt = np.zeros(12, np.int32)
    io, mo = preset("map-ont")
    on, o, o0 = _oracle_pair(targets, queries[:12], io, mo, MF_SEED_RESCUE, qtarget=qt)
    assert _same_output(o, o0)
    compare_all(engine, targets, queries[:12], io, on, qtarget=qt)


def test_qtarget_call_unrestricted_entries_follow_the_oracle(engine):
    """a per-query target array with -1 entries: the oracle applies the rule to the unrestricted queries (pooled cut-off) and not to the others"""
    targets, queries = I.two_family()
    qt = np.array([0, -1] * 6, np.int32)
    io, mo = preset("map-ont")
    on, o, o0 = _oracle_pair(targets, queries[:12], io, mo, MF_SEED_RESCUE, qtarget=qt)
    gain = np.diff(o["anchor_off"]) - np.diff(o0["anchor_off"])
    assert (gain[0::2] == 0).all() and (gain[1::2] > 0).any()
    compare_all(engine, targets, queries[:12], io, on, qtarget=qt)


def test_fixture_map_ont(engine, data_dir):
    """(a no-drift check of both modes on the bundled fixture, not a precondition)"""
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-ont", seed_rescue=True)
    res, _ = compare_all(engine, ts, qs, io, mo)
    assert len(res.alns) >= 18
    io, mo = preset("map-ont", seed_rescue=True, mm2_mapq=True)
    compare_all(engine, ts, qs, io, mo)


def _only_mapq_differs(o, o0):
    a, b = o["alns"], o0["alns"]
    assert len(a) == len(b) and np.array_equal(o["cigars"], o0["cigars"])
    for f in ALN_FIELDS:
        if f != "mapq":
            assert np.array_equal(a[f], b[f]), f
    return int((a["mapq"] != b["mapq"]).sum())


def test_mm2_mapq_hard_genome_2000_reads(engine):
    ref = [bytes(c).decode() for c in CI.hard_genome()["ref"]]
    reads = [bytes(r).decode() for r in CI.hard_ont_reads(2000)]
    assert len(reads) == 2000
    io, mo = preset("map-ont")
    on, o, o0 = _oracle_pair(ref, reads, io, mo, MF_MM2_MAPQ)
    assert _only_mapq_differs(o, o0) >= 1
    compare_all(engine, ref, reads, io, on)


@pytest.mark.parametrize("pname", ["map-ont", "asm10", "ngmlr-ont"])
def test_two_family_both_bits(engine, pname):
    targets, queries = I.two_family()
    io, mo = preset(pname)
    on, o, o0 = _oracle_pair(targets, queries, io, mo, MF_SEED_RESCUE | MF_MM2_MAPQ)
    assert on.flags & MF_SEED_RESCUE and on.flags & MF_MM2_MAPQ and _gainers(o, o0) >= 1 and _records_differ(o, o0)
    compare_all(engine, targets, queries, io, on)


# the other launch paths of the seeding stage, each in a process of its own (the switches are read once per process): the two-step
# seeding, the library sort, compacted minimizer arrays, and several ranges
PATHS = [
    {"TELR_AB": "seed_unfused"},
    {"TELR_AB": "sort64"},
    {"TELR_AB": "mz_compact"},
    {"TELR_BATCH_KBP": "40"},
    {"TELR_BATCH_KBP": "40", "TELR_PIPELINE": "force"},
]


@pytest.mark.parametrize("env", PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_launch_paths(env):
    e = dict(os.environ); e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seed_rescue_child.py")], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "seed rescue child ok" in out, out[-3000:]
