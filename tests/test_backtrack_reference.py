"""The oracle's tap between the chaining scores and the banded DP (tor_debug_backtrack: chain_backtrack, select_chains in pass 1 and
the problem list that align_chain runs), which tests/test_gpu_backtrack_edges.py holds the engine's telr_debug_backtrack to, checked
on the CPU: it equals the restatement in Python on every case of tests/backtrack_edges.py, every case reaches the edge it is built
for, and on the bundled fixture the tap reproduces the chains of the real pipeline from the pipeline's own anchors, f and p."""
import numpy as np
import pytest

from telr_amd.fasta import read_fasta
from telr_amd.presets import preset
import backtrack_edges as E

NAMES = [c["name"] for c in E.cases()]


@pytest.fixture(scope="module")
def restated():
    return {}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_tap_equals_restatement_and_reaches_edge(name, restated):
    case = E.cases()[NAMES.index(name)]
    want = E.ref_backtrack(case)
    got = E.oracle_out(case)
    E.assert_same(got, want, name)
    # what the case is built for, from the reference's output (parents: from the restatement, whose other arrays equal the oracle's)
    case["reach"](dict(got, parents=want["parents"]), case)


def test_every_listed_edge_has_a_case():
    """the sizes the kernels change their path at, over all cases (each case asserts its own edge in `reach`)"""
    per_q = np.concatenate([np.diff(c["q_aoff"]) for c in E.cases()])
    assert set((1, 63, 64, 65, 127, 128, 129, 511, 512, 513)) <= set(per_q) and 0 in per_q and per_q.max() > E.SEGSORT_CAP
    lb = set(int(c["mo"].chain_lookback) for c in E.cases())
    assert lb >= {64, 128, 256}
    assert any(c["mo"].flags & E.MF_CHAIN_SKIP for c in E.cases()) and any(c["mo"].flags & E.MF_PER_TARGET for c in E.cases())
    nch = np.concatenate([np.diff(E.oracle_out(c)["ch_off"]) for c in E.cases()])
    assert set((63, 64, 65, 129)) <= set(nch)
    kcnt = np.concatenate([E.oracle_out(c)["kept"][:, 2] for c in E.cases() if c["mo"].flags & E.MF_CIGAR])
    assert set((1, 2, 63, 64, 65, 128, 129)) <= set(kcnt)
    ncut = np.concatenate([np.diff(E.oracle_out(c)["prob_off"]) for c in E.cases()])
    assert ncut.max() >= 129


def fixture_tap_input(data_dir):
    """the bundled map-ont fixture through the oracle: its anchors, f, p as the tap's input, and the chains the pipeline reports"""
    from oracle import binding as ob
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-ont")
    o = ob.OracleIndex(ts, io).map(qs, mo, debug=True)
    goff, tlen = E.targets([len(t) for t in ts])
    g = (o["anchors"] >> np.uint64(32)).astype(np.int64) & 0x7fffffff
    assert len(g) > 0 and g.max() < int(goff[-1])
    args = (o["anchors"], o["anchor_off"].astype(np.int32), o["f"], o["p"], np.array([len(q) for q in qs], np.int32), goff, tlen, mo)
    return args, o


def test_tap_reproduces_the_pipeline_chains(data_dir):
    from oracle import binding as ob
    args, o = fixture_tap_input(data_dir)
    out = ob.debug_backtrack(*args)
    assert len(o["chains"]) >= 18
    np.testing.assert_array_equal(out["chains"], o["chains"])
    # every record of the pipeline comes from a chain that pass 1 kept, and with the CIGAR bit every kept chain has problems
    kept = set(map(tuple, out["kept"][:, (0, 4, 1, 2)]))
    assert set(map(tuple, np.stack([o["alns"][f] for f in ("qid", "tid", "score", "cnt")], 1))) <= kept
    assert np.all(np.diff(out["prob_off"]) >= 1)
