"""The three device stages between the chaining scores and the banded DP -- peaks and back-tracking (k_nonpeak, k_peaks, the peak sort,
k_bt_rank, k_bt_owner, k_bt_depth, k_bt_emit, k_bt_scatter), pass-1 chain selection (k_sel_keys, the chain sort, k_select1,
k_select1_write) and DP segmenting (k_segments_w) -- through the engine's tap telr_debug_backtrack, which runs the launches of telr_map
on a caller's anchors, f and p.  On every case of tests/backtrack_edges.py the tap's arrays (chains, chain anchors, kept list, DP
problem rows, and their offsets) equal the oracle tap's exactly; tests/test_backtrack_reference.py checks on the CPU that the oracle
tap is right and that each case reaches the edge it is built for (block, ring, round, SEL_PCAP, tally and window sizes)."""
import numpy as np
import pytest

from telr_amd._lib import TelrError
import backtrack_edges as E
from test_backtrack_reference import fixture_tap_input

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in E.cases()]


def _tap(engine, c, **kw):
    a = dict(keys=c["keys"], q_aoff=c["q_aoff"], f=c["f"], p=c["p"], qlen=c["qlen"], goff=c["goff"], tlen=c["tlen"], mo=c["mo"])
    a.update(kw)
    return engine.debug_backtrack(a["keys"], a["q_aoff"], a["f"], a["p"], a["qlen"], a["goff"], a["tlen"], a["mo"])


@pytest.mark.parametrize("name", NAMES)
def test_engine_tap_equals_oracle_tap(engine, name):
    case = E.cases()[NAMES.index(name)]
    E.assert_same(_tap(engine, case), E.oracle_out(case), name)


def test_both_rings_are_covered():
    flags = [int(c["mo"].flags) & E.MF_CHAIN_SKIP for c in E.cases()]
    assert any(flags) and not all(flags)


def test_fixture_round_trip(engine, data_dir):
    """the oracle's own anchors, f and p of the bundled fixture through the engine's tap: the chains the pipeline reports"""
    from oracle import binding as ob
    args, o = fixture_tap_input(data_dir)
    got = engine.debug_backtrack(*args)
    np.testing.assert_array_equal(got["chains"], o["chains"])
    E.assert_same(got, ob.debug_backtrack(*args), "fixture")


def test_refuses_what_a_kernel_would_index_with(engine):
    """every rule of the host-side validation comes back as TelrError, before anything is launched"""
    c = E.cases()[NAMES.index("bt_forest")]
    assert len(_tap(engine, c)["chains"]) == 2

    def changed(arr, i, v):
        a = c[arr].copy(); a[i] = v
        return {arr: a}
    L = int(c["mo"].chain_lookback)
    far = E.Build("far", c["mo"]).query(3000, E.line(L + 2), [50] * (L + 1) + [90], [-1] * (L + 1) + [0]).done(None, "")
    far_scan = dict(far, mo=E.opts(flags=E.MF_CHAIN_SKIP, min_cnt=2))
    assert len(_tap(engine, far_scan)["chains"]) > 0            # the same link is inside the look-back of the chain-skip mode
    n = E.CHAIN_SCAN_H + 2
    too_far_scan = E.Build("far2", E.opts(flags=E.MF_CHAIN_SKIP)).query(n * 10 + 300, E.line(n), [50] * (n - 1) + [90], [-1] * (n - 1) + [0]).done(None, "")
    bad = [
        ("options", dict(mo=E.opts(chain_lookback=100))),
        ("q_aoff[0]", changed("q_aoff", 0, 1)),
        ("q_aoff descends", dict(q_aoff=np.array([0, 14, 13], np.int32), qlen=np.array([1000, 1000], np.int32))),
        ("p below -1", changed("p", 3, -2)),
        ("p not before i", changed("p", 3, 3)),
        ("p after i", changed("p", 3, 7)),
        ("goff descends", dict(goff=np.array([c["goff"][1], c["goff"][0]], np.uint32))),
        ("anchor past goff", changed("keys", 5, E.key(int(c["goff"][-1]), 100))),
        ("query position at qlen", dict(qlen=np.array([(int(c["keys"][-1]) >> 8) & 0xffffff], np.int32))),
        ("qlen above 2^24", dict(qlen=np.array([(1 << 24) + 1], np.int32))),
        ("tlen outside goff", dict(tlen=np.array([int(c["goff"][1]) + 1], np.int32))),
    ]
    for what, kw in bad:
        with pytest.raises(TelrError):
            _tap(engine, c, **kw)
            pytest.fail("accepted: " + what)
    for what, case in (("link past the look-back", far), ("link past CHAIN_SCAN_H", too_far_scan)):
        with pytest.raises(TelrError):
            _tap(engine, case)
            pytest.fail("accepted: " + what)
    with pytest.raises(TelrError):                                # more than 2^16 queries
        n = (1 << 16) + 1
        engine.debug_backtrack(np.zeros(0, np.uint64), np.zeros(n + 1, np.int32), [], [], np.full(n, 100, np.int32), c["goff"], c["tlen"], c["mo"])
    with pytest.raises(TelrError):                                # more than 2^22 anchors (refused from the offsets alone)
        n = (1 << 22) + 1
        engine.debug_backtrack(np.zeros(n, np.uint64), np.array([0, n], np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32),
                               np.array([100], np.int32), c["goff"], c["tlen"], c["mo"])
    assert len(_tap(engine, c)["chains"]) == 2                    # and the engine still works
