"""The oracle's tap for the chaining scores (tor_debug_chain: chain_dp per query), which tests/test_gpu_chain_edges.py holds the
engine's telr_debug_chain to, checked on the CPU: fed the anchors of the oracle's own pipeline it returns that pipeline's f / p on the
bundled fixture under every preset; it equals the restatement in Python (tests/chain_edges.py: chain_default) on every case of at
most RESTATE_MAX anchors; and every case reaches the edge it is built for on the tap's output."""
import numpy as np
import pytest

from telr_amd.fasta import read_fasta
from telr_amd.presets import preset
from telr_amd._abi import MF_CHAIN_SKIP
import chain_edges as E

NAMES = [c["name"] for c in E.cases()]
PRESETS = ("map-ont", "map-pb", "ngmlr-ont", "ngmlr-pacbio", "asm10")


@pytest.mark.parametrize("pname", PRESETS)
def test_tap_reproduces_the_pipeline_scores(pname, data_dir):
    """default mode (no scan bit): chain_dp on the pipeline's anchor lists is what tor_map ran"""
    from oracle import binding as ob
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset(pname)
    assert not mo.flags & MF_CHAIN_SKIP
    o = ob.OracleIndex(ts, io).map(qs, mo, debug=True)
    assert len(o["anchors"]) > 1000 and np.count_nonzero(o["p"] >= 0) > 500
    f, p = ob.debug_chain(o["anchors"], o["anchor_off"].astype(np.int32), mo)
    np.testing.assert_array_equal(f, o["f"])
    np.testing.assert_array_equal(p, o["p"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_tap_equals_restatement_and_reaches_edge(name):
    case = E.case_named(name)
    keys, off = E.call_input(case)
    f, p = E.oracle_out(case)
    assert f.dtype == np.int32 and p.dtype == np.int32 and len(f) == len(p) == len(keys)
    if E.n_anchors(case) <= E.RESTATE_MAX:
        rf, rp = E.chain_default_all(keys, off, case["mo"])
        np.testing.assert_array_equal(f, rf, err_msg=name)
        np.testing.assert_array_equal(p, rp, err_msg=name)
    case["reach"](*E.split(f, p, off))


def test_no_setting_is_without_cases():
    for H, skip in E.SETTINGS:
        mine = [c for c in E.cases() if c["mo"].chain_lookback == H and c["mo"].chain_skip_q8 == skip]
        kinds = set(c["name"].split("_")[0] for c in mine)
        assert kinds >= {"len", "lookback", "tie", "limit", "score", "isolated", "islands", "lattice", "dense", "mw", "mixed"}, (H, skip)
        R = H // 64
        sizes = set(len(L) for c in mine for L in c["lists"])
        assert {0, 1, 2, 63, 64, 65, 64 * R - 1, 64 * R, 64 * R + 1, 2 * 64 * R + 1, 8 * 64 * R + 3, E.DENSE_N - 1, E.DENSE_N} <= sizes
    assert sum(c["name"].startswith("mw_default") for c in E.cases()) == 2
    # the restatement covers every kind of case but the two large ones
    big = set(c["name"].split("_h")[0] for c in E.cases() if E.n_anchors(c) > E.RESTATE_MAX)
    assert big == {"islands_many", "mixed_queries", "mw_default_s0", "mw_default_s3"}
