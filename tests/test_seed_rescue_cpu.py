"""TELR_MF_SEED_RESCUE and TELR_MF_MM2_MAPQ without a GPU: the numpy restatement of the rescue rule (tests/seed_rescue_ref.py) against
the oracle's 0x2000 on the small inputs and on every named edge, the integer form of k the device uses, the flag values, and the
keywords and argv shapes that reach the flags."""
import numpy as np
import pytest

from telr_amd import _abi
from telr_amd.presets import preset
import seed_rescue_inputs as I
import seed_rescue_ref as R


def test_flag_values_equal_the_oracle_bits():
    assert _abi.MF_SEED_RESCUE == 0x2000
    assert _abi.MF_MM2_MAPQ == 0x20000


def test_header_defines():
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "telr_hip.h")).read()
    d = dict(re.findall(r"#define\s+(TELR_MF_\w+)\s+(0x[0-9a-fA-F]+)", h))
    assert int(d["TELR_MF_SEED_RESCUE"], 16) == 0x2000 and int(d["TELR_MF_MM2_MAPQ"], 16) == 0x20000


def test_integer_form_of_k_over_every_span():
    """(pe - ps) / 500.0 + .499 never lies on an integer, so the device's integer division is the same floor: all of 0 .. 2^24"""
    d = np.arange(0, (1 << 24) + 1, dtype=np.int64)
    kf = (d.astype(np.float64) / 500.0 + .499).astype(np.int64)
    ki = (1000 * d + 249500) // 500000
    assert np.array_equal(kf, ki)
    for x in (0, 250, 251, 750, 751, 1250, 1251, 1 << 24):
        assert R.k_float(x) == R.k_int(x) == int(ki[x])
    assert [R.k_float(x) for x in (250, 251, 750, 751)] == [0, 1, 1, 2]


def test_preset_keywords():
    for name in ("map-ont", "asm10", "ngmlr-ont"):
        _, m0 = preset(name)
        assert not m0.flags & (_abi.MF_SEED_RESCUE | _abi.MF_MM2_MAPQ)
        _, m1 = preset(name, seed_rescue=True)
        assert m1.flags == m0.flags | _abi.MF_SEED_RESCUE
        _, m2 = preset(name, mm2_mapq=True)
        assert m2.flags == m0.flags | _abi.MF_MM2_MAPQ
        _, m3 = preset(name, chain_skip=True, seed_rescue=True, mm2_mapq=True)
        assert m3.flags == m0.flags | _abi.MF_CHAIN_SKIP | _abi.MF_SEED_RESCUE | _abi.MF_MM2_MAPQ


def test_alignment_keywords_minimap2_branch_only():
    import inspect
    from telr_amd.telr_alignment import alignment
    sig = inspect.signature(alignment)
    assert sig.parameters["seed_rescue"].default is False and sig.parameters["mm2_mapq"].default is False
    for kw in ({"seed_rescue": True}, {"mm2_mapq": True}):
        with pytest.raises(ValueError):
            alignment("x.bam", "r.fa", "t.fa", ".", "s", 1, "nglmr", "ont", engine=object(), **kw)


def test_cli_e_argv_shapes():
    from telr_amd.cli_mm2 import parse_argv
    base = ["minimap2", "--cs", "--MD", "-Y", "-L", "-ax", "map-ont"]
    assert "seed_rescue" not in parse_argv(base + ["R", "Q"])          # (the dict of the reference's shapes is unchanged)
    for extra in (["-e", "500"], ["-e500"]):
        o = parse_argv(base + extra + ["R", "Q"])
        assert o["seed_rescue"] is True and o["chain_skip"] is False and (o["target"], o["query"]) == ("R", "Q")
    o = parse_argv(["minimap2", "-cx", "asm10", "-v", "0", "-N", "10", "-e", "500", "--max-chain-skip", "25", "REF", "FLANK"])
    assert o["seed_rescue"] and o["chain_skip"] and o["best_n"] == 10
    for bad in (["-e", "400"], ["-e1000"], ["-e"]):
        with pytest.raises(SystemExit) as ei:
            parse_argv(base + bad + (["R", "Q"] if bad != ["-e"] else []))
        assert "only 500 is supported" in str(ei.value)


def _oracle_on_off(targets, queries, io, mo):
    from oracle import binding as ob
    oix = ob.OracleIndex(targets, io)
    on = mo.copy(); on.flags |= _abi.MF_SEED_RESCUE
    return oix, oix.map(queries, mo, debug=True), oix.map(queries, on, debug=True)


def _check_restatement(targets, queries, io, mo, expect=None):
    """the oracle's anchors with the bit == its anchors without it + every occurrence of the minimizers the restatement marks"""
    oix, off, on = _oracle_on_off(targets, queries, io, mo)
    counts = R.IndexCounts(oix)
    mid = oix.mid_occ(mo)
    gained = 0
    for q, seq in enumerate(queries):
        res, occ, pos = R.rescued_of_query(seq, io, counts, mid)
        if expect is not None:
            assert res == expect[q], q
        a0 = off["anchors"][off["anchor_off"][q]:off["anchor_off"][q + 1]]
        a1 = on["anchors"][on["anchor_off"][q]:on["anchor_off"][q + 1]]
        extra = R.anchor_keys(seq, io, counts, res)
        assert len(extra) == int(sum(occ[i] for i in res))
        np.testing.assert_array_equal(np.sort(np.concatenate([a0, extra])), a1, err_msg="query %d" % q)
        gained += len(extra) > 0
    return gained


@pytest.mark.parametrize("pname", ["map-ont", "asm10"])
def test_restatement_against_oracle_small_case(pname):
    targets, queries = I.small_case()
    io, mo = I.clamp_opts(pname)
    assert _check_restatement(targets, queries, io, mo) == 1


def test_small_case_voting_preset_gains_anchors():
    """(sub-read voting filters the hits, so the anchors are not the plain sum: the oracle alone, bit on against bit off)"""
    targets, queries = I.small_case()
    io, mo = I.clamp_opts("ngmlr-ont")
    _, off, on = _oracle_on_off(targets, queries, io, mo)
    assert len(on["anchors"]) > len(off["anchors"])


def test_edges_named_and_restated():
    targets, io, mo, mid, cases = I.edge_cases()
    assert mid == 10 and tuple(c["name"] for c in cases) == I.EDGE_NAMES
    by = {c["name"]: c for c in cases}
    assert by["opens_query"]["stretches"][0][2] == 0
    assert by["closes_query"]["stretches"][-1][3] == len(by["closes_query"]["query"])
    for d, k in ((250, 0), (251, 1), (750, 1), (751, 2)):
        c = by["span_%d" % d]
        assert c["stretches"][0][3] - c["stretches"][0][2] == d and len(c["rescued"]) == k
    c = by["occ_4094_and_4095"]
    s, e = c["stretches"][0][:2]
    assert [int(c["occ"][i]) for i in c["rescued"]] == [4094] and int((c["occ"][s:e] == 4095).sum()) > 100
    assert by["longer_than_1024"]["stretches"][0][1] - by["longer_than_1024"]["stretches"][0][0] > 1024
    assert by["no_minimizer"]["rescued"] == []
    gained = _check_restatement(targets, [c["query"] for c in cases], io, mo, expect=[c["rescued"] for c in cases])
    assert gained == len(cases) - 2          # all but span_250 (k = 0) and no_minimizer


def test_rescue_rule_by_hand():
    """the restatement itself on lists written out by hand (mid_occ 10)"""
    # one stretch in the middle, pe - ps = 1000 -> k = 2: the two least frequent, the earlier of the equal ones
    occ = [1, 50, 30, 30, 20, 1]
    pos = [100, 200, 400, 600, 800, 1100]
    assert R.rescued(occ, pos, 2000, 10) == [2, 4]
    # opens and closes the query: ps = 0, pe = qlen = 751 -> k = 2, one candidate below 4095
    assert R.rescued([4095, 4094, 4096], [10, 20, 30], 751, 10) == [1]
    # an absent minimizer (0) splits: two stretches of one, spans 300 - 0 and 900 - 200
    assert R.rescued([11, 0, 12], [200, 300, 400], 900, 10) == [0, 2]
    # span 250 -> none
    assert R.rescued([1, 99, 1], [100, 200, 350], 1000, 10) == []
    assert R.rescued([], [], 7, 10) == []
