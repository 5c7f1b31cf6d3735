"""The depth-median definition (tests/depth_ref.py) against the hand-worked answers of tests/depth_cases.py and against the oracle's
tor_depth_medians on every well-formed case; and the cases themselves: each still reaches the edge it names."""
import numpy as np
import pytest

import depth_cases as dc
import depth_ref as ref

CASES = dc.cases() + [dc.GOOD]
BY_NAME = {c["name"]: c for c in CASES}


def same(got, want):
    """equal where both are numbers, NaN in the same places (never compared by equality)"""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_reference_gives_the_hand_worked_medians(c):
    alns, cig, tl, t, s, e = dc.arrays(c)
    same(ref.depth_medians(alns, cig, tl, t, s, e), dc.want_array(c))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_oracle_gives_the_hand_worked_medians(c):
    from oracle import binding as ob
    alns, cig, tl, t, s, e = dc.arrays(c)
    same(ob.depth_medians(alns, cig, tl, t, s, e), dc.want_array(c))


def test_every_median_is_an_integer_or_a_half():
    for c in CASES:
        w = dc.want_array(c)
        w = w[~np.isnan(w)]
        assert ((w * 2) == np.floor(w * 2)).all() and (w >= 0).all() and (w <= ref.DEPTH_CAP).all(), c["name"]


def test_cases_reach_their_edges():
    alns, cig, tl, *_ = dc.arrays(BY_NAME["cap"])
    d = ref.depths(alns, cig, tl)[0]
    assert d[10:14].tolist() == [ref.DEPTH_CAP - 1, ref.DEPTH_CAP, ref.DEPTH_CAP + 1, 20000] and d[9] == 0 and d[14] == 0
    assert all(a["n_cigar"] == 1 for a in alns)
    assert BY_NAME["cap"]["want"][:5] == [7999, 8000, 8000, 8000, 7999.5]
    # a .5 from an even interval with two different middle values, in several cases
    for name in ("cap", "order_statistics", "interval_lengths", "clamps", "ops", "ends", "records_64"):
        assert any(w is not None and w != int(w) for w in BY_NAME[name]["want"]), name
    # interval lengths 1 .. 4, and 255 / 256 / 257 (k_depth_median's stride) and two full strides
    assert {e - s + 1 for _, s, e in BY_NAME["order_statistics"]["iv"]} >= {1, 2, 3, 4}
    assert {e - s + 1 for _, s, e in BY_NAME["interval_lengths"]["iv"]} >= {255, 256, 257, 512, 513}
    # NaN: s == tlen, e < s, e < 0, and the two extremes
    c = BY_NAME["clamps"]
    L = c["tlens"][0]
    nan = {(s, e) for (_, s, e), w in zip(c["iv"], c["want"]) if w is None}
    assert {(L, 60), (10, 9), (-10, -1), (dc.I32_MAX, dc.I32_MIN)} <= nan
    num = {(s, e) for (_, s, e), w in zip(c["iv"], c["want"]) if w is not None}
    assert (dc.I32_MIN, dc.I32_MAX) in num and any(s < 0 and e >= L for s, e in num) and any(e == L - 1 for s, e in num)
    # the ops
    alns, cig, *_ = dc.arrays(BY_NAME["ops"])
    first = [int(cig[a["cigar_off"]]) & 0xf for a in alns if a["n_cigar"]]
    last = [int(cig[a["cigar_off"] + a["n_cigar"] - 1]) & 0xf for a in alns if a["n_cigar"]]
    assert 1 in first and 2 in last and 0 in alns["n_cigar"] and 65 in alns["n_cigar"]
    assert any(int(w) == 0 for w in cig)                                                       # 0M
    assert any((int(a) & 0xf) == 0 and (int(b) & 0xf) == 0 for a, b in zip(cig[:-1], cig[1:]))  # M beside M
    # the ends
    c = BY_NAME["ends"]
    alns, *_ = dc.arrays(c)
    assert 1 in c["tlens"] and any(a["te"] == c["tlens"][a["tid"]] for a in alns) and any(a["ts"] == 0 for a in alns)
    assert set(alns["tid"].tolist()) == {0, 1, 2} and len(c["tlens"]) == 4                       # target 3 has no record
    assert sum(1 for a in alns if a["tid"] == 0 and a["te"] == c["tlens"][0]) == 3 and (1, 0, 0) in c["iv"]
    # flags, counts
    alns, *_ = dc.arrays(BY_NAME["flags"])
    assert set(range(16)) <= set(alns["flags"].tolist())
    assert all(a["flags"] & dc.SEC for a in dc.arrays(BY_NAME["all_secondary"])[0]) and len(dc.arrays(BY_NAME["no_records"])[0]) == 0
    assert [len(BY_NAME["records_%d" % n]["recs"]) for n in (63, 64, 65)] == [63, 64, 65]
    assert [len(BY_NAME["intervals_%d" % n]["iv"]) for n in (0, 1, 300)] == [0, 1, 300]
    iv = BY_NAME["intervals_300"]["iv"]
    assert len(set(iv)) < len(iv) and iv != sorted(iv)


def test_refusals_are_malformed_in_the_way_they_name():
    R = {r[0]: r for r in dc.refusals()}
    for name, tlens, recs, iv, why in R.values():
        assert len(tlens) == 2                                    # a write past target 0 would land in target 1's slice
    rec = lambda name: R[name][2][-1]
    assert rec("ts_negative")["ts"] < 0
    assert R["te_before_ts"][2][0]["te"] < R["te_before_ts"][2][0]["ts"]
    assert rec("te_beyond_tlen")["te"] == 51 and rec("te_beyond_tlen_last_target")["te"] == 31
    for name in ("cigar_beyond_te_M", "cigar_beyond_te_D_then_M", "cigar_beyond_te_huge_ops"):
        r = rec(name)
        tl = R[name][1][r["tid"]]
        assert 0 <= r["ts"] <= r["te"] <= tl and r["ts"] + sum(n for n, o in r["cig"] if o in "MD") > tl, name
    assert R["interval_tid_outside"][3][-1][0] == 2 and R["interval_tid_negative"][3][0][0] == -1
    for name, tlens, recs, iv, why in R.values():
        dc.arrays(dict(recs=recs, iv=iv, tlens=tlens))             # every one packs
