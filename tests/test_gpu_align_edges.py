"""What turns per-problem DP results into a record's numbers and CIGAR -- the retry pass (k_retry_collect, k_retry_build, the second
dp_pass, k_retry_merge), the per-chain sums (k_chain_stats), CIGAR stitching (k_stitch_count, the offset scan, k_stitch_write), DpRes.mcols
of every trace-back walk and the per-class accounts (k_dp_account) -- through the engine's two taps: telr_debug_stitch runs the stitch
and chain-sum kernels on hand-made per-problem results, telr_debug_align runs the map path's dp_passes, stitch_count, k_stitch_write and
chain_numbers on a caller's chains of DP problems.  On every case of tests/align_edges.py the taps equal the references exactly
(ref_stitch: plain Python; ref_align: the oracle's per-problem DP and a restatement of align_chain's retry rule, stitching and sums);
tests/test_align_ref.py checks on the CPU that the references are right and that each case reaches the edge it is built for (64-problem
windows, merges across them, empty problems and extensions, retry lists of one wave, a retry in another class, every DP class, the
rounding of convex-cost scores, the last block of the accounts)."""
import numpy as np
import pytest

from telr_amd._abi import N_DPCLS
from telr_amd._lib import TelrError
from telr_amd.aligner import SeqSet
import align_edges as E

pytestmark = pytest.mark.gpu
STITCH, ALIGN = E.STITCH_NAMES, E.ALIGN_NAMES           # (the cases are built inside the tests: that loads the library)


def _stitch(engine, c, **kw):
    a = dict(p_off=c["p_off"], has_left=c["has_left"], prob=c["prob"], cigars=c["cigars"], cx_scale=c["cx_scale"])
    a.update(kw)
    return engine.debug_stitch(a["p_off"], a["has_left"], a["prob"], a["cigars"], a["cx_scale"])


_SETS = {}


def _align(engine, c, **kw):
    if c["name"] not in _SETS:
        _SETS.clear()                                   # one case's sequences on the device at a time
        _SETS[c["name"]] = (SeqSet(engine, c["qs"]), SeqSet(engine, c["ts"]))
    q, t = _SETS[c["name"]]
    a = dict(mo=c["mo"], chains=c["chains"], prob_off=c["prob_off"], rows=c["rows"])
    a.update(kw)
    return engine.debug_align(q, t, a["mo"], a["chains"], a["prob_off"], a["rows"])


@pytest.mark.parametrize("name", STITCH)
def test_stitch_tap_equals_restatement(engine, name):
    case = E.stitch_case(name)
    E.assert_stitch_same(_stitch(engine, case), E.ref_of(case), name)


@pytest.mark.parametrize("name", ALIGN)
def test_align_tap_equals_reference(engine, name):
    case = E.align_case(name)
    got = _align(engine, case)
    E.assert_align_same(got, E.ref_of(case), name)
    # the accounts of the call are a recount of its own per-problem output
    acc = E.account(case["rows"], got["probs"])
    bad = np.flatnonzero(got["acc"] != acc)
    assert len(bad) == 0, "%s: account slot %d (class %d, column %d) is %d, recounted %d" % (name, bad[0], bad[0] // 4, bad[0] % 4, got["acc"][bad[0]], acc[bad[0]])
    assert len(got["acc"]) == N_DPCLS * 4 + 1 and int(got["acc"][-1]) == int(case["rows"][:, 5].sum())


def test_the_retry_runs_in_another_class(engine):
    """the tap reports the class of the first pass; the wide row alone, as a chain of its own, reports the class the retry ran in"""
    case = E.align_case("al_retry_class_change")
    got, ref = _align(engine, case), E.ref_of(case)
    cls = [int(v) for v in got["probs"]["cls"]]
    assert cls == [int(v) for v in ref["probs"]["cls"]] and cls[0] != cls[1]
    assert list(got["probs"]["retried"]) == [1, 0] and got["n_retry"] == 1
    for f in ("score", "bi", "bj", "mlen", "mcols", "nops"):
        assert got["probs"][f][0] == got["probs"][f][1], f
    assert got["probs"]["cells"][0] > got["probs"]["cells"][1]          # both passes' cells
    assert np.array_equal(got["cigars"][0], got["cigars"][1])


def test_every_class_was_seen_on_the_device(engine):
    seen = set()
    for case in E.align_cases():
        if case["name"].startswith("al_classes_"):
            seen |= set(int(v) for v in _align(engine, case)["probs"]["cls"])
    assert seen == set(range(N_DPCLS))


def test_a_second_run_gives_the_same_bytes(engine):
    """the order of the retry list is not fixed (one atomic per wave); what comes out is"""
    for name in ("al_retry_257", "al_counts"):
        case = E.align_case(name)
        a, b = _align(engine, case), _align(engine, case)
        assert a["n_retry"] == b["n_retry"] > 64 and a["acc"].tobytes() == b["acc"].tobytes()
        for grp in ("chains", "probs"):
            for f in a[grp]:
                assert a[grp][f].tobytes() == b[grp][f].tobytes(), (name, grp, f)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["cigars"], b["cigars"]))
    case = E.stitch_case("st_counts")
    a, b = _stitch(engine, case), _stitch(engine, case)
    assert all(a[f].tobytes() == b[f].tobytes() for f in a if f != "cigars") and all(x.tobytes() == y.tobytes() for x, y in zip(a["cigars"], b["cigars"]))


def test_stitch_tap_refuses_malformed_input(engine):
    c = E.stitch_case("st_skip_and_owner")
    E.assert_stitch_same(_stitch(engine, c), E.ref_of(c), c["name"])

    def changed(arr, i, v):
        a = c[arr].copy(); a[i] = v
        return {arr: a}
    cig_bad_op = [x.copy() for x in c["cigars"]]; cig_bad_op[2][0] = E.op(3, 3)
    cig_no_len = [x.copy() for x in c["cigars"]]; cig_no_len[2][0] = E.op(0, E.M)
    bad = [
        ("p_off[0]", changed("p_off", 0, 1)),
        ("p_off descends", dict(p_off=np.array([0, 5, 4, 8], np.int32), has_left=np.array([0, 0, 0], np.int32))),
        ("a chain without a problem", dict(p_off=np.array([0, 4, 4, 8], np.int32), has_left=np.array([0, 0, 0], np.int32))),
        ("p_off past the problems", changed("p_off", 2, 9)),
        ("has_left 2", changed("has_left", 1, 2)),
        ("has_left too short", dict(has_left=c["has_left"][:1])),
        ("negative bi", changed("prob", (3, 1), -1)),
        ("negative mcols", changed("prob", (3, 4), -1)),
        ("op code 3", dict(cigars=cig_bad_op)),
        ("op of no length", dict(cigars=cig_no_len)),
        ("a CIGAR short of the problems", dict(cigars=c["cigars"][:-1])),
        ("cx_scale", dict(cx_scale=65)),
        ("cx_scale negative", dict(cx_scale=-1)),
    ]
    for what, kw in bad:
        with pytest.raises(TelrError):
            _stitch(engine, c, **kw)
            pytest.fail("accepted: " + what)
    E.assert_stitch_same(_stitch(engine, c), E.ref_of(c), c["name"])          # and the engine still works


def test_align_tap_refuses_malformed_input(engine):
    c = E.align_case("al_empty_ext")
    E.assert_align_same(_align(engine, c), E.ref_of(c), c["name"])
    o = c["prob_off"]
    assert [int(v) for v in c["rows"][o[0]:o[1], 8]] == [1, 0, 0, 0, 2] and [int(v) for v in c["rows"][o[4]:o[5], 8]] == [1, 0, 0]

    def rows(i, col, v):
        a = c["rows"].copy(); a[i, col] = v
        return dict(rows=a)

    def chain(k, col, v):
        a = c["chains"].copy(); a[k, col] = v
        return dict(chains=a)

    def both(k, cols, d):
        a = c["chains"].copy(); a[k, list(cols)] += d
        return dict(chains=a)

    def swapped(i, j):
        a = c["rows"].copy(); a[[i, j]] = a[[j, i]]
        return dict(rows=a)
    qlen0, tlen0 = len(c["qs"][0]), len(c["ts"][0])
    bad = [
        ("prob_off[0]", dict(prob_off=np.concatenate([[1], o[1:]]).astype(np.int32))),
        ("prob_off descends", dict(prob_off=np.concatenate([o[:2], [o[1] - 1], o[3:]]).astype(np.int32))),
        ("a chain without a row", dict(prob_off=np.concatenate([o[:2], [o[1]], o[3:]]).astype(np.int32))),
        ("prob_off past the rows", dict(prob_off=np.concatenate([o[:-1], [o[-1] + 1]]).astype(np.int32))),
        ("a row of another query", rows(1, 0, 1)),
        ("a row of another target", rows(1, 2, 1)),
        ("a row of the other strand", rows(1, 11, 1)),
        ("kind 4", rows(1, 8, 4)),
        ("odd dlo", rows(1, 6, int(c["rows"][1, 6]) + 1)),
        ("a window outside its sequence", rows(1, 4, 100000)),
        ("a fill in front of the left extension", swapped(0, 1)),
        ("a fill behind the right extension", swapped(3, 4)),
        ("two left extensions", rows(1, 8, 1)),
        ("no left extension although qs > 0 and rs > 0", dict(prob_off=np.concatenate([[0], o[1:] - 1]).astype(np.int32), rows=c["rows"][1:],
                                                            chains=c["chains"])),
        ("a left extension although qs = 0", chain(0, 3, 0)),
        ("a right extension although qe = qlen", chain(0, 4, qlen0)),
        ("a right extension although re = tlen", chain(0, 6, tlen0)),
        ("no right extension although the chain ends inside both", both(4, (4, 6), -1)),
        ("only extensions", dict(prob_off=np.concatenate([o[:4], [o[3] + 2], o[5:] - 1]).astype(np.int32), rows=np.delete(c["rows"], o[3] + 1, 0))),
        ("rev 2", chain(0, 2, 2)),
        ("qe past the query", chain(0, 4, qlen0 + 1)),
        ("qs behind qe", chain(0, 3, int(c["chains"][0, 4]) + 1)),
        ("a query that is not there", chain(0, 0, len(c["qs"]))),
        ("options", dict(mo=E._mo("map-ont", chain_lookback=100))),
    ]
    assert int(o[4] - o[3]) == 3 and [int(v) for v in c["rows"][o[3]:o[4], 8]] == [1, 0, 2]
    for what, kw in bad:
        with pytest.raises(TelrError):
            _align(engine, c, **kw)
            pytest.fail("accepted: " + what)
    with pytest.raises(TelrError) as e:
        _align(engine, c, **swapped(o[2], o[2] + 1))
    assert "chain 2" in str(e.value)                                          # the refusal names the chain
    E.assert_align_same(_align(engine, c), E.ref_of(c), c["name"])            # and the engine still works
