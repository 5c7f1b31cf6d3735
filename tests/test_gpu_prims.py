"""The hand-written radix sort and the tiled exclusive scan, each alone, against the plain references of tests/prim_cases.py at the
edges its tables name (tests/test_prim_ref.py shows on a CPU that the cases reach them).  Every comparison is exact."""
import numpy as np
import pytest

import prim_cases as pc
from telr_amd._abi import TELR_E_ARG, TELR_OK

pytestmark = pytest.mark.gpu


# ---- radix_sort_passes ------------------------------------------------------------------------------------------------------------------
def _sort_one(engine, bits, n, nbits, pattern):
    k = pc.sort_keys(bits, n, nbits, pattern)
    v = np.arange(n, dtype=np.uint32) if bits == 64 else None                # values = iota: the permutation itself is compared
    wk, wv = pc.sort_ref(k, nbits, v)
    gk, gv = engine.debug_radix_sort(k, nbits, v)
    return np.array_equal(gk, wk) and (v is None or np.array_equal(gv, wv)), gk, gv


@pytest.mark.parametrize("n", sorted(pc.SORT_N))
@pytest.mark.parametrize("bits", [64, 32])
def test_radix_sort_is_a_stable_sort_by_the_rounded_width(engine, bits, n):
    """<uint64_t, true> (the call stages' perm_sort_round, the index build's hash sort) and <uint32_t, false> (the index build's count
    sort): keys and permutation equal np.argsort(keys & mask, kind="stable") at every width and pattern of the table"""
    bad = [name for name, nb, pat in pc.sort_cases(bits, n) if not _sort_one(engine, bits, n, nb, pat)[0]]
    assert not bad, "%d of %d cases differ: %s" % (len(bad), len(pc.sort_cases(bits, n)), bad[:12])


def test_radix_sort_twice_gives_the_same_bytes(engine):
    a = _sort_one(engine, 64, 524289, 40, "garbage")
    b = _sort_one(engine, 64, 524289, 40, "garbage")
    assert a[0] and b[0]
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_radix_sort_tap_arguments(engine):
    L, h = engine.L, engine.h
    k = np.arange(8, dtype=np.uint64); v = np.arange(8, dtype=np.uint32); ok = np.full(8, 77, np.uint64); ov = np.full(8, 77, np.uint32)
    k32 = np.arange(8, dtype=np.uint32); ok32 = np.full(8, 77, np.uint32)
    call = lambda kb, keys, vals, n, nb, o, o2: L.telr_debug_radix_sort(h, kb, keys, vals, n, nb, o, o2)
    assert call(8, None, None, 0, 64, None, None) == TELR_OK                       # no key: no launch
    assert call(4, None, None, 0, 32, None, None) == TELR_OK
    for kb in (0, 1, 2, 16, -8):
        assert call(kb, k.ctypes.data, v.ctypes.data, 8, 8, ok.ctypes.data, ov.ctypes.data) == TELR_E_ARG
    for nb in (-1, 65):
        assert call(8, k.ctypes.data, v.ctypes.data, 8, nb, ok.ctypes.data, ov.ctypes.data) == TELR_E_ARG
    for nb in (-1, 33, 64):
        assert call(4, k32.ctypes.data, None, 8, nb, ok32.ctypes.data, None) == TELR_E_ARG
    assert call(8, None, v.ctypes.data, 8, 8, ok.ctypes.data, ov.ctypes.data) == TELR_E_ARG
    assert call(8, k.ctypes.data, None, 8, 8, ok.ctypes.data, ov.ctypes.data) == TELR_E_ARG          # 64-bit keys go with values
    assert call(8, k.ctypes.data, v.ctypes.data, 8, 8, None, ov.ctypes.data) == TELR_E_ARG
    assert call(8, k.ctypes.data, v.ctypes.data, 8, 8, ok.ctypes.data, None) == TELR_E_ARG
    assert call(4, k32.ctypes.data, v.ctypes.data, 8, 8, ok32.ctypes.data, ov.ctypes.data) == TELR_E_ARG  # 32-bit keys go without
    assert call(8, k.ctypes.data, v.ctypes.data, -1, 8, ok.ctypes.data, ov.ctypes.data) == TELR_E_ARG
    assert b"telr_debug_radix_sort: " in L.telr_last_error(h)
    assert (ok == 77).all() and (ov == 77).all() and (ok32 == 77).all()               # a refusal writes nothing
    gk, gv = engine.debug_radix_sort(k[::-1].copy(), 8, v)                               # and the context still sorts
    assert gk.tolist() == list(range(8)) and gv.tolist() == list(range(7, -1, -1))


# ---- dev_qscan --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(pc.SCAN_N))
def test_qscan_is_an_exclusive_scan(engine, n):
    """int32 -> int32, int32 -> int64 and int64 -> int64: out[0 .. n] equals the cumulative sum cast with wrap-around, tot64 the exact
    total -- the int32 output of three counts of 2^30 is negative at out[3] beside tot64 == 3 * 2^30"""
    bad = []
    for tin, tout in pc.SCAN_TYPES:
        for values in pc.SCAN_VALUES if n else ("zeros",):
            c = pc.scan_counts(n, tin, values)
            if c is None:
                continue
            want, tot = pc.scan_ref(c, tout)
            for want_tot in (True, False):
                g = engine.debug_qscan(c, tout, want_tot=want_tot)
                if not (np.array_equal(g["out"], want) and g["out"].dtype == want.dtype and g["tot64"] == (tot if want_tot else None)):
                    bad.append((np.dtype(tin).name, np.dtype(tout).name, values, want_tot))
            if values == "three_2p30":
                assert tot == 3 << 30
                assert want[3] == (-(1 << 30) if tout == np.int32 else 3 << 30)
    assert not bad, bad
    if n == 0:
        g = engine.debug_qscan(np.zeros(0, np.int32), np.int32)
        assert g["out"].tolist() == [0] and g["tot64"] == 0


@pytest.mark.parametrize("n", [n for n in sorted(pc.SCAN_N) if n > 0])
def test_qscan_reports_counts_above_the_cap(engine, n):
    """counts equal to the cap are not reported, counts of cap + 1 are: at the first and last index of the first and last tile; the
    indices as a sorted set (their order is the atomics' arrival order); the counter is cleared whatever the caller left in it"""
    for tin, tout in pc.SCAN_TYPES:
        c, over = pc.cap_counts(n, tin)
        want, tot = pc.scan_ref(c, tout)
        for n_over_in in (0, 77):
            g = engine.debug_qscan(c, tout, cap=pc.SCAN_CAP, want_n_over=True, want_list=True, n_over_in=n_over_in)
            np.testing.assert_array_equal(g["out"], want)
            assert g["tot64"] == tot and g["n_over"] == len(over)
            np.testing.assert_array_equal(np.sort(g["over_list"]), over)
        g = engine.debug_qscan(c, tout, cap=pc.SCAN_CAP, want_n_over=True, n_over_in=5)         # the counter without a list
        assert g["n_over"] == len(over) and g["over_list"] is None
        np.testing.assert_array_equal(g["out"], want)
        g = engine.debug_qscan(c, tout, cap=pc.SCAN_CAP)                                         # neither
        assert g["n_over"] is None and g["tot64"] == tot
        np.testing.assert_array_equal(g["out"], want)
        # one below: the neighbours at the cap are reported too
        g = engine.debug_qscan(c, tout, cap=pc.SCAN_CAP - 1, want_n_over=True, want_list=True)
        np.testing.assert_array_equal(np.sort(g["over_list"]), np.flatnonzero(c >= pc.SCAN_CAP))
        # no count is above its own maximum
        g = engine.debug_qscan(c, tout, cap=pc.SCAN_CAP + 1, want_n_over=True, want_list=True, n_over_in=3)
        assert g["n_over"] == 0 and len(g["over_list"]) == 0


def test_qscan_twice_gives_the_same_bytes(engine):
    c = pc.scan_counts(1048577, np.int32, "small")
    a = engine.debug_qscan(c, np.int32); b = engine.debug_qscan(c, np.int32)
    assert a["out"].tobytes() == b["out"].tobytes() and a["tot64"] == b["tot64"] == int(c.sum())


def test_qscan_tap_arguments(engine):
    L, h = engine.L, engine.h
    c = np.ones(4, np.int32); out = np.full(5, 77, np.int64); lst = np.full(4, 77, np.int32)
    call = lambda ib, ob, cnt, n, o, nov, ls: L.telr_debug_qscan(h, ib, ob, cnt, n, o, None, 0, nov, ls)
    for ib, ob in ((8, 4), (4, 2), (2, 4), (0, 0), (4, 16)):
        assert call(ib, ob, c.ctypes.data, 4, out.ctypes.data, None, None) == TELR_E_ARG
    assert call(4, 4, c.ctypes.data, -1, out.ctypes.data, None, None) == TELR_E_ARG
    assert call(4, 4, None, 4, out.ctypes.data, None, None) == TELR_E_ARG
    assert call(4, 4, c.ctypes.data, 4, None, None, None) == TELR_E_ARG
    assert call(4, 4, c.ctypes.data, 4, out.ctypes.data, None, lst.ctypes.data) == TELR_E_ARG        # a list needs its counter
    assert b"telr_debug_qscan: " in L.telr_last_error(h)
    assert (out == 77).all() and (lst == 77).all()
    assert call(4, 8, c.ctypes.data, 4, out.ctypes.data, None, None) == TELR_OK
    assert out.tolist() == [0, 1, 2, 3, 4]
