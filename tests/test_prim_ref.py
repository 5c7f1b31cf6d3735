"""tests/prim_cases.py on a CPU: every case of the sort and scan tables reaches the edge it names (tile counts, pass parity, the
one-digit tile, ties under garbage, the int32 wrap, the cap), and the two numpy references give hand-worked answers."""
import numpy as np
import pytest

import prim_cases as pc


# ---- the sort table ---------------------------------------------------------------------------------------------------------------------
def test_sort_counts_reach_their_tile_edges():
    for n, t in pc.SORT_N.items():
        assert pc.tiles(n) == t, n
    ts = set(pc.SORT_N.values())
    assert {1, 2, 3, 256, 257} <= ts
    # 2,048 k +- 1 for k = 1 and k = 256; a thread of k_rs_scan owns one row entry up to 256 tiles and two from 257 on
    assert {2047, 2048, 2049, 524288 - 0, 524288 + 1} <= set(pc.SORT_N) and 524288 == 256 * pc.RS_TILE
    per = lambda n: (pc.tiles(n) + pc.RS_ROW - 1) // pc.RS_ROW
    assert per(524288) == 1 and per(524289) == 2 and per(599999) == 2
    assert 599999 % 2 == 1 and 599999 % pc.RS_TILE not in (0, 1, pc.RS_TILE - 1)
    # the wave and workgroup sizes
    assert {63, 64, 65, 255, 256, 257} <= set(pc.SORT_N)


def test_sort_widths_reach_both_parities():
    for bits, tab in pc.SORT_NBITS.items():
        for nb, p in tab.items():
            assert pc.passes(nb) == p and 0 <= nb <= bits
            assert pc.sort_mask(nb) == (1 << (8 * p)) - 1
        assert {0, bits} <= set(tab)
    assert set(pc.SORT_NBITS[64].values()) == set(range(9))              # 0 .. 8 passes
    for bits in (64, 32):                                                # the large counts keep an odd and an even pass count
        assert {pc.passes(nb) % 2 for nb in pc.SORT_NBITS_LARGE[bits]} == {0, 1}
        assert set(pc.SORT_NBITS_LARGE[bits]) <= set(pc.SORT_NBITS[bits])
    assert {"equal", "two_digits", "high_bit"} <= set(pc.SORT_PATTERNS_LARGE) <= set(pc.SORT_PATTERNS)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n", sorted(pc.SORT_N))
def test_sort_cases_are_what_they_claim(bits, n):
    full = (1 << bits) - 1
    seen = set()
    for name, nb, pat in pc.sort_cases(bits, n):
        k = pc.sort_keys(bits, n, nb, pat)
        assert k.dtype == (np.uint64 if bits == 64 else np.uint32) and len(k) == n, name
        np.testing.assert_array_equal(k, pc.sort_keys(bits, n, nb, pat))                  # the same keys at every call
        seen.add(pat)
        w = 8 * pc.passes(nb)
        masked = k.astype(np.uint64) & np.uint64(pc.sort_mask(nb) & full)
        if pat == "equal":
            # every full tile holds 2,048 equal digits in every pass
            for p in range(pc.passes(nb)):
                d = pc.digits(k, p)
                assert (d == d[0]).all() and d[0] != 0, name
            assert int(k[0]) >> (bits - 1) == 1
        elif pat == "ascending" and n > 1:
            assert (np.diff(k.astype(np.int64)) == 1).all()
        elif pat == "descending" and n > 1:
            assert (np.diff(k.astype(np.int64)) == -1).all()
        elif pat == "two_digits":
            for p in range(pc.passes(nb)):
                np.testing.assert_array_equal(pc.digits(k, p), (np.arange(n) & 1) * 255, err_msg=name)
        elif pat == "digit_cycle":
            for p in range(pc.passes(nb)):
                np.testing.assert_array_equal(pc.digits(k, p), np.arange(n) & 255, err_msg=name)
        elif pat == "high_bit" and n >= 2:
            top = (k.astype(np.uint64) >> np.uint64(bits - 1)).astype(np.int64)
            assert abs(int(top.sum()) - n // 2) <= 1 and top.min() == 0 and top.max() == 1, name
        elif pat == "confined":
            assert nb == 64 or int(k.max()) < (1 << nb), name
            assert n < 64 or nb == 0 or int(k.max()) >= (1 << (nb - 1)) // 2, name
        elif pat == "garbage" and w < bits and n >= 64:
            # two equal masked keys with different upper bits: in one tile, and (with more than one tile) in two tiles
            up = k.astype(np.uint64) >> np.uint64(w)
            t0 = slice(0, min(n, pc.RS_TILE))
            assert any(len(set(up[t0][masked[t0] == m].tolist())) >= 2 for m in np.unique(masked[t0])), name
            if pc.tiles(n) >= 2:
                first, last = slice(0, pc.RS_TILE), slice((pc.tiles(n) - 1) * pc.RS_TILE, n)
                assert any((masked[first] == m).any() and (masked[last] == m).any() and
                           set(up[first][masked[first] == m].tolist()) != set(up[last][masked[last] == m].tolist()) for m in np.unique(masked[last])), name
    assert seen == set(pc.SORT_PATTERNS_LARGE if n >= pc.SORT_N_LARGE else pc.SORT_PATTERNS)


def test_sort_ref_by_hand():
    # by the low byte only (nbits 1 .. 8): 0x1ff and 0x0ff tie and keep their order; the values are the permutation
    k = np.array([0x2FF, 0x100, 0x1FF, 0x001, 0x300], np.uint64)
    for nb in (1, 7, 8):
        gk, gv = pc.sort_ref(k, nb, np.arange(5, dtype=np.uint32))
        assert gk.tolist() == [0x100, 0x300, 0x001, 0x2FF, 0x1FF] and gv.tolist() == [1, 4, 3, 0, 2]
    # by two bytes (nbits 9 .. 16)
    gk, gv = pc.sort_ref(k, 9, np.arange(5, dtype=np.uint32))
    assert gk.tolist() == [0x001, 0x100, 0x1FF, 0x2FF, 0x300] and gv.tolist() == [3, 1, 2, 0, 4]
    # no pass: the input
    gk, gv = pc.sort_ref(k, 0, np.arange(5, dtype=np.uint32))
    assert gk.tolist() == k.tolist() and gv.tolist() == [0, 1, 2, 3, 4]
    # bit 63 / bit 31 sort as unsigned
    gk, _ = pc.sort_ref(np.array([1 << 63, 5, (1 << 63) + 1, 0], np.uint64), 64)
    assert gk.tolist() == [0, 5, 1 << 63, (1 << 63) + 1]
    gk, gv = pc.sort_ref(np.array([1 << 31, 5, 0xFFFFFFFF, 0], np.uint32), 32)
    assert gk.tolist() == [0, 5, 1 << 31, 0xFFFFFFFF] and gv is None and gk.dtype == np.uint32


def test_sort_ref_is_stable_on_a_garbage_case():
    k = pc.sort_keys(64, 4097, 16, "garbage")
    gk, gv = pc.sort_ref(k, 16, np.arange(len(k), dtype=np.uint32))
    m = gk & np.uint64(0xFFFF)
    assert (np.diff(m.astype(np.int64)) >= 0).all()
    assert sorted(gv.tolist()) == list(range(len(k)))
    same = m[1:] == m[:-1]
    assert same.any() and (np.diff(gv.astype(np.int64))[same] > 0).all()            # ties in input order
    np.testing.assert_array_equal(gk, k[gv])                                        # every key with its own upper bits


# ---- the scan table ---------------------------------------------------------------------------------------------------------------------
def test_scan_counts_reach_their_tile_edges():
    for n, t in pc.SCAN_N.items():
        assert pc.scan_tiles(n) == t, n
    assert {0, 4095, 4096, 4097, 256 * pc.QSCAN_TILE, 256 * pc.QSCAN_TILE + 1} <= set(pc.SCAN_N)
    assert {15, 16, 17} <= set(pc.SCAN_N) and pc.QSCAN_TILE // pc.QSCAN_ROW == 16       # a thread's sixteen counts
    assert {255, 256, 257} <= set(pc.SCAN_N)
    # the loop over the tile sums: one step up to 256 tiles, a second from 257
    assert {(t + pc.QSCAN_ROW - 1) // pc.QSCAN_ROW for t in pc.SCAN_N.values()} == {1, 2}


def test_scan_ref_by_hand():
    out, tot = pc.scan_ref(np.array([3, 0, 4], np.int32), np.int32)
    assert out.tolist() == [0, 3, 3, 7] and tot == 7 and out.dtype == np.int32
    out, tot = pc.scan_ref(np.zeros(0, np.int32), np.int64)
    assert out.tolist() == [0] and tot == 0
    # three counts of 2^30: the int32 scan wraps at out[3], the 64-bit one and the total do not
    c = pc.scan_counts(17, np.int32, "three_2p30")
    o32, tot = pc.scan_ref(c, np.int32)
    o64, _ = pc.scan_ref(c, np.int64)
    assert o32[:4].tolist() == [0, 1 << 30, -(1 << 31), -(1 << 30)] and o32[3] < 0 and o32[-1] == -(1 << 30)
    assert o64[:4].tolist() == [0, 1 << 30, 1 << 31, 3 << 30] and tot == 3 << 30 == int(o64[-1])
    # 64-bit counts above 2^32
    c = pc.scan_counts(16, np.int64, "above_2p32")
    out, tot = pc.scan_ref(c, np.int64)
    assert c.max() > 1 << 32 and tot == int(c.sum()) == int(out[-1]) and tot > 1 << 33


def test_scan_cases_are_what_they_claim():
    for n in pc.SCAN_N:
        for tin, tout in pc.SCAN_TYPES:
            have = set()
            for v in pc.SCAN_VALUES:
                c = pc.scan_counts(n, tin, v)
                if c is None:
                    continue
                have.add(v)
                assert c.dtype == tin and len(c) == n and (c >= 0).all()
                if v.startswith("one_at"):
                    assert np.count_nonzero(c) == 1
            assert {"zeros", "ones", "small"} <= have
            if n >= 3:
                assert "three_2p30" in have
            if n >= 4097:
                assert {"one_at_0", "one_at_4095", "one_at_4096", "one_at_last"} <= have
            if n >= 1 and tin == np.int64:
                assert "above_2p32" in have


@pytest.mark.parametrize("n", [n for n in sorted(pc.SCAN_N) if n > 0])
def test_cap_cases_sit_on_the_cap(n):
    c, over = pc.cap_counts(n, np.int32)
    np.testing.assert_array_equal(np.flatnonzero(c > pc.SCAN_CAP), over)
    assert (c[over] == pc.SCAN_CAP + 1).all()
    assert 0 in over and n - 1 in over
    if n > 2:
        assert (c == pc.SCAN_CAP).any()                    # counts equal to the cap stand beside them and are not reported
    if n >= 4097:
        last0 = (pc.scan_tiles(n) - 1) * pc.QSCAN_TILE
        assert {0, 4095, 4096, last0, n - 1} <= set(over.tolist())
