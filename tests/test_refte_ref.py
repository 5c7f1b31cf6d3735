"""The reference TE annotation without a device: the plain-Python definition (tests/refte_ref.py) against hand-derived
answers and against the edge every case of tests/refte_cases.py claims; telr_tile_plan through the library against the definition, its
error codes and the covering property by brute force; and the planted reference -- tiles mapped with the CPU oracle, features that must
equal the planted intervals exactly."""
import ctypes as C

import numpy as np
import pytest

import refte_cases as rc
import refte_ref as ref
from telr_amd import _lib
from telr_amd._abi import MF_CIGAR, TELR_E_ARG, TELR_E_RANGE, TILE_DTYPE
from telr_amd.aligner import Engine
from telr_amd.presets import preset


def tiles_of(c):
    return [tuple(int(x) for x in t) for t in c["tiles"]]


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def test_features_by_hand():
    # [0,100) [10,20) [50,60) [100,110): two features under join_gap 0 (the running maximum keeps [50,60) inside), one under join_gap 1
    h = [(0, 0, 100, 0, 0, 4), (0, 10, 20, 0, 0, 3), (0, 50, 60, 0, 0, 2), (0, 100, 110, 0, 0, 1)]
    assert ref.features(h, dict(join_gap=0)) == [(0, 0, 100, 0, 0, 4, 3), (0, 100, 110, 0, 0, 1, 1)]
    assert ref.features(h, dict(join_gap=1)) == [(0, 0, 110, 0, 0, 4, 4)]
    assert ref.features_previous_end(h, dict(join_gap=0)) >= 3
    # the output order is (tid, start, end, family, strand), not the hits' run order
    h = [(0, 500, 600, 1, 0, 1), (0, 100, 200, 1, 1, 2), (0, 100, 200, 0, 1, 3), (1, 0, 50, 0, 0, 4), (0, 100, 150, 1, 1, 5)]
    assert ref.features(h) == [(0, 100, 200, 0, 1, 3, 1), (0, 100, 200, 1, 1, 5, 2), (0, 500, 600, 1, 0, 1, 1), (1, 0, 50, 0, 0, 4, 1)]
    assert ref.features([]) == []


def test_hits_by_hand():
    tiles = [(0, 0, 4096), (0, 2048, 4096), (1, 0, 300)]
    alns = [dict(qid=1, qs=10, qe=210, tid=2, flags=1 | 8, mapq=0, dp_score=77), dict(qid=2, qs=0, qe=300, tid=0, flags=4, mapq=3, dp_score=5),
            dict(qid=0, qs=0, qe=99, tid=0, flags=1, mapq=60, dp_score=1), dict(qid=0, qs=0, qe=500, tid=0, flags=2, mapq=60, dp_score=1)]
    assert ref.hits(alns, tiles) == [(0, 2058, 2258, 2, 1, 77), (1, 0, 300, 0, 0, 5)]
    assert ref.hits(alns, tiles, dict(min_mapq=1)) == [(1, 0, 300, 0, 0, 5)]
    for bad in (dict(qid=3, qs=0, qe=1), dict(qid=-1, qs=0, qe=1), dict(qid=2, qs=0, qe=301), dict(qid=0, qs=5, qe=4), dict(qid=0, qs=-1, qe=4)):
        with pytest.raises(ValueError):
            ref.hits([dict(dict(tid=0, flags=1, mapq=0, dp_score=0), **bad)], tiles)


@pytest.mark.parametrize("c", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_case_meets_the_edge_it_claims(c):
    h = ref.hits(c["alns"], tiles_of(c), c["opt"])
    got = ref.features(h, c["opt"])
    assert len(got) == c["n_expect"]
    if c["expect"] is not None:
        assert got == c["expect"]
    if c["name"].startswith("running maximum, join_gap 0"):
        assert ref.features_previous_end(h, c["opt"]) >= 3


def test_the_cases_cover_what_they_should():
    names = [c["name"] for c in rc.CASES]
    assert len(set(names)) == len(names) and len(rc.SMALL) >= 10
    for k in (63, 64, 65, 255, 256, 257, 4097):
        assert "long hit over %d short ones" % k in names
    for b in (64, 256):
        assert "run boundary at %d|%d" % (b - 1, b) in names
    for n in (4095, 4096, 4097):
        assert "%d single-hit features" % n in names
    assert "run boundary at 4095|4096, 5000 later hits" in names and "run boundary at 4999|5000, 9000 later hits" in names


# ---- the tile plan through the library --------------------------------------------------------------------------------------------------
def plan_lengths(tile, stride):
    return [0, 1, stride - 1, stride, stride + 1, tile - 1, tile, tile + 1, tile + stride, tile + stride + 1]


PAIRS = [(48, 16), (40, 40), (37, 11)]


@pytest.mark.parametrize("tile,stride", PAIRS)
def test_tile_plan_equals_the_definition(tile, stride):
    lengths = plan_lengths(tile, stride)
    for ls in [[n] for n in lengths] + [lengths, lengths[::-1], [5 * tile + 3, 0, 0, 1, 3 * stride]]:
        got = Engine.tile_plan(ls, tile, stride)
        assert got.dtype == TILE_DTYPE
        assert [tuple(int(x) for x in t) for t in got] == ref.tile_plan(ls, tile, stride)


def test_tile_plan_by_hand():
    # 100 bases, tile 48, stride 16: 1 + ceil(52 / 16) = 5 tiles; the last one holds the 36 bases from 64 on
    assert ref.tile_plan([100], 48, 16) == [(0, 0, 48), (0, 16, 48), (0, 32, 48), (0, 48, 48), (0, 64, 36)]
    assert ref.tile_plan([0, 48, 49], 48, 16) == [(1, 0, 48), (2, 0, 48), (2, 16, 33)]
    assert ref.tile_plan([81], 40, 40) == [(0, 0, 40), (0, 40, 40), (0, 80, 1)]


@pytest.mark.parametrize("tile,stride", PAIRS)
def test_every_short_interval_lies_in_a_tile_and_no_tile_in_another(tile, stride):
    for n in plan_lengths(tile, stride) + [3 * tile + 5]:
        tiles = ref.tile_plan([n], tile, stride)
        span = tile - stride + 1
        for a in range(n):
            for b in range(a + 1, min(n, a + span) + 1):
                assert any(s <= a and b <= s + l for _, s, l in tiles), (n, a, b)
        for i, (_, s, l) in enumerate(tiles):
            for j, (_, s2, l2) in enumerate(tiles):
                assert i == j or not (s2 <= s and s + l <= s2 + l2), (n, i, j)
        assert not tiles or (tiles[-1][1] + tiles[-1][2] == n and all(l >= 1 for _, _, l in tiles))


def call_plan(lengths, tile, stride, cap, with_out=True, with_needed=True, with_len=True):
    L = _lib.lib()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    out = np.full(max(cap, 1), -7, TILE_DTYPE)
    need = C.c_int64(-1)
    rcode = L.telr_tile_plan(len(a), a.ctypes.data if with_len else None, tile, stride, out.ctypes.data if with_out else None, cap,
                             C.byref(need) if with_needed else None)
    return rcode, need.value, out


def test_tile_plan_error_codes():
    assert call_plan([100], 48, 16, 5)[:2] == (0, 5)
    for tile, stride in ((0, 1), (-1, 1), (48, 0), (48, -3), (48, 49), (1 << 24, 16), ((1 << 24) + 5, 16)):
        assert call_plan([100], tile, stride, 64)[0] == TELR_E_ARG, (tile, stride)
    assert call_plan([100], (1 << 24) - 1, 16, 64)[:2] == (0, 1)
    assert call_plan([100, -1], 48, 16, 64)[0] == TELR_E_ARG
    assert call_plan([100], 48, 16, 5, with_out=False)[0] == TELR_E_ARG
    assert call_plan([100], 48, 16, 5, with_needed=False)[0] == TELR_E_ARG
    assert call_plan([100], 48, 16, 5, with_len=False)[0] == TELR_E_ARG
    # cap / needed: nothing is copied when the tiles do not fit
    code, need, out = call_plan([100], 48, 16, 4)
    assert (code, need) == (TELR_E_RANGE, 5) and (out["tid"] == -7).all()
    code, need, _ = call_plan([100], 48, 16, 0, with_out=False)
    assert (code, need) == (TELR_E_RANGE, 5)
    assert call_plan([], 48, 16, 0, with_out=False, with_len=False)[:2] == (0, 0)
    # 2^31 - 16 tiles and more: 2^31 - 1 bases in tiles of 1 base is 2^31 - 1 tiles; sixteen bases fewer stay below
    assert call_plan([0x7fffffff], 1, 1, 0, with_out=False)[0] == TELR_E_RANGE
    assert call_plan([0x7fffffff - 16], 1, 1, 0, with_out=False)[:2] == (TELR_E_RANGE, 0x7fffffff - 16)          # (fits the count; cap 0 does not hold it)
    assert call_plan([0x7ffffff0], 1, 1, 0, with_out=False)[1] == -1                                              # refused before `needed` is written
    with pytest.raises(_lib.TelrError) as e:
        Engine.tile_plan([100], 48, 49)
    assert e.value.code == TELR_E_ARG


# ---- the planted reference, mapped with the CPU oracle ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_records():
    from oracle import binding as ob
    P = rc.planted()
    tiles = ref.tile_plan([len(P["ref"])], rc.PLANT_TILE, rc.PLANT_STRIDE)
    io, mo = preset("map-ont")
    mo = mo.copy(); mo.bw_long = 0; mo.secondary = 0; mo.flags |= MF_CIGAR
    res = ob.OracleIndex(P["lib_seqs"], io).map([P["ref"][s:s + l] for _, s, l in tiles], mo)
    return P, tiles, res["alns"]


def test_planted_reference_comes_back_exactly(planted_records):
    P, tiles, alns = planted_records
    assert len(tiles) == 14 and any(s == 4096 for _, s, _ in tiles)
    h = ref.hits(alns, tiles)
    seen = {p: sum(1 for x in h if x[1] < p[1] and x[2] > p[0] and (x[3], x[4]) == p[2:]) for p in P["plants"]}
    print("hits per plant:", seen)
    got = [(f[1], f[2], f[3], f[4]) for f in ref.features(h, dict(join_gap=0))]
    assert got == P["plants"]
    assert (36000, 37200, 2, 0) in got and (37200, 38400, 2, 0) in got          # the book-ended copies stay apart
    got1 = [(f[1], f[2], f[3], f[4]) for f in ref.features(h, dict(join_gap=1))]
    assert got1 == rc.planted_joined(P["plants"]) and (36000, 38400, 2, 0) in got1 and len(got1) == len(got) - 1
    assert all(f[0] == 0 and f[6] >= 1 for f in ref.features(h))
