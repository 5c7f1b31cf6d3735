"""The oracle's problem-list entry (tor_debug_dp), which tests/test_gpu_dp_edges.py holds the engine's DP classes to, checked
against the oracle's own single-problem entries and against a plain numpy int64 banded DP; and the engine library's int16
bounds (telr_debug_dp_limits) for the five presets.  CPU only."""
import numpy as np
import pytest

from oracle import binding as ob
from telr_amd.aligner import Engine
from telr_amd.presets import preset
import dp_edges as de

NEG = -(1 << 40)
LUT = np.full(256, 4, np.int64)
for _i, _c in enumerate(b"ACGT"):
    LUT[_c] = _i


def ref_band_dp(A, B, dlo, dhi, a, b, q, e, q2, e2, amb):
    """H of every cell of the band dlo <= j - i <= dhi (NEG outside it) of the global DP of nt4 arrays A (query) and B
    (target): match a, mismatch -b, -amb on any N, a gap of L bases costs min(q + e L, q2 + e2 L)"""
    m, n = len(A), len(B)
    S = np.where((A[:, None] > 3) | (B[None, :] > 3), -amb, np.where(A[:, None] == B[None, :], a, -b)).astype(np.int64)
    j = np.arange(n + 1, dtype=np.int64)
    H = np.full((m + 1, n + 1), NEG, np.int64)
    best_up1 = np.full(n + 1, NEG, np.int64)        # max over rows k < i of H[k, j] + e * k, per gap piece
    best_up2 = np.full(n + 1, NEG, np.int64)
    for i in range(m + 1):
        inb = (j - i >= dlo) & (j - i <= dhi)
        h = np.full(n + 1, NEG, np.int64)
        if i == 0:
            h[0] = 0
        else:
            h[1:] = H[i - 1, :-1] + S[i - 1]
            h = np.maximum(h, np.maximum(best_up1 - q - e * i, best_up2 - q2 - e2 * i))
        h = np.where(inb, np.maximum(h, NEG), NEG)
        # gaps along the row: opened from any earlier cell of the row (a gap that starts where another ends never wins)
        for ee, qq in ((e, q), (e2, q2)):
            pm = np.maximum.accumulate(h + ee * j)
            left = np.concatenate([[NEG], pm[:-1]])
            h = np.where(inb, np.maximum(h, left - qq - ee * j), NEG)
        h = np.where(h < NEG // 2, NEG, h)
        H[i] = h
        best_up1 = np.maximum(best_up1, np.where(h > NEG, h + e * i, NEG))
        best_up2 = np.maximum(best_up2, np.where(h > NEG, h + e2 * i, NEG))
    return H


def _affine_sets():
    """every preset's affine scoring (the convex presets: their two-piece envelope) and the edge of the int16 acceptance"""
    out = []
    for p in de.PRESETS:
        mo = preset(p)[1]
        mo.cx_scale = 0
        out.append((p, mo))
    mo = preset("map-ont")[1]
    mo.a, mo.b, mo.q, mo.e, mo.q2, mo.e2, mo.sc_ambi = 4, 9, 4, 2, 63, 1, 9
    out.append(("affine-edge", mo))
    return out


def _seq_pair(rng, m, n, style):
    B = de._rand(rng, n)
    if style == "homopolymer":
        return np.full(m, ord("A"), np.uint8), np.full(n, ord("A"), np.uint8)
    A = de._fit(rng, de._mutate(rng, B, float(rng.uniform(0.0, 0.3))), m).copy()
    if style == "n":
        A[rng.random(m) < 0.05] = ord("N")
        B[rng.random(n) < 0.05] = ord("N")
    return A, B


def _problems(rng, count, kind, mo, maxlen=200):
    qs, ts, rows = [], [], []
    for x in range(count):
        style = ("random", "n", "homopolymer")[x % 3]
        if kind == 0:
            m, n = int(rng.integers(1, maxlen + 1)), int(rng.integers(1, maxlen + 1))
            lo, hi = de.fill_band(m, n, int(rng.integers(0, 40)))
        else:
            m = int(rng.integers(1, min(maxlen, mo.ext_max) + 1))
            n = int(rng.integers(1, m + mo.ext_band + 1))
            lo, hi = de.ext_band(mo)
        A, B = _seq_pair(rng, m, n, style)
        qs.append(A.tobytes())
        ts.append(B.tobytes())
        rows.append((x, 0, x, 0, m, n, lo, hi, kind, 1, 1, 0))
    return qs, ts, np.array(rows, np.int32)


@pytest.mark.parametrize("name", de.PRESETS)
def test_problem_list_entry_equals_single_problem_entries(name):
    import ctypes as C
    mo = preset(name)[1]
    L = ob.lib()
    rng = np.random.default_rng(7)
    for _ in range(12):
        m, n = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        A, B = _seq_pair(rng, m, n, "random")
        cig = np.zeros(2 * (m + n) + 8, np.uint32)
        nc = C.c_int32(0)
        sc = L.tor_nw(A.tobytes(), m, B.tobytes(), n, C.byref(mo), cig.ctypes.data, C.byref(nc), len(cig))
        lo, hi = de.fill_band(m, n, min(2 + ((mo.fill_band_q4 if mo.fill_band_q4 > 0 else 8) * int(np.sqrt(min(m, n))) >> 4), mo.bw))
        r = ob.debug_dp([A.tobytes()], [B.tobytes()], mo, [(0, 0, 0, 0, m, n, lo, hi, 0, 1, 1, 0)])
        assert r["score"][0] == sc and r["bi"][0] == m and r["bj"][0] == n
        np.testing.assert_array_equal(r["cigars"][0], cig[:nc.value])
        # extension
        qe, te = C.c_int32(0), C.c_int32(0)
        sc = L.tor_ext(A.tobytes(), m, B.tobytes(), n, C.byref(mo), cig.ctypes.data, C.byref(nc), len(cig), C.byref(qe), C.byref(te))
        mq = min(m, mo.ext_max)
        mt = min(n, mq + mo.ext_band)
        lo, hi = de.ext_band(mo)
        r = ob.debug_dp([A.tobytes()], [B.tobytes()], mo, [(0, 0, 0, 0, mq, mt, lo, hi, 2, 1, 1, 0)])
        assert (r["score"][0], r["bi"][0], r["bj"][0]) == (sc, qe.value, te.value)
        np.testing.assert_array_equal(r["cigars"][0], cig[:nc.value])


def test_problem_list_entry_reads_both_strands():
    """a problem stored reversed and complemented (qstep / tstep -1, qcomp) is the same DP as the forward one"""
    mo = preset("map-ont")[1]
    rng = np.random.default_rng(11)
    qs, ts, rows = _problems(rng, 30, 0, mo)
    fwd = ob.debug_dp(qs, ts, mo, rows)
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    qr = [q[::-1].translate(comp) for q in qs]
    tr = [t[::-1] for t in ts]
    rrows = rows.copy()
    rrows[:, 1] = rows[:, 4] - 1
    rrows[:, 3] = rows[:, 5] - 1
    rrows[:, 9] = -1
    rrows[:, 10] = -1
    rrows[:, 11] = 1
    rev = ob.debug_dp(qr, tr, mo, rrows)
    for k in ("score", "bi", "bj", "touched"):
        np.testing.assert_array_equal(fwd[k], rev[k], err_msg=k)
    for a, b in zip(fwd["cigars"], rev["cigars"]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name,mo", _affine_sets(), ids=[n for n, _ in _affine_sets()])
def test_oracle_fill_equals_numpy_int64_dp(name, mo):
    rng = np.random.default_rng(sum(name.encode()))
    qs, ts, rows = _problems(rng, 50, 0, mo)
    r = ob.debug_dp(qs, ts, mo, rows)
    for x in range(len(rows)):
        m, n, lo, hi = (int(v) for v in rows[x, 4:8])
        H = ref_band_dp(LUT[np.frombuffer(qs[x], np.uint8)], LUT[np.frombuffer(ts[x], np.uint8)], lo, hi,
                        mo.a, mo.b, mo.q, mo.e, mo.q2, mo.e2, mo.sc_ambi)
        assert r["score"][x] == H[m, n], (name, x, m, n, lo, hi)
        assert (r["bi"][x], r["bj"][x]) == (m, n)


@pytest.mark.parametrize("name,mo", _affine_sets(), ids=[n for n, _ in _affine_sets()])
def test_oracle_extension_without_zdrop_is_the_band_maximum(name, mo):
    mo.zdrop = 1 << 28
    rng = np.random.default_rng(5 + sum(name.encode()))
    qs, ts, rows = _problems(rng, 25, 1, mo)
    r = ob.debug_dp(qs, ts, mo, rows)
    for x in range(len(rows)):
        lo, hi = (int(v) for v in rows[x, 6:8])
        H = ref_band_dp(LUT[np.frombuffer(qs[x], np.uint8)], LUT[np.frombuffer(ts[x], np.uint8)], lo, hi,
                        mo.a, mo.b, mo.q, mo.e, mo.q2, mo.e2, mo.sc_ambi)
        best = max(0, int(H.max()))
        assert r["score"][x] == best, (name, x)
        if best > 0:
            assert H[r["bi"][x], r["bj"][x]] == best


# the engine's int16 bounds for the presets (telr_engine.hip: dp_limits; TELR_AB unset)
PRESET_LIMITS = {
    "map-ont": (7822, 7374, 1024, 7854, 64, 3, 1889, 909),
    "map-pb": (7822, 7374, 1024, 7854, 64, 3, 1889, 909),
    "asm10": (3471, 3272, 1024, 3485, 64, 3, 835, 399),
    "ngmlr-ont": (7900, 7900, 512, 7900, 128, 0, 3782, 0),
    "ngmlr-pacbio": (7900, 7900, 256, 7900, 64, 0, 1484, 0),
}


def _limits_restated(mo):
    """the affine bounds, restated from their comments: |H| <= b (m + n) / 2 + q2 + D e2 and a (m + n) / 2 inside +-16000"""
    b, a = max(mo.b, 1), max(mo.a, 1)
    lim = lambda hb, D, ha: max(0, min(2 * (hb - mo.q2 - D * mo.e2) // b - 2, ha // a - 2))
    d = de.d_onep_d(mo.q, mo.e, mo.q2, mo.e2)
    ext_d = 64 if 2 * mo.ext_band + 2 <= 64 else 128 if 2 * mo.ext_band + 2 <= 128 else 256
    return (lim(15800, 128, 32000), lim(15800, 1024, 32000), 1024, lim(15800, ext_d, 32000) if mo.zdrop <= 4000 else 0,
            ext_d if mo.zdrop <= 4000 else 64, (d >= 16) | (d >= 20) << 1,
            max(0, min(2 * (3850 - mo.q - 32 * mo.e) // b - 2, 7700 // a - 2)), lim(1975, 128, 4000))


@pytest.mark.parametrize("name", de.PRESETS)
def test_dp_limits_of_the_presets(name):
    mo = preset(name)[1]
    got = Engine.dp_limits(mo)
    assert tuple(got[k] for k in Engine.DP_LIMITS) == PRESET_LIMITS[name]
    if mo.cx_scale == 0:
        assert tuple(got[k] for k in Engine.DP_LIMITS) == _limits_restated(mo)


def test_dp_limits_edges_of_the_affine_acceptance():
    mo = preset("map-ont")[1]
    mo.a, mo.b, mo.q, mo.e, mo.q2, mo.e2, mo.sc_ambi = 4, 9, 4, 2, 63, 1, 9
    assert Engine.dp_limits(mo)["pk_steps_limit"] == _limits_restated(mo)[0] > 0
    for f, v in (("a", 5), ("b", 10), ("q2", 64), ("sc_ambi", 10)):
        m2 = mo.copy()
        setattr(m2, f, v)
        assert Engine.dp_limits(m2)["pk_steps_limit"] == 0, f
    for z, on in ((4000, True), (4001, False)):
        m2 = preset("map-ont")[1]
        m2.zdrop = z
        assert (Engine.dp_limits(m2)["pk_ext_limit"] > 0) == on


def test_dp_class_table():
    """the engine's class table (kernels.hip.h: DP_CLASS) against this suite's own statement of the classes (dp_edges) and
    against the dwords per trace-back row as the kernels had them before the table (literals)"""
    T = Engine.dp_class_table()
    col = {k: T[:, x] for x, k in enumerate(Engine.DP_CLASS_COLUMNS)}
    assert T.shape == (25, 6)
    assert {c: int(col["maxd"][c]) for c in range(25)} == {**de.UPPER_D, 4: 4096}
    assert {c for c in range(25) if col["interleaved"][c]} == set(de.INTERLEAVED)
    assert {c for c in range(25) if col["tiled"][c]} == {18, 23, 24}
    for c in (10, 11, 12, 13, 14, 15, 16, 17, 22):
        assert col["row_dwords"][c] == col["lanes"][c] * col["regs"][c], c
    row_dwords = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 32, 6: 64, 7: 128, 8: 256, 9: 512, 10: 5, 11: 6, 12: 7, 13: 8, 14: 10, 15: 12,
                  16: 16, 17: 4, 18: 16, 19: 64, 20: 128, 21: 256, 22: 32, 23: 32, 24: 64}
    assert {c: int(col["row_dwords"][c]) for c in range(25)} == row_dwords
