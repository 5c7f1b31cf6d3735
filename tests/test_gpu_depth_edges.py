"""telr_depth_medians at the edges of k_depth_diff and k_depth_median (tests/depth_cases.py): engine == the plain definition
(tests/depth_ref.py) == the oracle == the hand-worked medians, exactly -- every value is an integer or a half; NaN positions are
compared separately.  And what the entry refuses: a record or a CIGAR that would leave its target's slice of the depth array comes
back as TELR_E_ARG with a reason and an untouched output, and the context still answers afterwards."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import depth_ref as ref
from telr_amd._abi import TELR_E_ARG, TELR_OK

pytestmark = pytest.mark.gpu

CASES = dc.cases() + [dc.GOOD]
UNTOUCHED = -12345.0


def same(got, want):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def make_result(engine, alns, cig, resident=False):
    r = C.c_void_p()
    if resident:
        import torch
        t = torch.from_numpy(cig.view(np.int32).copy()).to("cuda:0")
        torch.cuda.synchronize()
        engine._chk(engine.L.telr_result_from_device_cigars(engine.h, alns.ctypes.data, len(alns), C.c_void_p(t.data_ptr() if len(cig) else 0), len(cig), C.byref(r)),
                    "telr_result_from_device_cigars")
    else:
        engine._chk(engine.L.telr_result_from_arrays(engine.h, alns.ctypes.data, len(alns), cig.ctypes.data, len(cig), C.byref(r)), "telr_result_from_arrays")
    return r


def medians(engine, alns, cig, tl, t, s, e, resident=False):
    """-> (return code, the output array -- UNTOUCHED where the entry wrote nothing --, the context's error text)"""
    r = make_result(engine, alns, cig, resident)
    out = np.full(max(len(t), 1), UNTOUCHED, np.float64)
    try:
        rc = engine.L.telr_depth_medians(engine.h, r, len(tl), tl.ctypes.data, len(t), t.ctypes.data, s.ctypes.data, e.ctypes.data, out.ctypes.data)
    finally:
        engine.L.telr_result_free(r)
    return rc, out[:len(t)], engine.L.telr_last_error(engine.h).decode()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_depth_medians_at_the_edge(engine, c):
    from oracle import binding as ob
    alns, cig, tl, t, s, e = dc.arrays(c)
    want = dc.want_array(c)
    same(ref.depth_medians(alns, cig, tl, t, s, e), want)
    same(ob.depth_medians(alns, cig, tl, t, s, e), want)
    for resident in (False, True):
        rc, got, err = medians(engine, alns, cig, tl, t, s, e, resident)
        assert rc == TELR_OK, err
        same(got, want)


REFUSALS = dc.refusals()


@pytest.mark.parametrize("c", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_depth_medians_refuses(engine, c):
    name, tlens, recs, iv, why = c
    alns, cig, tl, t, s, e = dc.arrays(dict(recs=recs, iv=iv, tlens=tlens))
    for resident in (False, True):
        rc, got, err = medians(engine, alns, cig, tl, t, s, e, resident)
        assert rc == TELR_E_ARG
        assert err.startswith("telr_depth_medians: ") and why in err, err
        assert (got == UNTOUCHED).all()
        # the context is still usable: a well-formed call gives the definition's medians
        a2, c2, tl2, t2, s2, e2 = dc.arrays(dc.GOOD)
        rc, got, err = medians(engine, a2, c2, tl2, t2, s2, e2, resident)
        assert rc == TELR_OK, err
        same(got, ref.depth_medians(a2, c2, tl2, t2, s2, e2))
        same(got, dc.want_array(dc.GOOD))


def test_depth_medians_refuses_a_negative_target_length(engine):
    alns, cig, tl, t, s, e = dc.arrays(dc.GOOD)
    tl = tl.copy(); tl[1] = -1
    alns = alns[:1].copy()                                        # (the record on target 0 alone)
    rc, got, err = medians(engine, alns, cig, tl, t, s, e)
    assert rc == TELR_E_ARG and err.startswith("telr_depth_medians: target 1: negative length") and (got == UNTOUCHED).all()


def test_index_depth_medians_raises_with_the_reason(engine):
    """the same refusal through Index.depth_medians, as telr_af.py reaches the entry"""
    from telr_amd import _lib
    from telr_amd.presets import preset
    name, tlens, recs, iv, why = [r for r in REFUSALS if r[0] == "cigar_beyond_te_M"][0]
    alns, cig, tl, t, s, e = dc.arrays(dict(recs=recs, iv=iv, tlens=tlens))
    rng = np.random.default_rng(5)
    io, _ = preset("map-ont")
    ix = engine.index(["".join("ACGT"[x] for x in rng.integers(0, 4, L)) for L in tlens], io)
    try:
        r = ix.result_from_arrays(alns, cig)
        try:
            with pytest.raises(_lib.TelrError, match="telr_depth_medians: record's CIGAR leaves its target") as ei:
                ix.depth_medians(r, t, s, e)
            assert ei.value.code == TELR_E_ARG
        finally:
            ix.free_raw(r)
        a2, c2, _, t2, s2, e2 = dc.arrays(dc.GOOD)
        r = ix.result_from_arrays(a2, c2)
        try:
            same(ix.depth_medians(r, t2, s2, e2), dc.want_array(dc.GOOD))
        finally:
            ix.free_raw(r)
    finally:
        ix.free()
