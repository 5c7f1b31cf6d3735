"""Sorted anchor lists aimed at the edges of the default chaining stage -- chain_dispatch (telr_engine.hip) and section 4 of
kernels.hip.h: the push loop d_chain_run<R>, the lazy far look-back d_chain_run_lazy<R>, the R-wave ring d_chain_run_mw<R> and the
island launch (k_isl_heads, k_isl_fill, k_chain_isl), which must all yield the f / p of the oracle's chain_dp -- and a restatement in
Python of that loop.  tests/test_chain_edges_ref.py holds the oracle's tap (tor_debug_chain) to the restatement and checks that every
case reaches the edge it is built for; tests/test_gpu_chain_edges.py holds the engine's tap (telr_debug_chain) to the oracle's, in
process and under the switches that pin one loop (tests/chain_edges_child.py).

A case is a dict: name, lists (one sorted key list per query), mo, and `reach`, a function of the reference's (F, P) -- per-query
lists of f and p -- that asserts the edge the case aims at is in the reference's answer.  Every case is built for the look-backs 64,
128 and 256 (R = 1, 2, 4 slots per lane) and for chain_skip_q8 0 and 3 (the SKIP template argument) unless it says otherwise, with
max_gap 5000, bw 500 and no long join except where a case sets them.  Anchors are the engine's 64-bit keys: strand << 63 | global
reference position << 32 | query position << 8 | span."""
import functools

import numpy as np

from telr_amd.presets import preset
from chain_scan_ref import chain_scores, key, concat_lists, INT32_MIN

SETTINGS = [(h, s) for h in (64, 128, 256) for s in (0, 3)]
RESTATE_MAX = 6000              # anchors of a case the Python restatement is run on (~100 us per anchor)
CHAIN_ISL_NQ = 4096             # kernels.hip.h: calls of at most this many queries chain island by island
ISL_GRID = 256 * 32             # chain_dispatch: workgroups of k_chain_isl's grid-stride loop
DENSE_N, DENSE_SPAN, MW_N = 2048, 48, 1 << 19       # chain_dispatch: dense_v (TELR_CHAIN_DENSE moves them)
TPAD = 16384                    # part_plan.h: global positions stay below 2^31 - TPAD, and max_gap below TPAD
G0, Q0 = 100000, 1000


def opts(lookback, skip, **kw):
    """map-ont without the long join, with this look-back and chain_skip_q8, and the fields of kw replaced"""
    _, mo = preset("map-ont")
    mo.bw_long = 0
    mo.chain_lookback, mo.chain_skip_q8 = lookback, skip
    assert (mo.max_gap, mo.bw) == (5000, 500)
    for k, v in kw.items():
        assert hasattr(mo, k), k
        setattr(mo, k, v)
    return mo


# ---------------------------------------------------------------------------------------------------------------------
# the restatement


def chain_default(a, mo):
    """the oracle's default chain_dp loop on one query's sorted anchors: for anchor i, j descends from i - 1 to max(0, i - H) and a
    link is taken on v > best, best starting at the span -- the largest index wins ties, and a link that only equals the span is not
    taken.  -> f, p (p relative to the list, -1 for none)"""
    a = np.asarray(a, np.uint64)
    n, H = len(a), int(mo.chain_lookback)
    f = np.zeros(n, np.int64)
    p = np.full(n, -1, np.int64)
    lowest = np.iinfo(np.int64).min
    for i in range(n):
        best, bp = int(a[i] & np.uint64(0xff)), -1
        st = max(0, i - H)
        if st < i:
            js = np.arange(i - 1, st - 1, -1)
            sc = chain_scores(a[i], a[js], mo)
            v = np.where(sc != INT32_MIN, f[js] + sc, lowest)
            k = int(np.argmax(v))                     # the first maximum in scan order: the largest j among equals
            if v[k] > best:
                best, bp = int(v[k]), int(js[k])
        f[i], p[i] = best, bp
    return f.astype(np.int32), p.astype(np.int32)


def chain_default_all(keys, off, mo):
    f = np.zeros(len(keys), np.int32)
    p = np.zeros(len(keys), np.int32)
    for q in range(len(off) - 1):
        s, e = int(off[q]), int(off[q + 1])
        f[s:e], p[s:e] = chain_default(keys[s:e], mo)
    return f, p


def split(f, p, off):
    """(f, p) of a concatenated call -> per-query lists (F, P)"""
    return ([f[off[q]:off[q + 1]] for q in range(len(off) - 1)], [p[off[q]:off[q + 1]] for q in range(len(off) - 1)])


def link_score(ai, aj, mo):
    return int(chain_scores(ai, np.array([aj], np.uint64), mo)[0])


def n_anchors(case):
    return sum(len(L) for L in case["lists"])


def n_islands(L, max_gap):
    """island heads of one list as k_isl_heads counts them: the first anchor and every anchor whose reference WORD (strand in bit 31)
    lies more than max_gap beyond its predecessor's"""
    if len(L) == 0:
        return 0
    w = (np.asarray(L, np.uint64) >> np.uint64(32)).astype(np.int64)
    return 1 + int(np.count_nonzero(np.diff(w) > max_gap))


def dense_samples(L, dense_span=DENSE_SPAN):
    """d_chain_dense's count: 64 samples at i = lane (n - 65) // 63, dense where 64 consecutive anchors lie within dense_span bases"""
    w = (np.asarray(L, np.uint64) >> np.uint64(32)).astype(np.int64)
    n = len(w)
    i = (np.arange(64) * (n - 65)) // 63
    return int(np.count_nonzero(w[i + 64] - w[i] <= dense_span))


def make(name, lists, mo, reach):
    for L in lists:
        a = np.asarray(L, np.uint64)
        assert np.all(a[1:] > a[:-1]), name + ": a list is not strictly ascending"
    return dict(name=name, lists=lists, mo=mo, reach=reach)


def fill(idx, g, q):
    """anchors that link to nothing in these cases: one reference position (dr == 0 among themselves), query positions far above
    the anchors under test (dq < 0 towards them, dq > max_gap from them); groups at ascending g take descending q ranges"""
    return [key(g, q + i) for i in idx]


# ---------------------------------------------------------------------------------------------------------------------
# len_*: one collinear chain of n anchors, every size at which a loop changes its path (the last chunk's `jn`, `inext < n`, the slot
# refill of d_chain_run after 64 R anchors, `if (j0 + 64 < n)` of the lazy loop's history, `nchunk` of d_chain_run_mw)


def case_len(n, H, skip, tag):
    L = [key(G0 + 10 * i, Q0 + 10 * i) for i in range(n)]

    def reach(F, P):
        assert len(P[0]) == n and P[0][0] == -1 and np.array_equal(P[0][1:], np.arange(n - 1))
    return make("len_%d%s" % (n, tag), [L], opts(H, skip), reach)


# lookback_*: the predecessor at exactly i - H is still seen (d = H) and the one at i - H - 1 is not (d = H + 1), whichever lane the
# anchor sits in.  d_chain_run: "anchors currently owned: index > j and <= j + 64R by construction" (the owner of j takes anchor
# j + 64 R before j is pushed); d_chain_run_lazy: the far set, `h == R - 1 ? lane >= jj` ("lanes >= l of chunk c-R"), reached because
# the target has no near link at all (sMs > sB >> 1) and its anchor 65 back lies within max_gap; d_chain_run_mw: "lanes >= l of chunk
# c - R: the wave's OWN previous chunk".  lead = 0 / 64: T in lane 0 (chunk R / R + 1), 63: lane 63, 200: lane 8.


def case_lookback(d, lead, H, skip, tag):
    L = (fill(range(lead), G0 - 50, 300000) + [key(G0, Q0)] + fill(range(d - 1), G0 + 5, 200000) + [key(G0 + 30, Q0 + 30)])
    ip, it = lead, lead + d

    def reach(F, P):
        assert it - ip == d and d in (H, H + 1)
        if d == H:
            assert P[0][it] == ip and F[0][it] == 30
        else:
            assert P[0][it] == -1 and F[0][it] == 15
        assert np.all(np.delete(P[0], it) == -1)
    return make("lookback_%s_lead%d%s" % ("H" if d == H else "H+1", lead, tag), [L], opts(H, skip), reach)


# tie_*: X = (g0, q0 + 20) and Y = (g0 + 20, q0) cannot link to each other and give T = (g0 + 120, q0 + 120) the same score: the
# larger index, Y, wins.  d_chain_push: `v2 >= B` with ascending j; d_chain_run_lazy: "near beats far on equality", `if (m > sB)`,
# and among far ones the largest index (`w = Bl == m ? bl : -1`, then the maximum of w; the chunks pushed oldest first with ">=").
# Placed by index: T at lane 10 of chunk R + 1.


def tie_list(t, xi, yi, X, Y, T):
    assert 0 <= xi < yi < t
    return (fill(range(xi), G0 - 50, 300000) + [X] + fill(range(xi + 1, yi), G0 + 10, 250000) + [Y]
            + fill(range(yi + 1, t), G0 + 50, 200000) + [T])


def tie_places(H):
    R = H // 64
    c, l = R + 1, 10
    t = 64 * c + l
    places = [("near_near", t - 9, t - 6)]                                                   # both within the nearest 64
    if R >= 2:                                                                                # (a look-back of 64 has no far part)
        places += [("far_near", t - 77, t - 6),                                              # X at least 65 back, Y near
                   ("far_far_chunks", 64 * (c - R) + l + 1, 64 * (c - 1) + l - 2),           # chunk c - R (lanes >= l) and chunk c - 1 (lanes < l)
                   ("far_far_newest", 64 * (c - 1) + 2, 64 * (c - 1) + 5),                   # both in chunk c - 1
                   ("far_far_oldest", 64 * (c - R) + l + 1, 64 * (c - R) + l + 5)]           # both in chunk c - R
    return t, places


def cases_tie(H, skip, tag):
    out = []
    t, places = tie_places(H)
    mo = opts(H, skip)
    X, Y, T = key(G0, Q0 + 20), key(G0 + 20, Q0), key(G0 + 120, Q0 + 120)
    for what, xi, yi in places:
        def reach(F, P, xi=xi, yi=yi):
            assert t - xi <= H and link_score(T, X, mo) == link_score(T, Y, mo)
            assert F[0][xi] == F[0][yi] == 15 and P[0][xi] == P[0][yi] == -1
            assert P[0][t] == yi and F[0][t] == 15 + link_score(T, Y, mo)
        out.append(make("tie_%s%s" % (what, tag), [tie_list(t, xi, yi, X, Y, T)], mo, reach))
    # the mirror: the far (or merely smaller-index) anchor is better by exactly 1 (its span, hence its f, is 16) and must win
    X16 = key(G0, Q0 + 20, 16)
    for what, xi, yi in places[:2]:
        def reach(F, P, xi=xi, yi=yi):
            assert F[0][xi] == F[0][yi] + 1 and link_score(T, X16, mo) == link_score(T, Y, mo)
            assert P[0][t] == xi and F[0][t] == 16 + link_score(T, X16, mo)
        out.append(make("tie_better_by_one_%s%s" % (what, tag), [tie_list(t, xi, yi, X16, Y, T)], mo, reach))
    # the far bound at equality (d_chain_run_lazy: "the far ones are out as soon as span_i + M_i <= best so far", `if (sMs > (sB >> 1))`):
    # Y, near, gives T 15 + sc; X, 70 back on T's diagonal (sc = span_T = 15, the most a link can score), has f = its span = sc, so
    # span_T + f_X equals the near best exactly and X would only tie; every other far anchor has span 1, so M = f_X.  Skipping the
    # far ones is right: Y wins.  With X one better the bound does not decide and X wins.
    if H >= 128:
        Y2, T2 = key(G0 + 100, Q0 + 20), key(G0 + 120, Q0 + 120)
        scy = link_score(T2, Y2, mo)
        for what, more in (("equal", 0), ("plus1", 1)):
            X2 = key(G0 + 90, Q0 + 90, scy + more)
            xi, yi = t - 70, t - 6
            L = ([key(G0 - 50, 300000 + i, 1) for i in range(xi)] + [X2] + [key(G0 + 95, 250000 + i, 1) for i in range(xi + 1, yi)] + [Y2]
                 + fill(range(yi + 1, t), G0 + 110, 200000) + [T2])

            def reach(F, P, more=more, xi=xi, yi=yi, X2=X2):
                assert 1 <= scy < 15 and link_score(T2, X2, mo) == 15 and F[0][xi] == scy + more and P[0][xi] == -1 and F[0][yi] == 15
                assert 15 + int(F[0][t - H:t - 64].max()) == (15 + scy) + more          # span_T + M against the near best
                assert (P[0][t], F[0][t]) == ((yi, 15 + scy) if more == 0 else (xi, 16 + scy))
            out.append(make("tie_far_bound_%s%s" % (what, tag), [L], mo, reach))
    # a best link that only EQUALS the span is not taken (B starts at 2 span + 1: `v2 >= B` fails at 2 v == 2 span; in the lazy loop
    # `m > sB` with sB odd), one better is: J = (g0, q0) with span 5 / 6, T 10 bases on (sc = 10, f_J + sc = 15 / 16 against span 15)
    for what, back in (("near", 1), ("far", 70)):
        if back > H:
            continue
        for sj in (5, 6):
            L = fill(range(20), G0 - 50, 300000) + [key(G0, Q0, sj)] + fill(range(back - 1), G0 + 5, 200000) + [key(G0 + 10, Q0 + 10)]
            it = 20 + back

            def reach(F, P, sj=sj, it=it, back=back):
                assert F[0][it - back] == sj
                assert (P[0][it], F[0][it]) == ((-1, 15) if sj == 5 else (it - back, 16))
            out.append(make("tie_span_%s_%s%s" % ("equal" if sj == 5 else "plus1", what, tag), [L], mo, reach))
    return out


# limit_*: pairs on each side of each limit of d_chain_link's folded range test `ok = max3(dr-1, dq-1, dd + ddc) < max_gap` with
# ddc = bw < max_gap ? max_gap - 1 - bw : 0, and the strand in bit 31 of the reference word.  Query 0: the link is taken, query 1:
# it is not.  `mid`: an unrelated anchor between the two keeps consecutive anchors within max_gap, so that the link test itself is
# asked (without it the scalar shortcut `gnext - gj > max_gap` and the island heads answer first).


def pair_case(name, mo, pre, B_in, B_out, mid=None, rev=0):
    """pre: the anchors before the pair's second one, the last of them its first one (a chain, so that a link with a large penalty
    still wins on f_j)"""
    def mk(B):
        L = list(pre) + ([mid] if mid is not None else []) + [B]
        return [k | (rev << 63) for k in L]
    lists = [mk(B_in), mk(B_out)] if B_in is not None else [mk(B_out)]
    ia = len(pre) - 1
    last = ia + (2 if mid is not None else 1)

    def reach(F, P):
        if B_in is not None:
            assert P[0][last] == ia and F[0][last] == F[0][ia] + link_score(lists[0][last], lists[0][ia], mo)
        assert P[-1][last] == -1 and F[-1][last] == 15
        assert all(np.array_equal(p[:ia + 1], np.arange(-1, ia)) for p in P)
    return make(name, lists, mo, reach)


def cases_limit(H, skip, tag):
    out = []
    A = [key(G0, Q0)]
    pre = [key(G0 + 255 * i, Q0 + 255 * i, 255) for i in range(9)]         # f = 2295 at its end (gp, qp)
    gp, qp = G0 + 255 * 8, Q0 + 255 * 8
    for rev in (0, 1):                       # "the same coordinates on the other strand"
        r = "_rev" if rev else ""
        mo = opts(H, skip)
        mg, bw = mo.max_gap, mo.bw
        mid = key(gp + 2500, 300000)
        for m, mt in ((None, ""), (mid, "_mid")):
            out.append(pair_case("limit_dr_max_gap%s%s%s" % (mt, r, tag), mo, pre, key(gp + mg, qp + mg - 400), key(gp + mg + 1, qp + mg - 399), m, rev))
            out.append(pair_case("limit_dq_max_gap%s%s%s" % (mt, r, tag), mo, pre, key(gp + mg - 400, qp + mg), key(gp + mg - 399, qp + mg + 1), m, rev))
        # dd = bw and bw + 1 on both sides of the diagonal, bw < max_gap (ddc = max_gap - 1 - bw)
        out.append(pair_case("limit_dd_bw_dr%s%s" % (r, tag), mo, pre, key(gp + 2 * bw, qp + bw), key(gp + 2 * bw + 1, qp + bw), None, rev))
        out.append(pair_case("limit_dd_bw_dq%s%s" % (r, tag), mo, pre, key(gp + bw, qp + 2 * bw), key(gp + bw, qp + 2 * bw + 1), None, rev))
        # bw >= max_gap: the `ddc == 0` branch -- dd is bounded by max_gap - 1 alone
        mo2 = opts(H, skip, max_gap=2000, bw=6000)
        out.append(pair_case("limit_bw_above_max_gap_dr%s%s" % (r, tag), mo2, pre, key(gp + 2000, qp + 1), key(gp + 2001, qp + 1), None, rev))
        out.append(pair_case("limit_bw_above_max_gap_dq%s%s" % (r, tag), mo2, pre, key(gp + 1, qp + 2000), key(gp + 1, qp + 2001), None, rev))
        # bw = max_gap - 2: ddc = 1, the smallest one that still bites (dd = max_gap - 2 passes, max_gap - 1 does not)
        mo3 = opts(H, skip, bw=mg - 2)
        out.append(pair_case("limit_bw_just_below_max_gap%s%s" % (r, tag), mo3, pre, key(gp + mg, qp + 2), key(gp + mg, qp + 1), None, rev))
        # the long join: chain_dispatch takes max(bw, bw_long); 20000 > max_gap (ddc == 0), 2000 < max_gap (dd = 2000 / 2001)
        mo4 = opts(H, skip, bw_long=20000)
        out.append(pair_case("limit_bw_long_20000%s%s" % (r, tag), mo4, pre, key(gp + mg, qp + 1), key(gp + mg + 1, qp + 1), None, rev))
        mo5 = opts(H, skip, bw_long=2000)
        out.append(pair_case("limit_bw_long_2000%s%s" % (r, tag), mo5, pre, key(gp + 4000, qp + 2000), key(gp + 4001, qp + 2000), None, rev))
        # dr == 0 (same reference position, two query positions), dq == 0, dq < 0: `dr1 = gi - gj1` and `dq1 = qi - qj1` wrap to 2^32 - 1
        out.append(pair_case("limit_dr_zero%s%s" % (r, tag), mo, A, key(G0 + 1, Q0 + 1), key(G0, Q0 + 10), None, rev))
        out.append(pair_case("limit_dq_zero%s%s" % (r, tag), mo, A, key(G0 + 1, Q0 + 1), key(G0 + 10, Q0), None, rev))
        out.append(pair_case("limit_dq_negative%s%s" % (r, tag), mo, [key(G0, Q0 + 10)], None, key(G0 + 10, Q0), None, rev))
    mo = opts(H, skip)
    # a strand change in the middle of a 64-chunk, at lane 63 and at lane 0: the reverse anchors continue the forward chain's
    # coordinates, so only bit 31 keeps them apart ("a strand mismatch fails the unsigned range test of dr")
    for s in (64 + 20, 127, 128):
        L = [key(G0 + 10 * i, Q0 + 10 * i, rev=int(i >= s)) for i in range(s + 70)]

        def reach(F, P, s=s):
            want = np.arange(-1, s + 69)
            want[s] = -1
            assert np.array_equal(P[0], want) and F[0][s] == 15
        out.append(make("limit_strand_change_at_%d%s" % (s, tag), [L], mo, reach))
    # the two strands at the extremes of the legal positions (an index keeps global positions below 2^31 - TPAD, and max_gap is below
    # TPAD): a forward anchor at the top, a reverse one at g = span - 1 whose query position would link; the words differ by less
    # than 2^32 only through bit 31
    mo6 = opts(H, skip, max_gap=TPAD - 1, bw_long=20000)
    top = (1 << 31) - TPAD - 64
    L = [key(top - 100, Q0), key(top, Q0 + 100), key(14, Q0 + 200, rev=1), key(114, Q0 + 300, rev=1)]

    def reach(F, P):
        assert list(P[0]) == [-1, 0, -1, 2]
    out.append(make("limit_strand_extremes" + tag, [L], mo6, reach))
    # the smallest legal global position (g = span - 1) at the head of a list longer than 64 R: a chain fills chunk 0, the anchors of
    # the next chunks have no near link and a far bound that does not decide (Ms = the chain's f), so d_chain_run_lazy evaluates
    # their far links against the history's empty chunks (hg == 0, hq == 0x7fffffff: "no such anchor -- fails every range test")
    # with `gj - gfar <= max_gap` true for the small g
    for rev in (0, 1):
        R = H // 64
        L = [key(14 + 10 * i, 14 + 10 * i, rev=rev) for i in range(64)] + [k | (rev << 63) for k in fill(range(64 * R + 10 - 64), 14 + 635, 300000)]

        def reach(F, P, L=L):
            assert len(P[0]) > H and (int(L[0]) >> 32) & 0x7fffffff == 14 and F[0][0] == 15 and F[0][63] == 15 + 630
            assert np.array_equal(P[0][:64], np.arange(-1, 63)) and np.all(P[0][64:] == -1)
        out.append(make("limit_smallest_g%s%s" % ("_rev" if rev else "", tag), [L], mo, reach))
    return out


# score_*: d_chain_link's arithmetic against chain_sc: min(span, dg) by v_min3 on the values less one, the penalty
# `__umul24(gap_q8, dd) + l2h - 16256` with ilog2_q8(dd + 1) >> 1 read off the float exponent, `__umul24(skip_q8, dgm + 1)`, and the
# SKIP branch `if (dd == 0u && dgm <= sp1) pen = 0`.  Every row is a query: a chain of nine anchors of span 255 (f = 2295, so that
# a link whose own score is negative still wins), then the successor one base on (dg = 1).  max_gap = TPAD - 1 and bw_long = 20000 allow dd up to
# 2^14 - 2; the rows beyond are refused by the range test.


def cases_score(H, skip, tag):
    mo = opts(H, skip, max_gap=TPAD - 1, bw_long=20000)
    pre = [key(G0 + 255 * i, Q0 + 255 * i, 255) for i in range(9)]
    gp, qp = G0 + 255 * 8, Q0 + 255 * 8
    lists, rows = [], []
    for k in range(1, 15):
        for dd in ((1 << k) - 2, (1 << k) - 1, 1 << k):
            lists.append(pre + [key(gp + dd + 1, qp + 1)]); rows.append(("dr", dd))
            if dd > 0:              # (dd == 0 is one list, not two)
                lists.append(pre + [key(gp + 1, qp + dd + 1)]); rows.append(("dq", dd))

    def reach(F, P):
        assert all(F[q][8] == 2295 for q in range(len(lists)))
        for q, (side, dd) in enumerate(rows):
            if dd + 1 <= mo.max_gap:
                sc = link_score(lists[q][9], lists[q][8], mo)
                assert P[q][9] == 8 and F[q][9] == 2295 + sc, (side, dd)
                if dd >= 512:
                    assert sc < 0
            else:
                assert P[q][9] == -1 and F[q][9] == 15, (side, dd)
        # worked by hand (gap_q8 = 31, dg = 1 so min(span, dg) = 1): dd = 1: pen = 31 + 128 (+ 3) >> 8 = 0; dd = 2: 62 + 192 = 254 >> 8 = 0,
        # with chain_skip_q8 = 3: 257 >> 8 = 1; dd = 16382: 507842 + (13 * 256 + 255 >> 1 = 1791) (+ 3) >> 8 = 1990
        by = {r: q for q, r in enumerate(rows)}
        assert F[by[("dr", 1)]][9] == 2296 and F[by[("dq", 2)]][9] == (2295 if skip else 2296) and F[by[("dr", 16382)]][9] == 2296 - 1990
    out = [make("score_dd_powers" + tag, lists, mo, reach)]

    # spans 1, 15 and 255 with dg < span (overlapping minimizers), dg == span, dg == span + 1, at dd == 0 and dd == 1; and a link whose
    # negative score does NOT win (f_j = 15 against a penalty of 31 at dd = 200)
    lists2, rows2 = [], []
    for sp in (1, 15, 255):
        for dg in (sp - 1, sp, sp + 1):
            for dd in (0, 1):
                if dg >= 1:
                    lists2.append([key(G0, Q0, sp), key(G0 + dg + dd, Q0 + dg, sp)]); rows2.append((sp, dg, dd))
    lists2.append([key(G0, Q0), key(G0 + 300, Q0 + 100)]); rows2.append("loses")
    mo2 = opts(H, skip)

    def reach2(F, P):
        for q, r in enumerate(rows2):
            a = lists2[q]
            sc = link_score(a[1], a[0], mo2)
            if r == "loses":
                assert sc < 0 and sc != INT32_MIN and P[q][1] == -1 and F[q][1] == 15
            elif sc > 0:
                assert P[q][1] == 0 and F[q][1] == r[0] + sc, r
            else:
                assert P[q][1] == -1 and F[q][1] == r[0], r
        by = {r: q for q, r in enumerate(rows2)}
        # worked by hand: span 255, dd == 0: dg = 254 -> 254, dg = 255 -> 255 (with chain_skip_q8 = 3 the `pen = 0` branch: 3 * 255 >> 8
        # would take 2), dg = 256 -> 255 - (768 >> 8) = 252 with the skip cost, 255 without
        assert F[by[(255, 254, 0)]][1] == 509 and F[by[(255, 255, 0)]][1] == 510 and F[by[(255, 256, 0)]][1] == (507 if skip else 510)
        assert F[by[(1, 1, 0)]][1] == 2 and F[by[(15, 14, 0)]][1] == 29
    out.append(make("score_spans" + tag, lists2, mo2, reach2))
    return out


# isolated_*: consecutive anchors exactly max_gap apart (linked) and max_gap + 1 apart (not linked): d_chain_run's and
# d_chain_run_lazy's scalar shortcut `gnext - gj > max_gap` and k_isl_heads' `> max_gap`, on one strand and across the strand change.
# The heads fall at indices 71, 77 and 148 (no multiples of 64), so k_isl_fill's isl_pd (`myp + pdelta`) matters.


def case_isolated(H, skip, tag):
    mo = opts(H, skip)
    mg = mo.max_gap
    pts = [(G0 + 10 * i, Q0 + 10 * i, 0) for i in range(70)]

    def add(dg, dq, rev=0, n=1):
        for _ in range(n):
            g, q, _r = pts[-1]
            pts.append((g + dg, q + dq, rev))
    add(mg, mg - 400)               # 70: linked to 69
    add(mg + 1, mg - 400)           # 71: an island head
    add(10, 10, n=5)                # 72..76
    add(mg, 100, rev=1)             # 77: max_gap on, but the other strand: a head
    add(10, 10, rev=1, n=69)        # 78..146
    add(mg, mg - 400, rev=1)        # 147: linked to 146
    add(mg + 1, mg - 400, rev=1)    # 148: a head
    add(10, 10, rev=1, n=70)        # 149..218
    L = [key(g, q, rev=r) for g, q, r in pts]

    def reach(F, P):
        p = P[0]
        assert p[70] == 69 and p[71] == -1 and p[72] == 71 and p[77] == -1 and p[78] == 77 and p[147] == 146 and p[148] == -1 and p[149] == 148
        assert n_islands(L, mg) == 4
    return make("isolated" + tag, [L], mo, reach)


# islands_many: more islands than the ISL_GRID = 8,192 workgroups of k_chain_isl's grid-stride loop (`s += gridDim.x`), on both
# strands, with three short chains among them; one wave walks the whole list where the call has more than CHAIN_ISL_NQ queries


def case_islands_many(H, skip, tag):
    mo = opts(H, skip)
    mg = mo.max_gap
    L, chains, g = [], [], 50
    for i in range(8200):
        rev = int(i >= 4100)
        if i == 4100:
            g = 50
        g += mg + 1
        L.append(key(g, Q0 + (i % 97), rev=rev))
        if i in (0, 4099, 8199):
            for k in range(1, 5):
                g += 10
                L.append(key(g, Q0 + (i % 97) + 10 * k, rev=rev))
                chains.append(len(L) - 1)

    def reach(F, P):
        assert n_islands(L, mg) > ISL_GRID
        assert all(P[0][i] == i - 1 for i in chains) and np.count_nonzero(P[0] >= 0) == len(chains)
    return make("islands_many" + tag, [L], mo, reach)


# lattice_*: a tandem array (WHICH LOOP: "an anchor's collinear predecessor lies (copies in the read) x (a few bases) anchors back,
# past the 64 nearest, the bound never decides and EVERY anchor pays the far evaluation"): 80 reference positions 4 apart, 70 query
# positions each.  With H >= 128 every link lies more than 64 back; with H = 64 there is none.


def lattice(n):
    """the first n anchors of the array, in sorted order"""
    ng = -(-n // 70)
    return [key(g, 2000 + (g - 1000) % 40 + 40 * c) for g in range(1000, 1000 + 4 * ng, 4) for c in range(70)][:n]


def case_lattice(H, skip, tag):
    L = lattice(5600)

    def reach(F, P):
        back = (np.arange(5600) - P[0])[P[0] >= 0]
        if H >= 128:
            assert len(back) == 5523 and back.min() > 64 and back.max() == 71
        else:
            assert len(back) == 0
    return make("lattice" + tag, [L], opts(H, skip), reach)


# dense_choice_*: d_chain_dense at its two thresholds: `n < o.dense_n` (runs of 2,047 and 2,048 anchors) and `>= 21` of the 64
# samples (a lattice prefix sized for 20 and for 21 dense windows).  A chain whose links lie 67 back follows the prefix, in the same
# island (the run must stay one run on the island path).


def dense_choice_list(n, want):
    pre, tail, k = lattice(n), [], 0
    while len(tail) < n:
        tail.append(key(1400 + 100 * k, 10000 + 100 * k))
        tail += [key(1400 + 100 * k + 1 + t, 600000 - 100 * k - t) for t in range(66)]
        k += 1
    pre, tail = np.array(pre, np.uint64), np.array(tail, np.uint64)
    for npre in range(64, n - 64):
        L = np.concatenate((pre[:npre], tail[:n - npre]))
        if dense_samples(L) == want:
            return [int(x) for x in L]
    raise AssertionError("no prefix gives %d dense samples" % want)


def cases_dense_choice(H, skip, tag):
    out = []
    for n in (DENSE_N - 1, DENSE_N):
        for want in (20, 21):
            L = _dense_list(n, want)

            def reach(F, P, L=L, n=n, want=want):
                assert len(L) == n and dense_samples(L) == want and n_islands(L, 5000) == 1
                back = (np.arange(n) - P[0])[P[0] >= 0]
                assert back.max() > 64 if H >= 128 else len(back) == 0
            out.append(make("dense_choice_%d_%d%s" % (n, want, tag), [L], opts(H, skip), reach))
    return out


@functools.lru_cache(maxsize=None)
def _dense_list(n, want):
    return dense_choice_list(n, want)


# mw_*: dense runs for the R-wave ring (under the child's TELR_CHAIN_DENSE=128,300,128 every dense run of 128 anchors and more goes
# to k_chain_mw where the call has more than CHAIN_ISL_NQ queries): fewer chunks than waves (128, 129 with R = 4), runs just under
# the threshold, a tail chunk that is no multiple of the eight-anchor publish group (`(jj & 7) == 7 || jj == jn - 1`), and the ring's
# wrap-around (`& (RING - 1)`, eight times round)


def cases_mw(H, skip, tag):
    R = H // 64
    out = []
    for n in sorted(set((128, 129, 64 * R - 1, 64 * R + 1, 64 * (R + 1) + 5, 8 * 64 * R + 3))):
        L = lattice(n)

        def reach(F, P, L=L, n=n):
            assert len(P[0]) == n and (n < 128 or dense_samples(L, 300) == 64)
            back = (np.arange(n) - P[0])[P[0] >= 0]
            if H >= 128 and n > 128:
                assert back.min() > 64
            if H == 64:
                assert len(back) == 0
        out.append(make("mw_%d%s" % (n, tag), [L], opts(H, skip), reach))
    return out


# mw_default (look-back 128 only): dense runs of 2^19 and 2^19 - 1 anchors, the only input that reaches k_chain_mw through the
# over-size `list` at the production threshold (`n >= o.mw_n`; one short of it: the one-wave push loop); reference by the oracle's
# tap only


def lattice_np(n):
    ng = -(-n // 70)
    g = np.repeat(1000 + 4 * np.arange(ng, dtype=np.uint64), 70)
    c = np.tile(np.arange(70, dtype=np.uint64), ng)
    q = np.uint64(2000) + (g - np.uint64(1000)) % np.uint64(40) + np.uint64(40) * c
    return ((g << np.uint64(32)) | (q << np.uint64(8)) | np.uint64(15))[:n]


def case_mw_default(skip):
    lists = [lattice_np(MW_N), lattice_np(MW_N - 1)]

    def reach(F, P):
        assert [len(p) for p in P] == [MW_N, MW_N - 1] and MW_N > 20480
        for L, p in zip(lists, P):
            assert dense_samples(L) == 64
            back = (np.arange(len(p)) - p)[p >= 0]
            assert len(back) > len(p) * 99 // 100 and back.min() > 64 and back.max() == 71         # (one anchor in 700 starts a chain)
    return make("mw_default_s%d" % skip, lists, opts(128, skip), reach)


# mixed_queries: all the small cases of a setting that share its options as the queries of one call, an empty query between every
# two and three in front: list bases are unaligned, and every kernel finds a query only through the offsets (q_aoff[q], isl_off,
# isl_pd).  Each query still has to reach its own case's edge.


def case_mixed(parts, H, skip, tag):
    lists, spans = [[], [], []], []
    for c in parts:
        spans.append((c, len(lists), len(c["lists"])))
        for L in c["lists"]:
            lists += [L, []]

    def reach(F, P):
        assert len(lists) <= CHAIN_ISL_NQ and len(parts) > 20 and sum(len(L) == 0 for L in lists) > len(parts)
        for c, at, n in spans:
            c["reach"]([F[at + 2 * k] for k in range(n)], [P[at + 2 * k] for k in range(n)])
    return make("mixed_queries" + tag, lists, opts(H, skip), reach)


def same_opts(a, b):
    return bytes(a) == bytes(b)


# ---------------------------------------------------------------------------------------------------------------------


def cases_of(H, skip):
    tag = "_h%d_s%d" % (H, skip)
    R = H // 64
    out = []
    for n in sorted(set((1, 2, 63, 64, 65, 64 * R - 1, 64 * R, 64 * R + 1, 2 * 64 * R + 1))):
        out.append(case_len(n, H, skip, tag))
    for d in (H, H + 1):
        for lead in (0, 63, 64, 200):
            out.append(case_lookback(d, lead, H, skip, tag))
    out += cases_tie(H, skip, tag)
    out += cases_limit(H, skip, tag)
    out += cases_score(H, skip, tag)
    out.append(case_isolated(H, skip, tag))
    out.append(case_lattice(H, skip, tag))
    out += cases_dense_choice(H, skip, tag)
    out += cases_mw(H, skip, tag)
    base = opts(H, skip)
    small = [c for c in out if n_anchors(c) <= RESTATE_MAX and same_opts(c["mo"], base)]
    out.append(case_islands_many(H, skip, tag))
    out.append(case_mixed(small, H, skip, tag))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for H, skip in SETTINGS:
        out += cases_of(H, skip)
    out += [case_mw_default(0), case_mw_default(3)]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case_named(name):
    return _by_name()[name]


@functools.lru_cache(maxsize=None)
def _by_name():
    return {c["name"]: c for c in cases()}


def call_input(case, nq=None):
    """the tap's input: the concatenated keys and nq + 1 offsets; nq: padded with empty queries to that many"""
    if any(isinstance(L, np.ndarray) for L in case["lists"]):
        keys = np.concatenate([np.asarray(L, np.uint64) for L in case["lists"]])
        off = np.concatenate(([0], np.cumsum([len(L) for L in case["lists"]]))).astype(np.int32)
    else:
        keys, off = concat_lists(case["lists"])
    if nq is not None:
        assert nq >= len(off) - 1
        off = np.concatenate((off, np.full(nq - (len(off) - 1), off[-1], np.int32))).astype(np.int32)
    return keys, off


_ORACLE = {}


def oracle_out(case):
    """the oracle tap's (f, p) of a case as built (computed once per process, never changed)"""
    if case["name"] not in _ORACLE:
        from oracle import binding as ob
        keys, off = call_input(case)
        f, p = ob.debug_chain(keys, off, case["mo"])
        f.setflags(write=False); p.setflags(write=False)
        _ORACLE[case["name"]] = (f, p)
    return _ORACLE[case["name"]]


def poison_input(case, off):
    """a call of the same shape whose answer differs from the case's at EVERY anchor: the taps keep their device buffers from call to
    call, so an anchor that a launch under test fails to write would otherwise come back holding an earlier call's (right) answer.
    Every list at one reference position (no links: p = -1) with a span s that is no f of the case: f = s everywhere.
    -> (keys, s)"""
    ef, _ = oracle_out(case)
    s = case.get("_poison") or next(v for v in range(1, 256) if v not in set(np.unique(ef).tolist()))
    case["_poison"] = s
    o = np.asarray(off, np.int64)
    i = np.arange(o[-1]) - np.repeat(o[:-1], np.diff(o))              # an anchor's place in its list: its query position
    return (np.uint64(5) << np.uint64(32)) | (i.astype(np.uint64) << np.uint64(8)) | np.uint64(s), s
