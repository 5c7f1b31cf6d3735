"""Anchor lists with hand-made chaining scores aimed at the edges of the three device stages between chaining and the banded DP --
peaks and back-tracking without a walker (k_nonpeak .. k_bt_scatter: 64-anchor blocks, six rounds of pointer jumping, the LDS ring of
the last look-back anchors), pass-1 chain selection (k_select1: 64 chains at a time, SEL_PCAP = 1024 primaries in LDS and the rest in
global scratch, per-target tallies searched 64 at a time) and DP segmenting (k_segments_w: windows of 64 anchors, cuts found with
ballots) -- and a short restatement in Python of what the oracle does there (the visited-array walker, select_chains, the breakpoint
loop and problem geometry of align_chain).  tests/test_backtrack_reference.py holds the oracle's tap (tor_debug_backtrack) to the
restatement and checks that every case reaches its edge; tests/test_gpu_backtrack_edges.py holds the engine's tap
(telr_debug_backtrack) to the oracle's.

A case is a dict: name, keys, q_aoff, f, p, qlen, goff, tlen, mo (the tap's input) and `reach`, a function of the reference's output
(and the case) that asserts the edge is there.  Anchors are the engine's 64-bit keys: strand << 63 | global reference position << 32
| query position << 8 | span; positions are the LAST base of the minimizer."""
import math

import numpy as np

from telr_amd.presets import preset
from telr_amd._abi import MF_CIGAR, MF_CHAIN_SKIP, MF_PER_TARGET

BLOCK = 64                  # anchors per block of the owner / depth sweeps, chains per round of k_bt_emit / k_select1, anchors per window of k_segments_w
BT_RING = 512
CHAIN_SCAN_H = 5000
SEL_PCAP = 1024
SEGSORT_CAP = 20480
DP_DMAX = 4096
ADAPT_MAX_STEPS = 1000
TPAD = 16384

CHAIN_F = ("qid", "score", "cnt", "rev", "tid", "rs", "re", "qs", "qe")
ARRAYS = ("chains", "ch_off", "ch_aoff", "canch", "kept", "prob_off", "probs")


def key(g, q, span=15, rev=0):
    return (int(rev) << 63) | (int(g) << 32) | (int(q) << 8) | int(span)


def opts(flags=0, **kw):
    """map-ont with the fields of kw replaced; flags: TELR_MF_* bits in place of the preset's (no CIGAR unless asked for)"""
    _, mo = preset("map-ont")
    mo.flags = flags
    for k, v in kw.items():
        assert hasattr(mo, k), k
        setattr(mo, k, v)
    return mo


def targets(tlens):
    """goff / tlen of targets laid out as the engine's index does (padding between them, offsets multiples of 64)"""
    goff, g = [], 0
    for t in tlens:
        goff.append(g)
        g = (g + t + TPAD + 63) & ~63
    goff.append(g)
    assert g < (1 << 31)
    return np.array(goff, np.uint32), np.array(tlens, np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement


def ref_walker(keys, f, p, mo):
    """chain_backtrack of the oracle on one query: peaks (no successor of larger f, f >= min_chain_score) in (f descending, index
    ascending) order, each walked up to the first visited anchor.  -> list of (score, cnt, [anchor indices ascending])"""
    n = len(keys)
    nonpeak = [False] * n
    for i in range(n):
        if p[i] >= 0 and f[i] > f[p[i]]:
            nonpeak[p[i]] = True
    peaks = sorted((i for i in range(n) if not nonpeak[i] and f[i] >= mo.min_chain_score), key=lambda i: (-int(f[i]), i))
    vis = [False] * n
    out = []
    for i in peaks:
        if vis[i]:
            continue
        idx, j = [], i
        while j >= 0 and not vis[j]:
            vis[j] = True
            idx.append(j)
            j = int(p[j])
        sc = int(f[i]) - (int(f[j]) if j >= 0 else 0)
        if sc < mo.min_chain_score or len(idx) < mo.min_cnt:
            continue                                    # dropped; its anchors stay visited
        out.append((sc, len(idx), idx[::-1]))
    return out


def ref_box(a0, a1, goff):
    a0, a1 = int(a0), int(a1)
    g0, span = (a0 >> 32) & 0x7fffffff, a0 & 0xff
    tid = int(np.searchsorted(goff[:-1], g0, side="right")) - 1
    go = int(goff[tid])
    rs = max(0, g0 - go - span + 1)
    return a0 >> 63, tid, rs, ((a1 >> 32) & 0x7fffffff) - go + 1, ((a0 >> 8) & 0xffffff) - span + 1, ((a1 >> 8) & 0xffffff) + 1


def ref_select(rows, qlen, mo):
    """select_chains of the oracle in pass 1 on one query's chain rows (CHAIN_F): (score descending, discovery ascending) order, a
    chain overlapping an earlier PRIMARY by more than mask_level x the shorter interval is its secondary (the first such primary);
    secondaries stay with score >= pri_ratio x parent while fewer than best_n are kept (per target under TELR_MF_PER_TARGET).  The
    products and comparisons are float32, as in C.  -> (kept discovery indices in rank order, parent rank among primaries or -1)"""
    per_t = bool(mo.flags & MF_PER_TARGET)
    n = len(rows)
    order = sorted(range(n), key=lambda c: (-int(rows[c][1]), c))
    pfs = np.zeros(n, np.int64); pfe = np.zeros(n, np.int64); ptid = np.zeros(n, np.int64); pkey = np.zeros(n, np.int64)
    n_prim = 0
    ml, pr = np.float32(mo.mask_level), np.float32(mo.pri_ratio)
    kept, parents, n2 = [], [], {}
    for c in order:
        _, sc, _, rev, tid, _, _, qs, qe = (int(v) for v in rows[c])
        fs, fe = (qlen - qe, qlen - qs) if rev else (qs, qe)
        ol = np.maximum(np.minimum(pfe[:n_prim], fe) - np.maximum(pfs[:n_prim], fs), 0)
        mn = np.minimum(pfe[:n_prim] - pfs[:n_prim], fe - fs)
        hit = ol.astype(np.float32) > ml * mn.astype(np.float32)
        if per_t:
            hit &= ptid[:n_prim] == tid
        w = np.flatnonzero(hit)
        if len(w) == 0:
            pfs[n_prim], pfe[n_prim], ptid[n_prim], pkey[n_prim] = fs, fe, tid, sc
            n_prim += 1
            kept.append(c); parents.append(-1)
            continue
        par = int(w[0])
        if not mo.secondary or np.float32(sc) < np.float32(pkey[par]) * pr:
            continue
        t = tid if per_t else -1
        if n2.get(t, 0) < mo.best_n:
            n2[t] = n2.get(t, 0) + 1
            kept.append(c); parents.append(par)
    return kept, parents


def _even_lo(lo):
    return lo - (lo & 1)


def _fill_band(m, n, mo):
    q4 = mo.fill_band_q4 if mo.fill_band_q4 > 0 else 8
    return min(2 + ((q4 * math.isqrt(min(m, n))) >> 4), mo.bw)


def _fill_band_wide(m, n, mo):
    mn, adl = min(m, n), abs(n - m)
    w = min(24 + (mn >> 3) if mn <= 512 else 88 + ((mn - 512) >> 4), mo.bw)
    cap = max(int((1022 - adl) / 2), _fill_band(m, n, mo))          # (C division: towards zero)
    return min(w, cap)


def ref_problems(row, anchors, go, qlen, tlen, mo):
    """the DP problems of one kept chain (the breakpoint loop and geometry of the oracle's align_chain) as telr_debug_dp rows"""
    qid, _, cnt, rev, tid, rs, re, qs, qe = (int(v) for v in row[:9])
    out = []

    def put(q_off, t_off, m, n, dlo, dhi, kind, qstep, tstep):
        out.append((qid, q_off, tid, t_off, m, n, dlo, dhi, kind, qstep, tstep, rev))
    eb = mo.ext_band
    if qs > 0 and rs > 0:
        mq = min(qs, mo.ext_max); mt = min(rs, mq + eb)
        put(qlen - qs if rev else qs - 1, rs - 1, mq, mt, _even_lo(-eb), eb, 1, 1 if rev else -1, -1)
    lr, lq = rs, qs
    for i in range(cnt):
        a = int(anchors[i])
        cr, cq = ((a >> 32) & 0x7fffffff) - go + 1, ((a >> 8) & 0xffffff) + 1
        if not (i == cnt - 1 or (cq - lq >= mo.min_ksw_len and cr - lr >= mo.min_ksw_len)):
            continue
        m, n = cq - lq, cr - lr
        w = _fill_band_wide(m, n, mo) if m + n > ADAPT_MAX_STEPS else _fill_band(m, n, mo)
        dl = n - m
        dlo, dhi, kind = _even_lo(min(dl, 0) - w), max(dl, 0) + w, 0
        if mo.bw_long > mo.bw and abs(dl) > mo.bw:
            dlo, dhi, kind = _even_lo(-eb), eb, 5
        elif dhi - dlo + 1 > DP_DMAX:
            kind = 3
        put(qlen - 1 - lq if rev else lq, lr, m, n, dlo, dhi, kind, -1 if rev else 1, 1)
        lr, lq = cr, cq
    if qe < qlen and re < tlen:
        mq = min(qlen - qe, mo.ext_max); mt = min(tlen - re, mq + eb)
        put(qlen - 1 - qe if rev else qe, re, mq, mt, _even_lo(-eb), eb, 2, -1 if rev else 1, 1)
    return out


def ref_backtrack(case):
    """the whole tap restated: -> the dict of ARRAYS that ob.debug_backtrack and Engine.debug_backtrack return, plus `parents`
    (per kept chain: the rank among its query's primaries of the primary that masks it, -1 for a primary)"""
    keys, off, f, p, mo, goff = case["keys"], case["q_aoff"], case["f"], case["p"], case["mo"], case["goff"]
    chains, ch_off, ch_aoff, canch, kept, prob_off, probs, parents = [], [0], [0], [], [], [0], [], []
    for q in range(len(off) - 1):
        a0, a1 = int(off[q]), int(off[q + 1])
        k = keys[a0:a1]
        rows = []
        for sc, cnt, idx in ref_walker(k, f[a0:a1], p[a0:a1], mo):
            rev, tid, rs, re, qs, qe = ref_box(k[idx[0]], k[idx[-1]], goff)
            rows.append((q, sc, cnt, rev, tid, rs, re, qs, qe))
            canch.extend(int(k[i]) for i in idx)
            ch_aoff.append(len(canch))
        base = len(chains)
        chains.extend(rows)
        ch_off.append(len(chains))
        kq, pq = ref_select(rows, int(case["qlen"][q]), mo)
        for c, par in zip(kq, pq):
            kept.append(rows[c] + (base + c,))
            parents.append(par)
            if mo.flags & MF_CIGAR:
                tid = rows[c][4]
                probs.extend(ref_problems(rows[c], canch[ch_aoff[base + c]:ch_aoff[base + c + 1]], int(goff[tid]), int(case["qlen"][q]),
                                          int(case["tlen"][tid]), mo))
            prob_off.append(len(probs))
    return dict(chains=np.array(chains, np.int32).reshape(-1, 9), ch_off=np.array(ch_off, np.int32), ch_aoff=np.array(ch_aoff, np.int32),
                canch=np.array(canch, np.uint64), kept=np.array(kept, np.int32).reshape(-1, 10), prob_off=np.array(prob_off, np.int32),
                probs=np.array(probs, np.int32).reshape(-1, 12), parents=np.array(parents, np.int64))


def assert_same(got, want, name):
    for a in ARRAYS:
        assert got[a].shape == want[a].shape, "%s: %s has shape %s, the reference %s" % (name, a, got[a].shape, want[a].shape)
        bad = np.argwhere(got[a] != want[a])
        assert len(bad) == 0, "%s: %s differs at %s: %s, the reference %s (%d differences)" % (
            name, a, tuple(bad[0]), got[a][tuple(bad[0])], want[a][tuple(bad[0])], len(bad))


# ---------------------------------------------------------------------------------------------------------------------
# building cases


class Build:
    """queries added one by one; a query's anchors are sorted by key (p follows) as the engine's are"""

    def __init__(self, name, mo, tlens=(1 << 20,)):
        self.name, self.mo = name, mo
        self.goff, self.tlen = targets(tlens)
        self.keys, self.f, self.p, self.off, self.qlen = [], [], [], [0], []

    def query(self, qlen, anchors=(), f=(), p=()):
        """anchors: (tid, r, q, span, rev) with r, q the target-local / strand-local position of the minimizer's last base"""
        k = np.array([key(int(self.goff[t]) + r, q, s, rv) for t, r, q, s, rv in anchors], np.uint64)
        f = np.asarray(f, np.int64); p = np.asarray(p, np.int64)
        assert len(k) == len(f) == len(p)
        o = np.argsort(k, kind="stable")
        inv = np.empty(len(o), np.int64); inv[o] = np.arange(len(o))
        self.keys.append(k[o]); self.f.append(f[o]); self.p.append(np.where(p[o] >= 0, inv[np.maximum(p[o], 0)], -1))
        self.off.append(self.off[-1] + len(k)); self.qlen.append(qlen)
        return self

    def done(self, reach, note):
        p = np.concatenate(self.p) if self.p else np.zeros(0, np.int64)
        case = dict(name=self.name, note=note, mo=self.mo, goff=self.goff, tlen=self.tlen, q_aoff=np.array(self.off, np.int32),
                    keys=np.concatenate(self.keys).astype(np.uint64), f=np.concatenate(self.f).astype(np.int32), p=p.astype(np.int32),
                    qlen=np.array(self.qlen, np.int32), reach=reach)
        idx = np.concatenate([np.arange(n) for n in np.diff(case["q_aoff"])]) if len(p) else p
        assert np.all((p >= -1) & (p < idx)), self.name
        return case


def line(n, r0=100, q0=100, dr=10, dq=10, tid=0, span=15, rev=0):
    return [(tid, r0 + i * dr, q0 + i * dq, span, rev) for i in range(n)]


def links(case):
    """(query, i, i - p[i]) of every link, as arrays"""
    off, p = case["q_aoff"], case["p"]
    q = np.repeat(np.arange(len(off) - 1), np.diff(off))
    i = np.arange(len(p)) - off[:-1][q]
    m = p >= 0
    return q[m], i[m], (i - p)[m]


def random_forest(rng, n, lookback, p_root=0.15):
    """f, p of a forest with links of up to `lookback` anchors, children that share parents, children below their parents and ties in f"""
    f = np.zeros(n, np.int64); p = np.full(n, -1, np.int64)
    for i in range(n):
        if i == 0 or rng.random() < p_root:
            f[i] = rng.integers(5, 70)
        else:
            p[i] = i - (rng.integers(1, min(i, lookback) + 1) if rng.random() < 0.5 else rng.integers(1, min(i, 4) + 1))
            f[i] = f[p[i]] + rng.integers(-5, 25)
    return f, p


def chains_of(out, q):
    return out["chains"][out["ch_off"][q]:out["ch_off"][q + 1]]


def kept_of(out, q):
    return out["kept"][out["kept"][:, 0] == q]


# ---- back-tracking ------------------------------------------------------------------------------------------------


def case_sizes(lookback):
    """queries of the sizes around one, two and eight blocks, empty ones between them: random forests with links up to the look-back"""
    rng = np.random.default_rng(100 + lookback)
    b = Build("bt_sizes_lb%d" % lookback, opts(chain_lookback=lookback, min_cnt=2, min_chain_score=30))
    sizes = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513)
    for n in sizes:
        f, p = random_forest(rng, n, lookback)
        b.query(n * 10 + 300, line(n), f, p)
        b.query(500)

    def reach(out, case):
        assert list(np.diff(case["q_aoff"])[::2]) == list(sizes) and np.all(np.diff(case["q_aoff"])[1::2] == 0)
        _, _, d = links(case)
        assert d.max() == lookback
        assert all(len(chains_of(out, 2 * k)) > 0 for k in range(3, len(sizes))) and all(len(chains_of(out, 2 * k + 1)) == 0 for k in range(len(sizes)))
    return b.done(reach, "query sizes at the block edges, empty queries between")


def case_path64():
    """64 consecutive links in a row: inside one block (63 hops: all that six doublings resolve), and across a block edge at every lane"""
    b = Build("bt_path64", opts(chain_lookback=64, min_cnt=2, min_chain_score=30))
    for s in range(64):
        n = 256
        f = np.full(n, 35, np.int64); p = np.full(n, -1, np.int64)          # singletons: peaks that min_cnt drops
        f[::3] = 10                                                        # and anchors that are no peaks at all
        for i in range(64 + s, 128 + s):
            p[i] = i - 1 if i > 64 + s else -1
            f[i] = 40 + 3 * (i - 64 - s)
        b.query(3000, line(n), f, p)

    def reach(out, case):
        for s in range(64):
            c = chains_of(out, s)
            assert len(c) == 1 and c[0, 2] == 64 and c[0, 1] == 40 + 3 * 63, (s, c)
    return b.done(reach, "a path of 64 anchors at every offset to the blocks")


def case_lookback(lookback):
    """links of exactly the look-back: two sparse ones that start at lane 0 and at lane 63, and a query in which EVERY link is that long"""
    L = lookback
    b = Build("bt_lookback%d" % L, opts(chain_lookback=L, min_cnt=2, min_chain_score=30))
    n = L + 293
    f = np.full(n, 20, np.int64); p = np.full(n, -1, np.int64)
    for i in (L + 64, L + 127):               # lane 0, lane 63
        p[i] = i - L; f[i - L] = 40; f[i] = 90 + i
        p[i + 1] = i; f[i + 1] = f[i] + 7      # (the chain goes on below the long link)
    b.query(n * 10 + 300, line(n), f, p)
    f = np.zeros(n, np.int64); p = np.full(n, -1, np.int64)
    for i in range(n):
        if i >= L:
            p[i] = i - L
        f[i] = (f[i - L] if i >= L else 30) + 10 + i % 7
    b.query(n * 10 + 300, line(n), f, p)

    def reach(out, case):
        q, i, d = links(case)
        assert d.max() == L and np.any((d == L) & (i % 64 == 0) & (q == 0)) and np.any((d == L) & (i % 64 == 63) & (q == 0))
        c = chains_of(out, 0)
        assert len(c) == 2 and np.all(c[:, 2] == 3)                       # both long links lie INSIDE a chain
        c = chains_of(out, 1)
        assert len(c) == L and set(c[:, 2]) == {n // L, n // L + 1}       # L interleaved paths
    return b.done(reach, "links of exactly chain_lookback from lane 0 and lane 63")


def case_scan_ring():
    """TELR_MF_CHAIN_SKIP: links of exactly CHAIN_SCAN_H = 5000 anchors, and links of BT_RING + 1 = 513, past the ring of the default mode"""
    b = Build("bt_scan_ring", opts(flags=MF_CHAIN_SKIP, min_cnt=2, min_chain_score=30))
    n = 5900
    f = np.full(n, 20, np.int64); p = np.full(n, -1, np.int64)
    for i in range(5000, 5300):
        p[i] = i - 5000; f[i] = f[i - 5000] + 30 + i % 5
    for i in range(5513, 5700):
        p[i] = i - 513; f[i] = f[i - 513] + 25
    b.query(n * 10 + 300, line(n), f, p)
    f, p = random_forest(np.random.default_rng(7), 700, 600)
    b.query(7300, line(700), f, p)

    def reach(out, case):
        q, i, d = links(case)
        assert d.max() == CHAIN_SCAN_H and np.sum(d == CHAIN_SCAN_H) == 300 and np.any(d == BT_RING + 1) and np.diff(case["q_aoff"])[0] >= 5200
        assert np.any((d == CHAIN_SCAN_H) & (i % 64 == 0)) and np.any((d == CHAIN_SCAN_H) & (i % 64 == 63))
        c = chains_of(out, 0)
        assert np.sum(c[:, 2] == 3) == 187 and np.sum(c[:, 2] == 2) == 113          # i -> i - 513 -> i - 5513: three anchors
    return b.done(reach, "the rings of the chain-skip mode")


def case_forest():
    """children that share a parent, peaks that tie in f (rank to the lower index), a chain truncated at an anchor that a better peak
    owns (score = f(peak) - f(that anchor)), a truncated chain that min_cnt drops while its anchors stay owned, peaks below min_chain_score"""
    b = Build("bt_forest", opts(chain_lookback=64, min_cnt=3, min_chain_score=10))
    #       0   1   2   3   4    5   6   7   8   9  10  11  12
    f = [10, 20, 30, 40, 100, 35, 45, 40, 42, 45, 5, 50, 50]
    p = [-1, 0, 1, 2, 3, 2, 5, 5, 7, 8, -1, 3, 3]
    b.query(1000, line(13), f, p)

    def reach(out, case):
        c = chains_of(out, 0)
        # peak 4 owns 0..4; 11 and 12 tie at 50 and are both cut off at anchor 3 (one anchor each: dropped); 6 and 9 tie at 45: {5, 6}
        # is dropped by min_cnt but keeps 5, so {7, 8, 9} scores 45 - f(5) = 10
        assert [tuple(r[1:3]) for r in c] == [(100, 5), (10, 3)], c
        assert list(out["canch"][out["ch_aoff"][1]:out["ch_aoff"][2]]) == [int(case["keys"][i]) for i in (7, 8, 9)]
    return b.done(reach, "ties, truncation and dropped chains that keep their anchors")


def case_peaks(counts, name):
    """`counts` peaks per query, every third chain dropped by min_cnt, scores in random order with ties: the rounds of k_bt_emit and
    the tiers of the peak sort"""
    rng = np.random.default_rng(len(counts) * 1000 + counts[0])
    b = Build(name, opts(chain_lookback=64, min_cnt=2, min_chain_score=30))
    for npk in counts:
        f, p = [], []
        for j in range(npk):
            if j % 3 != 2:
                p.append(-1); f.append(20)
                p.append(len(f) - 1); f.append(40 + int(rng.integers(0, max(npk // 3, 8))))
            else:
                p.append(-1); f.append(40 + int(rng.integers(0, max(npk // 3, 8))))
        b.query(len(f) * 10 + 300, line(len(f)), f, p)

    def reach(out, case):
        for q, npk in enumerate(counts):
            a0, a1 = case["q_aoff"][q:q + 2]
            f, p = case["f"][a0:a1], case["p"][a0:a1]
            is_peak = (f >= 30)
            assert int(is_peak.sum()) == npk
            c = chains_of(out, q)
            assert len(c) == npk - npk // 3 and np.all(c[:, 2] == 2)
            assert len(set(c[:, 1])) < len(c) and np.any(np.diff(c[:, 6]) < 0)          # ties, and rank order is not index order
    return b.done(reach, "peaks per query %s, every third dropped" % (counts,))


# ---- selection ---------------------------------------------------------------------------------------------------


def chain_anchors(tid, rs, qs, qe, score, n=2, rev=0, span=15, f0=None):
    """anchors, f, p of a chain with the box target start rs, query [qs, qe) (strand coordinates) and the given score"""
    assert qe - qs >= span + n - 1
    q0, q1 = qs + span - 1, qe - 1
    qq = [q0 + (q1 - q0) * i // (n - 1) for i in range(n)] if n > 1 else [q1]
    if n == 1:
        assert qe - qs == span
    an = [(tid, rs + span - 1 + (x - q0), x, span, rev) for x in qq]
    f = [score * (i + 1) // n for i in range(n)]
    f[-1] = score
    return an, f, [-1] + list(range(n - 1))


def add_chains(b, qlen, specs):
    an, f, p = [], [], []
    for s in specs:
        a, ff, pp = chain_anchors(**s)
        p.extend(x + len(an) if x >= 0 else -1 for x in pp)
        an.extend(a); f.extend(ff)
    return b.query(qlen, an, f, p)


def case_sel_counts(per_target):
    """63, 64, 65 and 129 chains per query on random overlapping intervals: primaries, secondaries, best_n reached and passed, ties"""
    rng = np.random.default_rng(31 + per_target)
    b = Build("sel_counts_pt%d" % per_target, opts(flags=MF_PER_TARGET if per_target else 0, min_cnt=1, min_chain_score=20, best_n=3), tlens=(50000,) * 3)
    for nch in (63, 64, 65, 129):
        specs = []
        for _ in range(nch):
            ln = int(rng.integers(40, 400)); qs = int(rng.integers(0, 3000 - ln))
            specs.append(dict(tid=int(rng.integers(0, 3)), rs=int(rng.integers(0, 40000)), qs=qs, qe=qs + ln, score=int(rng.integers(30, 90)),
                              n=int(rng.integers(2, 4)), rev=int(rng.integers(0, 2))))
        add_chains(b, 3000, specs)

    def reach(out, case):
        for q, nch in enumerate((63, 64, 65, 129)):
            c, k = chains_of(out, q), kept_of(out, q)
            assert len(c) == nch and 3 < len(k) < nch and len(set(c[:, 1])) < nch
        assert np.sum(out["parents"] >= 0) >= 3 * 4
    return b.done(reach, "chains per query at the round edges of k_select1")


def case_sel_spill(nprim):
    """`nprim` primaries on disjoint intervals (chains of one to three anchors); secondaries under the first, the middle and the LAST
    primaries, so that with more than SEL_PCAP = 1024 of them the masking interval and the parent's score are read from the spill;
    one secondary under each of the last two sits just below pri_ratio x parent.  Where enough primaries are spilled, the last three
    are short low-scoring chains in the gaps between earlier ones: a spilled interval read with a wrong start or end swallows them"""
    b = Build("sel_spill_%d" % nprim, opts(min_cnt=1, min_chain_score=20, best_n=20, pri_ratio=0.8, mask_level=0.5), tlens=(100000,))
    gaps = (3, 700, 1020) if nprim >= SEL_PCAP + 8 else ()
    nreg = nprim - len(gaps)
    specs = []
    for j in range(nreg):
        n = 1 + j % 3
        specs.append(dict(tid=0, rs=100 + 40 * j, qs=10 + 40 * j, qe=10 + 40 * j + (15 if n == 1 else 30), score=20000 - 4 * j, n=n))
    under = sorted(set(j for j in (0, 500, 1022, 1023, 1024, 1025, 1030, nreg - 3, nreg - 2, nreg - 1) if j < nreg))
    for j in under:
        s = dict(specs[j]); s["score"] -= 1; s["n"] = 2; s["qe"] = s["qs"] + 30
        specs.append(s)
    low = (nreg - 2, nreg - 1)
    for j in low:           # 0.8 x (20000 - 4 j) is above 12000: dropped if the parent's score is read right, kept if it reads as anything below 15000
        s = dict(specs[j]); s["score"] = 12000; s["n"] = 2; s["qe"] = s["qs"] + 30
        specs.append(s)
    for x, j in enumerate(gaps):
        specs.append(dict(tid=0, rs=140 + 40 * j, qs=40 + 40 * j, qe=50 + 40 * j, score=100 - x, n=1, span=10))
    add_chains(b, 40 * nprim + 100, specs)

    def reach(out, case):
        k = kept_of(out, 0)
        assert len(chains_of(out, 0)) == nprim + len(under) + 2
        assert np.sum(out["parents"] < 0) == nprim and len(k) == nprim + len(under)
        assert out["parents"].max() == nreg - 1
        if nprim > SEL_PCAP:
            assert out["parents"].max() >= SEL_PCAP and np.sum(out["parents"] >= SEL_PCAP) == sum(j >= SEL_PCAP for j in under)
        if gaps:
            assert list(k[-3:, 1]) == [100, 99, 98] and nreg - SEL_PCAP >= 64         # primaries that come after a block of spilled ones
    return b.done(reach, "%d primaries: %s of LDS" % (nprim, "past the end" if nprim > SEL_PCAP else "inside"))


def case_sel_spill_targets():
    """TELR_MF_PER_TARGET, 1100 targets with one primary each on the SAME query interval, and secondaries on 140 of them in three
    rounds (best_n = 2: the third is dropped): tallies past the 64th and the 128th, parents past SEL_PCAP"""
    nt, ns = 1100, 140
    b = Build("sel_spill_targets", opts(flags=MF_PER_TARGET, min_cnt=1, min_chain_score=20, best_n=2), tlens=(2000,) * nt)
    specs = [dict(tid=t, rs=100, qs=50, qe=250, score=8900 + t, n=1 + t % 3, span=15) for t in range(nt)]
    for s in specs:
        if s["n"] == 1:
            s["qe"] = s["qs"] + 15
    for base in (8800, 8600, 8400):
        for t in range(ns):
            if base == 8400 and t % 2:
                continue
            specs.append(dict(tid=t, rs=100, qs=50, qe=80, score=base - t, n=2))
    for t in (0, 1, 70, 130):       # below pri_ratio x parent
        specs.append(dict(tid=t, rs=100, qs=50, qe=80, score=7000, n=2))
    add_chains(b, 400, specs)

    def reach(out, case):
        k = kept_of(out, 0)
        assert np.sum(out["parents"] < 0) == nt and len(k) == nt + 2 * ns
        assert np.sum(out["parents"] >= SEL_PCAP) >= 2 * 70                # primary of target t has rank nt - 1 - t
        sec = k[out["parents"] >= 0]
        assert len(set(sec[:, 4])) == ns > 128
    return b.done(reach, "per-target mode: 1100 primaries, 140 tallies")


def sel_threshold_case(per_target, secondary=1):
    flags = MF_PER_TARGET if per_target else 0
    mo = opts(flags=flags, min_cnt=1, min_chain_score=20, best_n=3, pri_ratio=0.8, mask_level=0.5, secondary=secondary)
    b = Build("sel_thresholds_pt%d_sec%d" % (per_target, secondary), mo, tlens=(50000, 50000))
    pr = np.float32(mo.pri_ratio)
    edge = min(s for s in range(700, 900) if not np.float32(s) < np.float32(1000) * pr)       # the lowest score that stays under a parent of 1000
    P = dict(tid=0, rs=1000, qs=1000, qe=1200, score=1000)
    # 0: the score edge of pri_ratio
    add_chains(b, 5000, [P, dict(P, qs=1010, qe=1100, score=edge), dict(P, qs=1100, qe=1190, score=edge - 1)])
    # 1: the overlap edge of mask_level: 50 of 100 is not masked, 51 is
    add_chains(b, 5000, [P, dict(P, qs=1150, qe=1250, score=500), dict(P, qs=951, qe=1051, score=499, n=3)])
    # 2: best_n reached exactly; 3: passed by one; 4: equal scores (discovery order decides which is dropped)
    add_chains(b, 5000, [P] + [dict(P, qs=1000 + 10 * i, qe=1100 + 10 * i, score=950 - i) for i in range(3)])
    add_chains(b, 5000, [P] + [dict(P, qs=1000 + 10 * i, qe=1100 + 10 * i, score=950 - i) for i in range(4)])
    add_chains(b, 5000, [P] + [dict(P, qs=1000 + 10 * i, qe=1100 + 10 * i, score=950, rs=1000 + 300 * i) for i in range(5)])
    # 5: the same on two targets: best_n per target, and a chain that overlaps only a primary of the OTHER target
    add_chains(b, 5000, [P, dict(P, tid=1, score=990)] + [dict(P, tid=i % 2, qs=1000 + 10 * i, qe=1100 + 10 * i, score=950 - i) for i in range(8)])
    # 6: reverse strand: [4000, 4200) on the reverse strand of a query of 5000 is [800, 1000) forward, [3750, 3950) is [1050, 1250)
    # (masked only AFTER the flip, and below pri_ratio: dropped), [1100, 1300) is [3700, 3900) (masked only WITHOUT the flip: kept)
    add_chains(b, 5000, [P, dict(P, qs=4000, qe=4200, rev=1, score=900), dict(P, qs=3750, qe=3950, rev=1, score=700, rs=3000),
                         dict(P, qs=1100, qe=1300, rev=1, score=700, rs=5000)])
    # 7: a chain whose first minimizer ends before base span - 1 of its target: rs clamps to 0
    b.query(5000, [(1, 5, 300, 15, 0), (1, 105, 400, 15, 0)], [30, 60], [-1, 0])

    def reach(out, case):
        n = [len(kept_of(out, q)) for q in range(8)]
        sec = n if secondary else None
        if secondary:
            assert n[0] == 2 and kept_of(out, 0)[1, 1] == edge and n[1] == 2 and kept_of(out, 1)[1, 1] == 500
            assert n[2] == 4 and n[3] == 4 and n[4] == 4 and list(kept_of(out, 4)[:, 5]) == [1000, 1000, 1300, 1600]
            assert n[5] == (8 if per_target else 4)
            assert n[6] == 3 and list(kept_of(out, 6)[:, 1]) == [1000, 900, 700] and kept_of(out, 6)[2, 5] == 5000
        else:
            assert n[:7] == [1, 2, 1, 1, 1, 2 if per_target else 1, 3] and sec is None
        assert tuple(chains_of(out, 7)[0, 5:9]) == (0, 106, 286, 401)
    return b.done(reach, "the thresholds of select_chains")


# ---- segmenting ---------------------------------------------------------------------------------------------------


def seg_query(b, pts, rev=0, qlen=None, tid=0, span=15):
    """one chain through the points (r, q)"""
    n = len(pts)
    return b.query(qlen, [(tid, r, q, span, rev) for r, q in pts], [40 + 10 * i for i in range(n)], list(range(-1, n - 1)))


def case_seg_windows(bw_long):
    """one kept chain per query: 1 .. 129 anchors, every anchor a cut (64 cuts per window), no cut in a whole window (only the forced
    one at the last anchor), a cut at lane 63, one axis far enough and the other not; both strands"""
    K = 200
    mo = opts(flags=MF_CIGAR, min_cnt=1, min_chain_score=20, min_ksw_len=K, bw_long=bw_long)
    T = 200000
    b = Build("seg_windows_bwlong%d" % bw_long, mo, tlens=(T,))
    counts = (1, 2, 63, 64, 65, 128, 129)
    what = []
    for rev in (0, 1):
        for n in counts:
            seg_query(b, [(1000 + K * i, 500 + K * i) for i in range(n)], rev, qlen=500 + K * n + 700, span=K); what.append(("all", n))      # (the span reaches min_ksw_len: anchor 0 is a cut too)
            seg_query(b, [(1000 + i, 500 + i) for i in range(n)], rev, qlen=2000); what.append(("none", n))
        seg_query(b, [(1000 + i, 500 + K * i) for i in range(110)], rev, qlen=500 + K * 110 + 50); what.append(("q_only", 110))
        seg_query(b, [(1000 + K * i, 500 + i) for i in range(110)], rev, qlen=2000); what.append(("r_only", 110))

    def reach(out, case):
        kept, po, pr = out["kept"], out["prob_off"], out["probs"]
        assert len(kept) == len(what) and list(kept[:, 0]) == list(range(len(what)))
        for x, (kind, n) in enumerate(what):
            fills = pr[po[x]:po[x + 1]]
            fills = fills[np.isin(fills[:, 8], (0, 3, 5))]
            if kind == "all":
                assert len(fills) == n
            elif kind in ("none", "q_only", "r_only"):
                assert len(fills) == 1
        assert set(pr[:, 8]) >= ({0, 1, 2, 5} if bw_long else {0, 1, 2, 3})
        assert np.diff(po).max() == 129 + 2                                # 129 cuts in three windows, and both extensions
    return b.done(reach, "windows of k_segments_w")


def case_seg_lane63():
    """the first cut on anchor 63 exactly (lane 63 of window 0), none in window 1, the next on anchor 130"""
    mo = opts(flags=MF_CIGAR, min_cnt=1, min_chain_score=20, min_ksw_len=201)
    b = Build("seg_lane63", mo, tlens=(50000,))
    for rev in (0, 1):
        for n in (64, 65, 129, 131, 200):
            seg_query(b, [(3000 + 3 * i, 2000 + 3 * i) for i in range(n)], rev, qlen=4000, span=12)

    def reach(out, case):
        po, pr = out["prob_off"], out["probs"]
        for x, n in enumerate((64, 65, 129, 131, 200) * 2):
            fills = pr[po[x]:po[x + 1]]
            fills = fills[fills[:, 8] == 0]
            pos, last, want = [3 * i + 12 for i in range(n)], 0, []          # distance of anchor i's end from the chain's start, on both axes
            assert pos[62] < 201 == pos[63]
            for i in range(n):
                if i == n - 1 or pos[i] - last >= 201:
                    want.append(pos[i] - last); last = pos[i]
            assert want[0] == 201 and (n < 131 or want[1] == 201)            # cuts on anchor 63 and, 67 anchors on, on anchor 130
            assert list(fills[:, 4]) == want and list(fills[:, 5]) == want, (n, fills[:, 4], want)
    return b.done(reach, "a cut at lane 63")


def case_seg_geometry(bw_long):
    """extensions present and absent (qs == 0, rs == 0, qe == qlen, re == tlen), their clamps (ext_max, mq + ext_band, the sequence
    ends), fills with m + n on both sides of ADAPT_MAX_STEPS, |n - m| on both sides of bw (kind 5 under bw_long > bw) and bands on
    both sides of DP_DMAX (kind 3); both strands"""
    mo = opts(flags=MF_CIGAR, min_cnt=1, min_chain_score=20, min_ksw_len=200, bw_long=bw_long, max_gap=5000)
    T, Q = 30000, 20000
    b = Build("seg_geometry_bwlong%d" % bw_long, mo, tlens=(T, T))
    em, eb = mo.ext_max, mo.ext_band
    for rev in (0, 1):
        for tid in (0, 1):
            # starts: at base 0 of the query / of the target / of both / inside both (short, at the clamps, beyond them)
            for r0, q0 in ((5000, 14), (14, 5000), (14, 14), (15, 15), (100, 50), (50, 100), (em + 14, em + 14), (em + 15 + eb, em + 15),
                           (em + 14 + eb, em + 14), (9000, em + 500), (em + 20, 9000), (1014, 9000)):
                seg_query(b, [(r0, q0), (r0 + 300, q0 + 300)], rev, qlen=Q, tid=tid)
            # ends
            for r1, q1 in ((T - 1, 9000), (9000, Q - 1), (T - 1, Q - 1), (T - 2, Q - 2), (T - 40, Q - 90), (T - 90, Q - 40),
                           (T - 1 - em, Q - 1 - em), (T - 2 - em - eb, Q - 2 - em), (T - 3000, Q - 5000)):
                seg_query(b, [(r1 - 300, q1 - 300), (r1, q1)], rev, qlen=Q, tid=tid)
        # fills (second point to third): (m, n)
        for m, n in ((500, 500), (500, 501), (501, 500), (300, 300 + mo.bw), (300, 301 + mo.bw), (301 + mo.bw, 300), (300 + mo.bw, 300),
                     (300, 4500), (4500, 300), (2000, 6068), (2000, 6069), (250, 4900), (200, 200), (4000, 4000)):
            seg_query(b, [(2000, 2000), (2300, 2300), (2300 + n, 2300 + m)], rev, qlen=Q)

    def reach(out, case):
        pr = out["probs"]
        kinds = set(pr[:, 8])
        assert kinds == ({0, 1, 2, 5} if bw_long else {0, 1, 2, 3}), kinds
        ext = pr[np.isin(pr[:, 8], (1, 2))]
        assert ext[:, 4].max() == em and ext[:, 5].max() == em + eb and ext[:, 4].min() == 1 and ext[:, 5].min() == 1
        assert np.any((ext[:, 4] == em) & (ext[:, 5] < em)) and np.any((ext[:, 4] < em) & (ext[:, 5] == ext[:, 4] + eb))
        assert len(out["kept"]) == len(case["qlen"])
        has_l = np.array([np.any(pr[a:z, 8] == 1) for a, z in zip(out["prob_off"][:-1], out["prob_off"][1:])])
        has_r = np.array([np.any(pr[a:z, 8] == 2) for a, z in zip(out["prob_off"][:-1], out["prob_off"][1:])])
        assert np.any(has_l & ~has_r) and np.any(~has_l & has_r) and np.sum(~has_l) >= 3 * 4 and np.sum(~has_r) >= 3 * 4
        fills = pr[np.isin(pr[:, 8], (0, 3, 5))]
        steps = fills[:, 4] + fills[:, 5]
        assert np.any(steps == ADAPT_MAX_STEPS) and np.any(steps == ADAPT_MAX_STEPS + 1)
        wide = fills[:, 7] - fills[:, 6] + 1
        if not bw_long:
            assert np.any((fills[:, 8] == 0) & (wide == DP_DMAX)) and np.any((fills[:, 8] == 3) & (wide == DP_DMAX + 1))
        else:
            dl = np.abs(fills[:, 5] - fills[:, 4])
            assert np.any((fills[:, 8] == 0) & (dl == mo.bw)) and np.any((fills[:, 8] == 5) & (dl == mo.bw + 1))
    return b.done(reach, "extension and fill geometry")


# ---- random -------------------------------------------------------------------------------------------------------


def case_random(seed, flags=0, lookback=128):
    """a few thousand anchors over about 50 queries: random forests on both strands of three targets, random spacing"""
    rng = np.random.default_rng(seed)
    mo = opts(flags=MF_CIGAR | flags, chain_lookback=lookback, min_cnt=2, min_chain_score=25, min_ksw_len=60, best_n=2)
    b = Build("random_%d" % seed, mo, tlens=(40000, 30000, 50000))
    for _ in range(50):
        if rng.random() < 0.1:
            b.query(int(rng.integers(0, 500)))
            continue
        an, f, p = [], [], []
        for tid in rng.permutation(3)[:rng.integers(1, 4)]:
            for rev in rng.permutation(2)[:rng.integers(1, 3)]:
                n = int(rng.integers(1, 90))
                r = 20 + np.cumsum(rng.integers(1, 90, n)); q = 20 + np.cumsum(rng.integers(1, 90, n))
                ff, pp = random_forest(rng, n, lookback if not flags & MF_CHAIN_SKIP else 700, p_root=0.1)
                p.extend(int(x) + len(an) if x >= 0 else -1 for x in pp)
                f.extend(int(x) for x in ff)
                an.extend((int(tid), int(r[i]), int(q[i]), int(rng.integers(10, 20)), int(rev)) for i in range(n))
        b.query(9000, an, f, p)

    def reach(out, case):
        assert 2000 < len(case["keys"]) < 20000 and len(out["chains"]) > 100 and len(out["kept"]) > 60 and np.sum(out["parents"] >= 0) > 5
        assert len(out["kept"]) < len(out["chains"]) and len(out["probs"]) > len(out["kept"])
    return b.done(reach, "random forests")


def case_over_cap():
    """one query with more peaks than SEGSORT_CAP: the peak sort takes the library fall-back; most peaks are single anchors that
    min_cnt drops, a few hundred are chains of two"""
    rng = np.random.default_rng(5)
    n = 21600
    f = rng.integers(40, 2000, n); p = np.full(n, -1, np.int64)
    for i in range(50, n, 50):
        p[i] = i - 1; f[i - 1] = 20; f[i] = int(rng.integers(60, 400))
    b = Build("bt_over_cap", opts(chain_lookback=64, min_cnt=2, min_chain_score=30), tlens=(300000,))
    b.query(n * 10 + 300, line(n), f, p)
    b.query(900, line(70), *random_forest(rng, 70, 64))

    def reach(out, case):
        f, p = case["f"][:n], case["p"][:n]
        child = np.zeros(n, bool); child[p[p >= 0]] = True
        assert np.sum(~child & (f >= 30)) > SEGSORT_CAP
        c = chains_of(out, 0)
        assert len(c) == n // 50 - 1 and len(set(c[:, 1])) < len(c) and len(chains_of(out, 1)) > 0
    return b.done(reach, "more peaks than one workgroup sorts in LDS")


_CASES = None


def cases():
    """every case, built once (the list is shared: treat it as read-only)"""
    global _CASES
    if _CASES is None:
        _CASES = [case_sizes(64), case_sizes(128), case_sizes(256), case_path64(), case_lookback(64), case_lookback(128), case_lookback(256),
                  case_scan_ring(), case_forest(), case_peaks((63, 64, 65, 128, 129), "bt_peaks_small"),
                  case_peaks((512, 513, 1024, 1025), "bt_peaks_tiers"), case_over_cap(),
                  case_sel_counts(0), case_sel_counts(1), case_sel_spill(1023), case_sel_spill(1024), case_sel_spill(1025), case_sel_spill(1100),
                  case_sel_spill_targets(), sel_threshold_case(0), sel_threshold_case(1), sel_threshold_case(0, secondary=0),
                  sel_threshold_case(1, secondary=0), case_seg_windows(20000), case_seg_windows(0), case_seg_lane63(),
                  case_seg_geometry(20000), case_seg_geometry(0), case_random(1), case_random(2, flags=MF_CHAIN_SKIP)]
        assert len(set(c["name"] for c in _CASES)) == len(_CASES)
    return _CASES


_REF = {}


def oracle_out(case):
    """the oracle tap's output on a case, computed once per process and shared"""
    from oracle import binding as ob
    if case["name"] not in _REF:
        _REF[case["name"]] = ob.debug_backtrack(case["keys"], case["q_aoff"], case["f"], case["p"], case["qlen"], case["goff"], case["tlen"], case["mo"])
    return _REF[case["name"]]
