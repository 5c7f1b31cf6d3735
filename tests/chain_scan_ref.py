"""A restatement in Python of minimap2's chaining scan as the oracle runs it under TELR_MF_CHAIN_SKIP (0x1000: oracle/telr_oracle.c,
chain_dp), and the hand-built anchor lists that aim at its edges.  The restatement is checked against the oracle's f / p in
tests/test_chain_skip_cpu.py; the GPU tests hold telr_debug_chain to it on the hand-built lists.

Anchors are the engine's 64-bit keys: strand << 63 | global reference position << 32 | query position << 8 | span."""
import numpy as np

MAX_ITER = 5000
MAX_SKIP = 25
INT32_MIN = -(1 << 31)


def key(g, q, span=15, rev=0):
    return (rev << 63) | (g << 32) | (q << 8) | span


def _ilog2_q8(v):
    v = np.asarray(v, np.int64)
    e = np.floor(np.log2(np.maximum(v, 1))).astype(np.int64)
    # exact integer log2 (log2 of a float can round up just below a power of two)
    e = np.where((1 << e) > v, e - 1, e)
    e = np.where((1 << (e + 1)) <= v, e + 1, e)
    frac = np.where(e <= 8, (v << np.maximum(8 - e, 0)) - 256, (v >> np.maximum(e - 8, 0)) - 256)
    return e * 256 + frac


def chain_scores(ai, aj, mo):
    """the oracle's chain_sc(a[i], a[j]) for an array of predecessors aj; INT32_MIN where the link is not allowed"""
    ai = int(ai)
    aj = np.asarray(aj, np.uint64)
    ri, gi, qi, si = ai >> 63, (ai >> 32) & 0x7fffffff, (ai >> 8) & 0xffffff, ai & 0xff
    rj = (aj >> np.uint64(63)).astype(np.int64)
    gj = ((aj >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(np.int64)
    qj = ((aj >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.int64)
    dr, dq = gi - gj, qi - qj
    bw = max(mo.bw_long, mo.bw)
    dd = np.abs(dr - dq)
    ok = (rj == ri) & (dq > 0) & (dq <= mo.max_gap) & (dr > 0) & (dr <= mo.max_gap) & (dd <= bw)
    dg = np.minimum(dr, dq)
    sc = np.minimum(si, dg)
    pen = mo.chain_gap_q8 * dd + mo.chain_skip_q8 * dg + np.where(dd >= 1, _ilog2_q8(dd + 1) >> 1, 0)
    sc = np.where((dd != 0) | (dg > si), sc - (pen >> 8), sc)
    return np.where(ok, sc, INT32_MIN)


def chain_scan(a, mo, stats=None):
    """f, p of one query's sorted anchor list a under the scan (p relative to the list, -1 for none).  stats (a dict), if given,
    collects 'breaks' (scans ended by the 25-skip rule) and 'max_link' (largest i - p[i])."""
    a = np.asarray(a, np.uint64)
    n = len(a)
    f = np.zeros(n, np.int64)
    p = np.full(n, -1, np.int64)
    rev = (a >> np.uint64(63)).astype(np.int64)
    g = ((a >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(np.int64)
    st = 0
    breaks = scanned = 0
    for i in range(n):
        while st < i and (rev[st] != rev[i] or g[i] - g[st] > mo.max_gap):
            st += 1
        if i - st > MAX_ITER:
            st = i - MAX_ITER
        best, bp = int(a[i] & np.uint64(0xff)), -1
        if st < i:
            js = np.arange(i - 1, st - 1, -1)
            sc = chain_scores(a[i], a[js], mo)
            valid = sc != INT32_MIN
            v = np.where(valid, f[js] + sc, np.iinfo(np.int64).min)
            # a predecessor lies on a chain through i once a valid predecessor above it (scanned before it) has it as its parent
            marked = np.zeros(i - st, bool)
            pj = p[js][valid]
            pj = pj[pj >= st]
            marked[i - 1 - pj] = True
            # the new maxima (strictly larger than the best so far), in scan order
            run = np.maximum.accumulate(np.concatenate(([best], v)))[:-1]
            imp = valid & (v > run)
            n_skip = 0
            cut = len(js)
            for k in np.flatnonzero(imp | (valid & marked)):
                if imp[k]:
                    n_skip = max(0, n_skip - 1)
                else:
                    n_skip += 1
                    if n_skip > MAX_SKIP:
                        cut = k
                        breaks += 1
                        break
            scanned += min(cut + 1, len(js))
            ik = np.flatnonzero(imp[:cut])
            if len(ik):
                best, bp = int(v[ik[-1]]), int(js[ik[-1]])
        f[i], p[i] = best, bp
    if stats is not None:
        stats["breaks"] = stats.get("breaks", 0) + breaks
        stats["scanned"] = stats.get("scanned", 0) + scanned          # predecessors looked at, the breaking one included
        stats["anchors"] = stats.get("anchors", 0) + n
        links = np.arange(n)[p >= 0] - p[p >= 0]
        stats["max_link"] = max(stats.get("max_link", 0), int(links.max()) if len(links) else 0)
    return f.astype(np.int32), p.astype(np.int32)


def chain_scan_all(anchors, anchor_off, mo, stats=None):
    """chain_scan over every query of a concatenated list (anchor_off: nq + 1 offsets)"""
    f = np.zeros(len(anchors), np.int32)
    p = np.zeros(len(anchors), np.int32)
    for q in range(len(anchor_off) - 1):
        s, e = int(anchor_off[q]), int(anchor_off[q + 1])
        f[s:e], p[s:e] = chain_scan(anchors[s:e], mo, stats)
    return f, p


# ---- hand-built lists ----------------------------------------------------------------------------------------------------
# Every case: (name, [list of uint64 keys per query], {query: {anchor: expected p}} checked by hand).  The options: map-ont with
# the scan and without the long join (bw 500), so that diagonals 700 apart cannot link.

def _skip_edge(m, z=False):
    """anchor I scans a chain C_m .. C_1 (C_m improves, every other C_k is the parent of C_{k+1}: marked, not improving) and below
    it a better chain X: with m = 26 the 25th mark is the last one and X_59 wins, with m = 27 the 26th mark breaks the scan and C_m
    stays.  z: one more predecessor Z between C_2 and C_1 that improves (taking one from n_skip just before the break) but is worse
    than X_59: with m = 27 the scan then reaches X_59 after all."""
    X = [key(1000 + 10 * k, 1000 + 10 * k) for k in range(60)]                 # diagonal 0, f = 15 + 10 k
    C = [key(1700 + 10 * k, 1000 + 10 * k) for k in range(1, m + 1)]           # diagonal 700, f = 15 + 10 (k - 1)
    Z = [key(1715, 1515)] if z else []                                         # diagonal 200: linked from X_51, f = 502
    I = [key(2050, 1700)]                                                      # diagonal 350: links from X, C and Z
    keys = sorted(X + C + Z) + I
    return keys


def hand_cases():
    cases = []
    k = _skip_edge(26)
    cases.append(("25 marks: the scan reaches X_59", [k], {0: {len(k) - 1: 59}}))
    k = _skip_edge(27)
    cases.append(("26 marks: the scan breaks before X_59", [k], {0: {len(k) - 1: len(k) - 2}}))
    k = _skip_edge(27, z=True)
    cases.append(("a new maximum just before the break keeps the scan going", [k], {0: {len(k) - 1: 59}}))
    # equal scores: J1 (diagonal -10) and J2 (diagonal +10) cannot link (J2's query position is below J1's) and lie equally far from
    # I (diagonal 0): the nearer one (higher index) is taken, the other one does not improve
    J = [key(1000, 1010), key(1010, 1000), key(1100, 1100)]
    cases.append(("equal scores: the higher index wins", [J], {0: {2: 1}}))
    # look-back of exactly 5,000 anchors (reached) and 5,001 (not): anchor 0 links to the last one, the fillers between link to nothing
    for nf in (4999, 5000):
        fill = [key(110, 200000 + t) for t in range(nf)]
        L = [key(100, 100)] + fill + [key(120, 120)]
        cases.append(("look-back %d" % (nf + 1), [L], {0: {nf + 1: 0 if nf == 4999 else -1}}))
    # reference distance max_gap (linked) and max_gap + 1 (not): the st bound and the link test agree at the edge
    for d in (5000, 5001):
        L = [key(1000, 1000), key(1000 + d, 1000 + min(d, 5000))]
        cases.append(("reference distance %d" % d, [L], {0: {1: 0 if d == 5000 else -1}}))
    # a strand boundary inside one query: the reverse-strand anchors sit where forward ones would link to them
    L = [key(1000, 1000), key(1010, 1010), key(1020, 1020), key(1030, 1030, rev=1), key(1040, 1040, rev=1)]
    cases.append(("strand boundary", [L], {0: {1: 0, 2: 1, 3: -1, 4: 3}}))
    # empty and one-anchor queries between others
    cases.append(("empty and one-anchor queries", [[], [key(500, 500)], [], J, []], {1: {0: -1}, 3: {2: 1}}))
    # a query of more than 20,480 anchors (SEGSORT_CAP): chains on a few diagonals with random anchors between
    rng = np.random.default_rng(20261016)
    big = set()
    for d in (0, 40, 300, 2500):
        for t in range(0, 6000):
            big.add(key(10000 + d + 7 * t + int(rng.integers(0, 3)), 10000 + 7 * t, int(rng.integers(12, 20))))
    while len(big) < 24000:
        big.add(key(10000 + int(rng.integers(0, 45000)), int(rng.integers(0, 45000)), int(rng.integers(12, 20))))
    cases.append(("one query of 24,000 anchors", [sorted(big)], {}))
    return cases


def random_lists(seed, nq=40, lo=0, hi=3000):
    """random lists in the shape of real ones: a few collinear runs (with jitter) on both strands, repeat copies, scattered hits"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nq):
        n = int(rng.integers(lo, hi + 1))
        s = set()
        while len(s) < n:
            kind = rng.random()
            rev = int(rng.random() < 0.3)
            if kind < 0.7:
                d, g0, q0 = int(rng.integers(0, 3000)), int(rng.integers(0, 200000)), int(rng.integers(0, 20000))
                for t in range(int(rng.integers(5, 120))):
                    s.add(key(g0 + d + 9 * t + int(rng.integers(0, 12)), q0 + 9 * t + int(rng.integers(0, 6)), int(rng.integers(10, 20)), rev))
            else:
                s.add(key(int(rng.integers(0, 200000)), int(rng.integers(0, 20000)), int(rng.integers(10, 20)), rev))
        out.append(sorted(s)[:n])
    return out


def concat_lists(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    for i, L in enumerate(lists):
        off[i + 1] = off[i] + len(L)
    keys = np.array([x for L in lists for x in L], dtype=np.uint64)
    return keys, off


def hand_opts():
    from telr_amd.presets import preset
    _, mo = preset("map-ont", chain_skip=True)
    mo.bw_long = 0
    return mo
