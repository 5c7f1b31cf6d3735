"""DP problems aimed at the routing edges of the engine's DP classes, run through the engine's own DP pass (telr_debug_dp)
and through the CPU oracle's banded DP (tor_debug_dp), compared problem by problem.

The edges come from the library itself (telr_debug_dp_limits: the int16 bounds the host computes for a preset), so the
set follows the engine's numbers: band widths D at every class edge, fills and extensions of m + n = L - 1, L, L + 1 steps
for every bound L, an N on the first / last base of either window and just outside it, windows at every residue mod 32, both
strands, and waves of 1 / 63 / 64 / 65 / 129 problems (one long problem in front of 63 short ones included).

usage: python tests/dp_edges.py   (prints "dp edges ok: <problems> problems"; tests/test_gpu_dp_edges.py runs it once per TELR_AB switch)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

from telr_amd.aligner import Engine, SeqSet
from telr_amd.presets import preset

DP_DMAX = 4096              # kernels.hip.h: the widest band the DP kernels take (wider fills are kind 3)
ADAPT_MAX_STEPS = 1000      # fills above this many steps are never retried
PRESETS = ("map-ont", "map-pb", "asm10", "ngmlr-ont", "ngmlr-pacbio")
INTERLEAVED = (10, 11, 12, 13, 17)       # classes whose 64 problems share one interleaved trace-back piece
# the widest band of every class (the upper D edge a problem must reach)
UPPER_D = {17: 16, 10: 20, 11: 24, 12: 28, 13: 32, 14: 40, 15: 48, 16: 64, 22: 128, 19: 256, 20: 512, 21: 1024,
           18: 64, 23: 128, 24: 256, 5: 64, 6: 128, 7: 256, 8: 512, 9: 1024, 0: 64, 1: 128, 2: 256, 3: 1024, 4: DP_DMAX}
# the step bound each packed class is entered under
STEP_LIMIT = {**{c: "pk_steps_limit" for c in (10, 11, 12, 13, 14, 15, 16, 17, 22)},
              **{c: "pk_wide_limit" for c in (19, 20, 21)}, **{c: "pk_ext_limit" for c in (18, 23, 24)}}
# kind-0 band widths: both sides of every class edge, the widest kind-0 band, and bands only kind 3 takes
D_EDGES = (16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 40, 41, 48, 49, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096, 4097, 4098, 5000)
PACKED_FILL_D = (16, 20, 24, 28, 32, 40, 48, 64, 128)
WIDE_FILL_D = (256, 512, 1024)

_COMP = np.zeros(256, np.uint8)
_COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b
_ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- the routing, restated from kernels.hip.h (d_dp_class, k_prob_sizes) ------------------------------------------------
def d_dp_class(kind, D, steps, pk_max, pk_ext, pk_wide, wide_maxd=1024, ext_maxd=64):
    if kind in (1, 2) and steps <= pk_ext:
        if D <= 64:
            return 18
        if D <= 128 and ext_maxd >= 128:
            return 23
        if D <= 256 and ext_maxd >= 256:
            return 24
    if kind == 0 and steps <= pk_max:
        for c, hi in ((17, 16), (10, 20), (11, 24), (12, 28), (13, 32), (14, 40), (15, 48), (16, 64), (22, 128)):
            if D <= hi:
                return c
    if kind == 0 and steps <= pk_wide and 64 < D <= wide_maxd:
        for c, hi in ((19, 256), (20, 512), (21, 1024)):
            if D <= hi:
                return c
    if kind == 0:
        for c, hi in ((5, 64), (6, 128), (7, 256), (8, 512), (9, 1024)):
            if D <= hi:
                return c
    return 0 if D <= 64 else 1 if D <= 128 else 2 if D <= 256 else 3 if D <= 1024 else 4


def expect_class(kind, D, steps, lim, has_n):
    c = d_dp_class(kind, D, steps, lim["pk_steps_limit"], lim["pk_ext_limit"], lim["pk_wide_limit"], lim["pk_wide_maxd"], lim["pk_ext_maxd"])
    if c >= 10 and kind < 3 and has_n:          # the packed kernels have no ambiguity case
        c = d_dp_class(kind, D, steps, 0, 0, 0)
    if ((c == 17 and lim["tb4_mask"] & 1) or (c == 10 and lim["tb4_mask"] & 2)) and steps > lim["tb4_steps"]:
        c = 14                                  # the nibble cell keeps scores x4
    return c


def d_onep_d(q, e, q2, e2):
    return (q2 - q + (e - e2) - 1) // (e - e2) if e > e2 else 1 << 20


def even_lo(x):
    return x - (x & 1)


def fill_band(m, n, W):
    dl = n - m
    return even_lo(min(dl, 0) - W), max(dl, 0) + W


def band_width(m, n, W):
    lo, hi = fill_band(m, n, W)
    return hi - lo + 1


def ext_band(mo):
    return even_lo(-mo.ext_band), mo.ext_band


# ---- scoring sets -----------------------------------------------------------------------------------------------------------
def _mo(name, **kw):
    mo = preset(name)[1]
    mo.ext_max = max(mo.ext_max, 8192)          # (the tap checks windows against it: long extensions reach the step bounds)
    for k, v in kw.items():
        setattr(mo, k, v)
    return mo


def scoring_sets():
    """-> [(name, mo, scope)]; scope "full" (every shape) or "ext" (extensions only: the sets that move an extension bound)"""
    out = [(p, _mo(p), "full") for p in PRESETS]
    out.append(("affine-edge", _mo("map-ont", a=4, b=9, q=4, e=2, q2=63, e2=1, sc_ambi=9), "full"))
    for q2 in (19, 20, 23):            # d_onep_d = 15 / 16 / 19 (map-ont itself: 20): both tb4_mask bits flip
        mo = _mo("map-ont", q2=q2)
        assert d_onep_d(mo.q, mo.e, mo.q2, mo.e2) == q2 - 4
        out.append(("onep%d" % (q2 - 4), mo, "full"))
    # convex cost: the cheapest extension where pk_cx_ok(mo, D) changes (1024 | 512 | 256 | none), read off the library's limits
    prev = None
    for emin in range(0, 121):
        mo = _mo("ngmlr-ont", cx_ext_min=emin, cx_ext_max=max(20, emin))
        lim = Engine.dp_limits(mo)
        key = (lim["pk_wide_maxd"], lim["pk_wide_limit"] > 0, lim["pk_steps_limit"] > 0, lim["pk_ext_limit"] > 0)
        if prev is not None and key != prev[1]:
            for e2, m2 in ((emin - 1, prev[0]), (emin, mo)):
                if not any(n == "cx-emin%d" % e2 for n, _, _ in out):
                    out.append(("cx-emin%d" % e2, m2, "full"))
        prev = (mo, key)
    for z in (4000, 4001):
        out.append(("zdrop%d" % z, _mo("map-ont", zdrop=z), "ext"))
    for z in (30000, 30001):           # convex z-drop x S at the bound: ngmlr-ont's scores at S = 1
        out.append(("cx-zdropS%d" % z, _mo("ngmlr-ont", a=20, b=20, sc_ambi=10, cx_scale=1, zdrop=z), "ext"))
    for eb in (31, 32, 63, 64, 127, 128, 511):      # extension bands D = 64 | 65, 128 | 129, 256 | 257, 1024
        for z in (400, 4001):
            out.append(("ext%d-z%d" % (eb, z), _mo("map-ont", ext_band=eb, bw_long=0, zdrop=z), "ext"))
    return out


# ---- contents (DP order: A = the query as the DP reads it, B = the target) ------------------------------------------------
def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)]


def _fit(rng, s, n):
    return s[:n] if len(s) >= n else np.concatenate([s, _rand(rng, n - len(s))])


def _mutate(rng, s, rate):
    out, i = [], 0
    while i < len(s):
        r = rng.random()
        if r < rate / 3:
            out.append(_ACGT[rng.integers(0, 4)])       # substitution (may be silent)
            i += 1
        elif r < 2 * rate / 3:
            i += int(rng.integers(1, 4))                 # deletion
        elif r < rate:
            out.extend(_rand(rng, int(rng.integers(1, 4))))       # insertion
        else:
            out.append(s[i])
            i += 1
    return np.array(out, np.uint8)


CONTENTS = ("match", "mismatch", "bandedge", "homopolymer", "tandem", "err", "nrich")


def content(rng, kind, m, n):
    B = _rand(rng, n)
    if kind == "match":
        A = _fit(rng, B, m)
    elif kind == "mismatch":
        A = _fit(rng, _COMP[B], m)
    elif kind == "bandedge":            # one gap run of |m - n| in the middle: the path runs along a band edge
        if n >= m:
            A = np.concatenate([B[:m // 2], B[m // 2 + n - m:]])
        else:
            A = np.concatenate([B[:n // 2], _rand(rng, m - n), B[n // 2:]])
    elif kind == "homopolymer":
        c = _ACGT[rng.integers(0, 4)]
        A, B = np.full(m, c, np.uint8), np.full(n, c, np.uint8)
    elif kind == "tandem":
        unit = _rand(rng, int(rng.integers(2, 7)))
        rep = np.tile(unit, (max(m, n) + 8) // len(unit) + 2)
        ph = int(rng.integers(0, len(unit)))
        A, B = rep[:m].copy(), rep[ph:ph + n].copy()
    else:                               # err / nrich: 5-15 % random error (nrich: and 2 % N on both sides)
        A = _fit(rng, _mutate(rng, B, float(rng.uniform(0.05, 0.15))), m)
        if kind == "nrich":
            A = A.copy()
            A[rng.random(m) < 0.02] = ord("N")
            B[rng.random(n) < 0.02] = ord("N")
    return A.astype(np.uint8), B.astype(np.uint8)


# ---- problems -------------------------------------------------------------------------------------------------------------
# strands as the map path combines them (k_segments_w): (qstep, tstep, qcomp) per kind, forward and reverse read
STRANDS = {0: ((1, 1, 0), (-1, 1, 1)), 3: ((1, 1, 0), (-1, 1, 1)), 5: ((1, 1, 0), (-1, 1, 1)),
           1: ((-1, -1, 0), (1, -1, 1)), 2: ((1, 1, 0), (-1, 1, 1))}
NPOS = ("q_first", "q_last", "q_before", "q_after", "t_first", "t_last", "t_before", "t_after")


class Prob:
    __slots__ = ("kind", "m", "n", "dlo", "dhi", "strand", "A", "B", "npos", "tag")

    def __init__(self, kind, m, n, dlo, dhi, strand, A, B, npos=None, tag=""):
        self.kind, self.m, self.n, self.dlo, self.dhi, self.strand = kind, m, n, dlo, dhi, strand
        self.A, self.B, self.npos, self.tag = A, B, npos, tag


def _store(window_dp, step, comp, lo, flank_l, flank_r):
    w = _COMP[window_dp] if comp else window_dp
    if step < 0:
        w = w[::-1]
    return np.concatenate([flank_l, w, flank_r]), (lo if step > 0 else lo + len(window_dp) - 1)


def materialize(rng, probs):
    """-> (query seqs, target seqs, (np, 12) int32 problem rows): every problem on a query and a target of its own, the windows
    starting at residue (index mod 32) of the problem's number, 32 bases of flank on either side"""
    qs, ts, rows = [], [], []
    for x, p in enumerate(probs):
        qstep, tstep, qcomp = STRANDS[p.kind][p.strand]
        rq, rt = x % 32, (7 * x + 3) % 32
        fl = lambda k: _rand(rng, k)
        qseq, q_off = _store(p.A, qstep, qcomp, 32 + rq, fl(32 + rq), fl(32 + (5 * x) % 32))
        tseq, t_off = _store(p.B, tstep, 0, 32 + rt, fl(32 + rt), fl(32 + (11 * x) % 32))
        if p.npos:                      # one N at a window edge (first / last stored base) or just outside it
            which, where = p.npos.split("_")
            seq, lo, ln = (qseq, 32 + rq, p.m) if which == "q" else (tseq, 32 + rt, p.n)
            seq[{"first": lo, "last": lo + ln - 1, "before": lo - 1, "after": lo + ln}[where]] = ord("N")
        qs.append(qseq.tobytes())
        ts.append(tseq.tobytes())
        rows.append((x, q_off, x, t_off, p.m, p.n, p.dlo, p.dhi, p.kind, qstep, tstep, qcomp))
    return qs, ts, np.array(rows, np.int32).reshape(-1, 12)


def fill_shape(rng, D, edge=False):
    """(m, n, W) of a fill whose band has exactly D diagonals; edge: |m - n| takes nearly all of it (W 0..3)"""
    for _ in range(200):
        if edge:
            W = int(rng.integers(0, 4))
            dl = (D - 2 * W - 1) * (1 if rng.random() < 0.5 else -1)
        else:
            W = max(0, (D - 1) // 2 - int(rng.integers(0, 5)))
            dl = int(rng.integers(-8, 9))
        m = int(rng.integers(30, 300)) + max(0, -dl)
        n = m + dl
        for w in (W, W - 1, W + 1):
            if w >= 0 and n >= 1 and band_width(m, n, w) == D:
                return m, n, w
    raise AssertionError("no fill shape for D=%d" % D)


def fill(rng, D, cont, strand, m=None, n=None, W=None, npos=None, tag=""):
    if m is None:
        m, n, W = fill_shape(rng, D, edge=cont == "bandedge")
    lo, hi = fill_band(m, n, W)
    assert hi - lo + 1 == D
    A, B = content(rng, cont, m, n)
    return Prob(0 if D <= DP_DMAX else 3, m, n, lo, hi, strand, A, B, npos, tag)


def fill_steps(rng, D, steps, cont, strand, tag=""):
    """a fill of exactly `steps` = m + n and D diagonals (|m - n| <= 1)"""
    m = steps // 2
    n = steps - m
    for dl_sign in (1, -1):
        mm, nn = (m, n) if dl_sign > 0 else (n, m)
        for W in range(max(0, D // 2 - 3), D // 2 + 2):
            if band_width(mm, nn, W) == D:
                return fill(rng, D, cont, strand, mm, nn, W, tag=tag)
    raise AssertionError("no fill of %d steps, D=%d" % (steps, D))


def extension(rng, mo, kind, cont, strand, m=None, n=None, npos=None, tag=""):
    lo, hi = ext_band(mo)
    if m is None:
        m = int(rng.integers(30, 600))
        n = max(1, m + int(rng.integers(-20, mo.ext_band + 1)))
    assert m <= mo.ext_max and n <= m + mo.ext_band
    A, B = content(rng, cont, m, n)
    return Prob(kind, m, n, lo, hi, strand, A, B, npos, tag)


def longgap(rng, mo, strand, ins, cont):
    """kind 5 (long join): a segment whose lengths differ by more than bw, one long gap between two matching ends"""
    S, g = int(rng.integers(60, 240)), mo.bw + int(rng.integers(1, 200))
    B = _rand(rng, S)
    left = int(rng.integers(10, S - 10))
    if cont == "err":
        A0 = _fit(rng, _mutate(rng, B, 0.08), S)
    else:
        A0 = B.copy()
    if ins:
        A, Bt = np.concatenate([A0[:left], _rand(rng, g), A0[left:]]), B
    else:
        A, Bt = A0, np.concatenate([B[:left], _rand(rng, g), B[left:]])
    lo, hi = ext_band(mo)
    return Prob(5, len(A), len(Bt), lo, hi, strand, A.astype(np.uint8), Bt.astype(np.uint8), tag="longgap")


def groups(mo, scope, lim, seed=1):
    """-> [(group name, [Prob])]: each group is one DP pass (the waves of a class are formed inside one pass)"""
    rng = np.random.default_rng(seed)
    G = []
    # 1. kind-0 / kind-3 band widths at every class edge, every content, both strands
    if scope == "full":
        ps = [fill(rng, D, c, s, tag="D") for D in D_EDGES for c in CONTENTS for s in (0, 1)]
        G.append(("D edges", ps))
        # 2. the N rule: an N on the first / last base of a window and just outside it
        ps = []
        for D in PACKED_FILL_D + WIDE_FILL_D:
            for s in (0, 1):
                for npos in NPOS:
                    ps.append(fill(rng, D, "err", s, npos=npos, tag="N"))
        G.append(("N fills", ps))
    # 3. extensions: contents, strands, the N rule
    ps = [extension(rng, mo, k, c, s, tag="ext") for k in (1, 2) for c in CONTENTS for s in (0, 1)]
    ps += [extension(rng, mo, k, "err", s, npos=npos, tag="N") for k in (1, 2) for s in (0, 1) for npos in NPOS]
    G.append(("extensions", ps))
    # 4. long-gap fills (presets with a long join)
    if scope == "full" and mo.bw_long > mo.bw and mo.ext_band <= 31:
        G.append(("long-gap fills", [longgap(rng, mo, s, ins, c) for s in (0, 1) for ins in (True, False) for c in ("match", "err")]))
    # 5. the step bounds: m + n = L - 1, L, L + 1 (one pass per step count: the two-piece tag decision is a wave's)
    bounds = []
    if scope == "full":
        if lim["pk_steps_limit"]:
            bounds.append(("pk_steps_limit", lim["pk_steps_limit"], [(0, D) for D in PACKED_FILL_D]))
        if lim["pk_wide_limit"]:
            bounds.append(("pk_wide_limit", lim["pk_wide_limit"], [(0, D) for D in WIDE_FILL_D if D <= lim["pk_wide_maxd"]] + [(0, 1024)]))
        if lim["tb4_mask"]:
            bounds.append(("tb4_steps", lim["tb4_steps"], [(0, D) for D, bit in ((16, 1), (20, 2)) if lim["tb4_mask"] & bit]))
        if lim["tag8_steps"]:
            bounds.append(("tag8_steps", lim["tag8_steps"], [(0, D) for D in (16, 20, 24, 32, 40, 48, 64, 128)]))
    if lim["pk_ext_limit"]:
        bounds.append(("pk_ext_limit", lim["pk_ext_limit"], [(1, None), (2, None)]))
    for name, L, shapes in bounds:
        for dL in (-1, 0, 1):
            steps = L + dL
            ps = []
            for kind, D in shapes:
                for c in ("match", "mismatch", "err"):
                    s = int(rng.integers(0, 2))
                    if kind == 0:
                        ps.append(fill_steps(rng, D, steps, c, s, tag="L:%s:%d" % (name, dL)))
                    else:
                        m = (steps + 1) // 2
                        if m <= mo.ext_max:
                            ps.append(extension(rng, mo, kind, c, s, m=m, n=steps - m, tag="L:%s:%d" % (name, dL)))
            if ps:
                G.append(("%s %+d" % (name, dL), ps))
    return G


def wave_groups(mo, lim, seed=2):
    """waves of 1 / 63 / 64 / 65 / 129 problems per class, and one long problem in front of 63 short ones"""
    rng = np.random.default_rng(seed)
    Ds = PACKED_FILL_D + tuple(D for D in WIDE_FILL_D if D <= lim["pk_wide_maxd"])
    G = []
    for cnt in (1, 63, 64, 65, 129):
        ps = []
        for D in Ds:
            for k in range(cnt):
                m = int(rng.integers(20, 160))
                ps.append(fill(rng, D, "err", k & 1, m, m, (D - 1) // 2 if D & 1 else (D - 2) // 2, tag="wave"))
        for kind in (1, 2):
            ps += [extension(rng, mo, kind, "err", k & 1, tag="wave") for k in range(cnt)]
        G.append(("waves of %d" % cnt, ps))
    ps = []
    for D in Ds:
        W = (D - 2) // 2
        ps.append(fill(rng, D, "err", 0, 700, 700, W, tag="wave"))
        for k in range(63):
            m = int(rng.integers(20, 60))
            ps.append(fill(rng, D, "err", k & 1, m, m, W, tag="wave"))
    for kind in (1, 2):
        ps.append(extension(rng, mo, kind, "match", 0, m=min(mo.ext_max, 1500), n=min(mo.ext_max, 1500), tag="wave"))
        for k in range(63):
            m = int(rng.integers(20, 60))
            ps.append(extension(rng, mo, kind, "err", k & 1, m=m, n=m + int(rng.integers(-10, min(10, mo.ext_band) + 1)), tag="wave"))
    G.append(("one long + 63 short", ps))
    return G


# ---- comparison -----------------------------------------------------------------------------------------------------------
def _dp_view(qs, ts, row):
    """the two windows in DP order as nt4 codes (4 = ambiguous)"""
    qid, q_off, tid, t_off, m, n, _, _, _, qstep, tstep, qcomp = (int(v) for v in row)
    q = np.frombuffer(qs[qid], np.uint8)
    t = np.frombuffer(ts[tid], np.uint8)
    qa = q[q_off + qstep * np.arange(m)]
    ta = t[t_off + tstep * np.arange(n)]
    if qcomp:
        qa = _COMP[qa]
    lut = np.full(256, 4, np.int8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    return lut[qa], lut[ta]


def mlen_of(cig, qa, ta):
    """matching M columns of a CIGAR over the DP-order windows"""
    i = j = ml = 0
    for w in cig:
        op, ln = int(w) & 0xf, int(w) >> 4
        if op == 0:
            a, b = qa[i:i + ln], ta[j:j + ln]
            ml += int(((a == b) & (a < 4)).sum())
            i += ln
            j += ln
        elif op == 1:
            i += ln
        else:
            j += ln
    return ml, i, j


def oracle_dp(qs, ts, mo, rows, threads=8):
    """binding.debug_dp over chunks of the list on a few threads (the C call releases the GIL)"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import binding as ob
    cut = np.linspace(0, len(rows), min(threads, max(1, len(rows) // 16)) + 1).astype(int)
    with ThreadPoolExecutor(len(cut) - 1) as ex:
        parts = list(ex.map(lambda k: ob.debug_dp(qs, ts, mo, rows[cut[k]:cut[k + 1]]), range(len(cut) - 1)))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("score", "bi", "bj", "touched")}
    out["cigars"] = [c for p in parts for c in p["cigars"]]
    return out


def run_group(eng, mo, lim, probs, rng, label):
    """one engine DP pass and the oracle over the same problems; -> (list of mismatch strings, [(cls, D, steps, tag)])"""
    qs, ts, rows = materialize(rng, probs)
    got = eng.debug_dp(SeqSet(eng, qs), SeqSet(eng, ts), mo, rows)
    ref = oracle_dp(qs, ts, mo, rows)
    bad, seen = [], []
    for x, p in enumerate(probs):
        row = rows[x]
        D, steps = p.dhi - p.dlo + 1, p.m + p.n
        qa, ta = _dp_view(qs, ts, row)
        has_n = bool((qa == 4).any() or (ta == 4).any())
        want = expect_class(p.kind, D, steps, lim, has_n)
        cls = int(got["cls"][x])
        seen.append((cls, D, steps, p.tag))
        where = "%s #%d (%s kind %d m %d n %d D %d strand %d npos %s)" % (label, x, p.tag, p.kind, p.m, p.n, D, p.strand, p.npos)
        errs = []
        if cls != want:
            errs.append("class %d, routing says %d" % (cls, want))
        for f in ("score", "bi", "bj"):
            if int(got[f][x]) != int(ref[f][x]):
                errs.append("%s %d != oracle %d" % (f, got[f][x], ref[f][x]))
        gc, rc = got["cigars"][x], ref["cigars"][x]
        if len(gc) != len(rc) or not np.array_equal(gc, rc):
            errs.append("CIGAR differs (%d vs %d ops)" % (len(gc), len(rc)))
        want_retry = int(p.kind == 0 and ref["touched"][x] != 0 and steps <= ADAPT_MAX_STEPS)
        if int(got["retry"][x]) != want_retry:
            errs.append("retry %d, oracle touched %d" % (got["retry"][x], ref["touched"][x]))
        ml, ci, cj = mlen_of(gc, qa, ta)
        if int(got["mlen"][x]) != ml:
            errs.append("mlen %d, CIGAR says %d" % (got["mlen"][x], ml))
        if (ci, cj) != (int(got["bi"][x]), int(got["bj"][x])):
            errs.append("CIGAR spans (%d, %d)" % (ci, cj))
        tb = int(got["tb_off"][x])
        if tb % (8 if cls in INTERLEAVED and p.kind < 3 else 64):
            errs.append("tb_off %d not line-aligned" % tb)
        if errs:
            bad.append(where + ": " + "; ".join(errs))
    return bad, seen


def run_set(eng, name, mo, scope, waves=False, seed=1):
    """-> (problem count, mismatches, coverage records (set name, cls, D, steps, tag))"""
    lim = Engine.dp_limits(mo)
    rng = np.random.default_rng(seed + 1000)
    G = groups(mo, scope, lim, seed)
    if waves:
        G += wave_groups(mo, lim, seed + 1)
    n, bad, cov = 0, [], []
    for gname, probs in G:
        b, seen = run_group(eng, mo, lim, probs, rng, "%s / %s" % (name, gname))
        n += len(probs)
        bad += b
        cov += [(name,) + s for s in seen]
    return n, bad, cov


def run_all(eng, waves_on=PRESETS):
    total, bad, cov, per_set = 0, [], [], {}
    for name, mo, scope in scoring_sets():
        n, b, c = run_set(eng, name, mo, scope, waves=name in waves_on)
        total += n
        bad += b
        cov += c
        per_set[name] = (n, sorted({r[1] for r in c}))
    return total, bad, cov, per_set


if __name__ == "__main__":
    import torch  # noqa: F401  (the engine binds to the HIP runtime torch loads)
    eng = Engine(0)
    total, bad, cov, per_set = run_all(eng)
    for name, (n, cls) in per_set.items():
        print("%-16s %6d problems, classes %s" % (name, n, " ".join(map(str, cls))))
    if bad:
        print("\n".join(bad[:40]))
        print("dp edges FAILED: %d of %d problems" % (len(bad), total))
        sys.exit(1)
    print("dp edges ok: %d problems" % total)
