"""DP problems whose optimal PATH is planted, aimed at the edges of the three trace-back walks (kernels.hip.h: d_traceback_rows,
k_traceback_w, d_traceback_lane), run through the engine's DP pass and the CPU oracle's banded DP with tests/dp_edges.py's machinery.

A path is given start to end as [(op, len)] (op "M" / "I" / "D"); plant() writes two windows that have it, and a case claims its
path only if the ORACLE's CIGAR for the windows equals it (seeds 0 .. SEEDS - 1 are drawn until it does).  The geometry of the
walks is restated here from Engine.dp_class_table() and the walks' offset formulas, so every family reports which edges its
realised paths hit (tests/test_tb_paths_ref.py asserts them; no device needed for that):

  A  packed fills through d_traceback_rows (classes 17, 10-16, 22): diagonal runs of 1 .. 9 between two gaps on every row phase of
     the class's 64-byte line, first runs of 0 .. 4 cells, gap runs around d_onep_d, the three encodings, mixed waves of 63 / 64 / 65
  B  tail classes through k_traceback_w (19-21 lines, 7-9 register rows, 1 / 2 / 4 bytes): runs of 31 .. 129 (the ballot's reach),
     window reloads inside an open gap run, the window clamped at column 0, unaligned byte rows
  C  the lane walk k_traceback (tiled extensions 18 / 23 / 24, class 0, classes 5 / 6): runs of 1 .. 5 from every row of a tile
  D  2,048 | 2,049 problems of one tail class in one pass: the switch from k_traceback_w to the lane walk (dp_pass: tbw_max)

usage: python tests/tb_paths_child.py   (one engine run of every group; tests/test_gpu_tb_paths.py runs it once per TELR_AB switch)
"""
import os
import sys
import zlib
from math import gcd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

import dp_edges as de
from telr_amd.aligner import Engine

SEEDS = 40
TBW_MAX = 2048              # telr_engine.hip, dp_pass: a tail class with more problems than this takes the lane walk
A_CLASSES = (17, 10, 11, 12, 13, 14, 15, 16, 22)
A_SETS = ("map-ont", "map-pb", "asm10", "ngmlr-ont")
AFFINE_SETS = ("map-ont", "map-pb", "asm10")
# band widths (diagonals) a fill must have to land in a class; with an N the packed fills take the register classes 5-9
D_RANGE = {17: (1, 16), 10: (17, 20), 11: (21, 24), 12: (25, 28), 13: (29, 32), 14: (33, 40), 15: (41, 48), 16: (49, 64), 22: (65, 128),
           19: (129, 256), 20: (257, 512), 21: (513, 1024), 5: (1, 64), 6: (65, 128), 7: (129, 256), 8: (257, 512), 9: (513, 1024)}
# ---- the geometry, restated (kernels.hip.h: DP_CLASS, d_tb4_rowb, and the offset formulas of the three walks) ----------------
ROW_BYTES = {17: 16, 10: 20, 11: 24, 12: 28, 13: 32, 14: 40, 15: 48, 16: 64, 22: 128, 19: 256, 20: 512, 21: 1024,
             5: 128, 6: 256, 7: 512, 8: 1024, 9: 2048, 18: 64, 23: 128, 24: 256}
NIBBLE_ROW_BYTES = {17: 8, 10: 12}
NIBBLE_BIT = {17: 1, 10: 2}
LANES = {17: 1, 10: 1, 11: 1, 12: 1, 13: 1, 14: 2, 15: 2, 16: 2, 22: 4}       # lanes per problem: a wave holds 64 / lanes problems
LINES, REGROWS, BYTES, TILES = "lines", "regrows", "bytes", "tiles"
LAYOUT = {**{c: LINES for c in (10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22)}, **{c: REGROWS for c in (5, 6, 7, 8, 9)},
          **{c: BYTES for c in (0, 1, 2, 3, 4)}, **{c: TILES for c in (18, 23, 24)}}
_OPC = {"M": 0, "I": 1, "D": 2}


def phase_period(rowb):
    """rows after which a row's place inside a 64-byte line repeats"""
    return 64 // gcd(rowb, 64)


def rows_off(i, j, dlo, rowb, nib):
    """d_traceback_rows: byte offset of cell (i, j) in the problem's trace-back piece"""
    a, sl = i + j, (j - i - dlo) >> 1
    if nib:
        return (a >> 1) * rowb + ((sl >> 2) << 2) + (((sl >> 1) & 1) << 1) + (sl & 1)
    return (a >> 1) * rowb + ((sl >> 1) << 2) + ((a & 1) << 1) + (sl & 1)


def w_rowcol(a, sl, layout):
    """k_traceback_w: row and byte column of a cell"""
    if layout == LINES:
        return a >> 1, ((sl >> 1) << 2) + ((a & 1) << 1) + (sl & 1)
    if layout == REGROWS:
        return a >> 2, (sl << 2) + (a & 3)
    return a, sl


def merged(spec):
    out = []
    for op, ln in spec:
        if ln <= 0:
            continue
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + ln)
        else:
            out.append((op, ln))
    return out


def cig_words(spec):
    return np.array([ln << 4 | _OPC[op] for op, ln in merged(spec)], np.uint32)


def dims(spec):
    return sum(l for o, l in spec if o != "D"), sum(l for o, l in spec if o != "I")


def ends(spec):
    """-> [(op, len, i, j)]: the cell each run ends at, start to end"""
    out, i, j = [], 0, 0
    for op, ln in merged(spec):
        i += ln if op != "D" else 0
        j += ln if op != "I" else 0
        out.append((op, ln, i, j))
    return out


def excursion(spec):
    ds = [0] + [j - i for _, _, i, j in ends(spec)]
    return min(ds), max(ds)


def inner_runs(spec):
    """diagonal runs between two gaps -> [(len, i, j of the run's top cell)]"""
    e = ends(spec)
    return [(e[k][1], e[k][2], e[k][3]) for k in range(1, len(e) - 1) if e[k][0] == "M"]


def rows_trips(spec, dlo, rowb, nib, run_ijl):
    """d_traceback_rows over one diagonal run (len, i, j): cells per trip, and whether a trip was cut by the wave's two lines"""
    ln, i, j = run_ijl
    trips, cut = [], False
    while ln > 0:
        room, mij, nn = rows_off(i, j, dlo, rowb, nib) & 63, min(i, j), 1
        while nn < 4 and nn < ln and mij > nn:
            if room < nn * rowb:
                cut = True
                break
            nn += 1
        trips.append(nn)
        i, j, ln = i - nn, j - nn, ln - nn
    return trips, cut


def gap_cost(mo, spec):
    """cost of the gap runs as the two-piece DP counts them: each run in its cheaper piece"""
    return sum(min(mo.q + mo.e * ln, mo.q2 + mo.e2 * ln) for op, ln in merged(spec) if op != "M")


def walk_w(spec, dlo, layout):
    """k_traceback_w restated over a realised path -> dict: trips (ballot runs), full (a run of 64 in one trip), cut32 (a trip of
    exactly 32 cut by the byte layout's reach), reloads, reload_in_gap (the window moved while a gap state was open), clamp (c0
    clamped to 0), edge (a run ended because i or j reached 0 inside the ballot)"""
    runs = [[op, ln] for op, ln in merged(spec)]
    i, j = dims(spec)
    ev = dict(trips=[], full=False, cut32=False, reloads=0, reload_in_gap=False, clamp=False, edge=False)
    r0, c0, open_gap = -1, 0, False
    while i > 0 and j > 0:
        op, rem = runs[-1]
        a, sl = i + j, (j - i - dlo) >> 1
        row, col = w_rowcol(a, sl, layout)
        k = r0 - row
        if r0 < 0 or k < 0 or k >= 64 or col < c0 or col >= c0 + 64:
            r0, c0 = row, max(col - 32, 0) & ~3
            ev["reloads"] += 1
            ev["reload_in_gap"] |= open_gap
            ev["clamp"] |= col - 32 < 0
        if op == "M":
            run = 0
            for x in range(64):
                if i - x <= 0 or j - x <= 0:
                    ev["edge"] = True
                    break
                if x >= rem:
                    break
                rk, ck = w_rowcol(a - 2 * x, sl, layout)
                if r0 - rk >= 64 or ck - c0 < 0 or ck - c0 >= 64:
                    ev["cut32"] |= layout == BYTES and x == 32
                    break
                run += 1
            assert run >= 1
            ev["full"] |= run == 64
            ev["trips"].append(run)
            i, j = i - run, j - run
            runs[-1][1] -= run
        else:
            i, j = (i - 1, j) if op == "I" else (i, j - 1)
            runs[-1][1] -= 1
            open_gap = runs[-1][1] > 0
        if runs[-1][1] == 0:
            runs.pop()
            open_gap = False
    return ev


def lane_trips(run_ijl):
    """d_traceback_lane, tiled: -> (kr of the run's top cell, cells per trip)"""
    ln, i, j = run_ijl
    kr0, trips = ((i + j) >> 1) & 3, []
    while ln > 0:
        kr, mij, nn = ((i + j) >> 1) & 3, min(i, j), 1
        while nn < 4 and nn < ln and kr >= nn and mij > nn:
            nn += 1
        trips.append(nn)
        i, j, ln = i - nn, j - nn, ln - nn
    return kr0, trips


def wave_cells(mo, lim, cls_steps):
    """d_pk_cell restated: [(cls, steps)] of one pass -> {cls: set of encodings its waves take} ("cx", "nibble", "onep", "tag8", "plain")"""
    out = {}
    onep = de.d_onep_d(mo.q, mo.e, mo.q2, mo.e2)
    for c in A_CLASSES:
        st = sorted((s for k, s in cls_steps if k == c), reverse=True)      # the class list: decreasing steps
        ppw = 64 // LANES[c]
        for w in range(0, len(st), ppw):
            if mo.cx_scale:
                enc = "cx"
            elif c in NIBBLE_BIT and onep >= de.UPPER_D[c]:
                enc = "nibble" if lim["tb4_mask"] & NIBBLE_BIT[c] else "onep"
            else:
                enc = "tag8" if st[w] <= lim["tag8_steps"] else "plain"
            out.setdefault(c, set()).add(enc)
    return out


# ---- planting -------------------------------------------------------------------------------------------------------------------
def plant(rng, spec, mism=0.04):
    """-> (A, B): query and target windows in DP order that have the path `spec`.  An M run is a copied stretch with a few
    substitutions, none within three bases of its ends; an I run is random bases on the query only, a D run on the target only
    (I runs draw from A / C and D runs from G / T: an inserted base never pairs with a deleted one, which is what lets a diagonal run
    of one or two cells between two gaps be the optimal path in a few seeds; and the copied base behind a gap run differs from the
    run's first base, the one in front of it from the run's last: the gap cannot slide without a loss)"""
    A, B = [], []
    runs = [rng.integers(0, 4, ln) if op == "M" else rng.integers(0, 2, ln) + (2 if op == "D" else 0) for op, ln in spec]
    for k, (op, ln) in enumerate(spec):
        if op != "M":
            continue
        ban = [{int(runs[k - 1][0])} if k > 0 else set(), {int(runs[k + 1][-1])} if k + 1 < len(spec) else set()]
        for pos, b in ((0, ban[0] | (ban[1] if ln == 1 else set())), (ln - 1, ban[1] | (ban[0] if ln == 1 else set()))):
            ok = [c for c in range(4) if c not in b]
            if int(runs[k][pos]) in b:
                runs[k][pos] = ok[int(rng.integers(0, len(ok)))]
    for (op, ln), s in zip(spec, runs):
        if op == "M":
            t = s.copy()
            hit = rng.random(ln) < mism
            hit[:3] = False
            hit[max(0, ln - 3):] = False
            t[hit] = (t[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
            A.append(s)
            B.append(t)
        elif op == "I":
            A.append(s)
        else:
            B.append(s)
    return de._ACGT[np.concatenate(A)].astype(np.uint8), de._ACGT[np.concatenate(B)].astype(np.uint8)


class Want:
    """a path to realise: kind 0 fills get the widest band of `cls`'s range that holds the path (narrow: the narrowest), extensions
    the scoring set's band; n_in: an N in the middle of the longest diagonal run of the query (the packed kernels have no N case)"""
    __slots__ = ("key", "fam", "what", "spec", "kind", "cls", "strand", "n_in", "drange", "narrow")

    def __init__(self, key, fam, what, spec, kind, cls, strand=0, n_in=False, drange=None, narrow=False):
        self.key, self.fam, self.what, self.spec, self.kind, self.cls = key, fam, what, merged(spec), kind, cls
        self.strand, self.n_in, self.drange, self.narrow = strand, n_in, drange or D_RANGE.get(cls), narrow


class Case:
    __slots__ = ("want", "seed", "prob", "score", "dlo")

    def __init__(self, want, seed, prob, score):
        self.want, self.seed, self.prob, self.score, self.dlo = want, seed, prob, score, prob.dlo


def band_of(mo, w):
    """-> (dlo, dhi) or None when no band of the class holds the path"""
    m, n = dims(w.spec)
    dmin, dmax = excursion(w.spec)
    if w.kind != 0:
        lo, hi = de.ext_band(mo)
        ok = lo <= dmin and dmax <= hi and m <= mo.ext_max and n <= m + mo.ext_band
        return (lo, hi) if ok else None
    dl, dh = w.drange
    Ws = range(0, dh + 1) if w.narrow else range(dh, -1, -1)
    for W in Ws:
        lo, hi = de.fill_band(m, n, W)
        if dl <= hi - lo + 1 <= dh and lo <= dmin and dmax <= hi:
            return lo, hi
    return None


def make(mo, w, seed):
    rng = np.random.default_rng([zlib.crc32(w.key.encode()), seed])
    A, B = plant(rng, w.spec)
    if w.n_in:
        i0, best = 0, (0, 0)
        for op, ln in w.spec:
            if op == "M" and ln > best[0]:
                best = (ln, i0)
            i0 += ln if op != "D" else 0
        A[best[1] + best[0] // 2] = ord("N")
    lo, hi = band_of(mo, w)
    return de.Prob(w.kind, len(A), len(B), lo, hi, w.strand, A, B, None, "%s:%s" % (w.fam, w.what))


def realise(mo, lim, wants):
    """-> (cases, dropped wants, wants no band of their class holds)"""
    fit = [w for w in wants if band_of(mo, w) is not None]
    narrow = [w for w in wants if band_of(mo, w) is None]
    got, pend = {}, list(range(len(fit)))
    for seed in range(SEEDS):
        if not pend:
            break
        probs = [make(mo, fit[k], seed) for k in pend]
        qs, ts, rows = de.materialize(np.random.default_rng(seed), probs)
        ref = de.oracle_dp(qs, ts, mo, rows)
        nxt = []
        for x, k in enumerate(pend):
            w, p = fit[k], probs[x]
            if np.array_equal(ref["cigars"][x], cig_words(w.spec)):
                has_n = bool((p.A == ord("N")).any())
                c = de.expect_class(p.kind, p.dhi - p.dlo + 1, p.m + p.n, lim, has_n)
                assert c == w.cls, "%s: routing says class %d, aimed at %d" % (w.key, c, w.cls)
                got[k] = Case(w, seed, p, int(ref["score"][x]))
            else:
                nxt.append(k)
        pend = nxt
    return [got[k] for k in sorted(got)], [fit[k] for k in pend], narrow


def allowed_drop(set_name, w):
    """the allow list: under the two ngmlr-* sets a diagonal run of at most 3 cells next to a gap is not the optimal path"""
    return set_name.startswith("ngmlr") and any(op == "M" and ln <= 3 for op, ln in w.spec)


# ---- the specs ------------------------------------------------------------------------------------------------------------------
def two_gap(run, order, lead, tail, g1=3, g2=2):
    return [("M", lead), (order[0], g1), ("M", run), (order[1], g2), ("M", tail)]


def sets():
    s = {n: de._mo(n) for n in A_SETS}
    # extension bands of 128 / 132 / 256 diagonals: byte rows of 65 / 67 / 129 bytes (classes 1, 2, 2 with an N; 23 / 24 without)
    for eb in (63, 65, 127):
        s["ext%d" % eb] = de._mo("map-ont", ext_band=eb, bw_long=0, zdrop=400)
    return s


def wants_a(name, mo):
    out = []
    onep = de.d_onep_d(mo.q, mo.e, mo.q2, mo.e2)
    for c in A_CLASSES:
        def W(what, spec):
            out.append(Want("A/%s/%d/%s" % (name, c, what), "A", what, spec, 0, c, strand=len(out) & 1))
        for run in (1, 2, 3, 4, 5, 8, 9):
            for order in ("ID", "DI"):
                for t in range(16):         # rows count from the path's start: the leading run moves the run's top cell over the row phases
                    W("run%d%s+%d" % (run, order, t), two_gap(run, order, 40 + t, 20 + t))
        for lead in (0, 1, 2, 3, 4):
            for op in "ID":
                W("lead%d%s" % (lead, op), [("M", lead), (op, 3), ("M", 60)])
        if name in AFFINE_SETS:
            for g in (onep - 1, onep, onep + 1, 2 * onep):
                for op in "ID":
                    W("gap%d%s" % (g, op), [("M", 40), (op, g), ("M", 60)])
                    W("gap%d%s first" % (g, op), [(op, g), ("M", 60)])
        # the long path of the mixed waves
        W("long", [("M", 80), ("I", 3), ("M", 4), ("D", 2), ("M", 80), ("D", 3), ("M", 3), ("I", 2), ("M", 10)])
    return out


B_RUNS = (31, 32, 33, 63, 64, 65, 127, 128, 129)
B_GAPS = {REGROWS: (17, 40), LINES: (70, 130), BYTES: (70, 130)}


def wants_b(name, mo, targets):
    """targets: [(cls, kind, n_in, drange or None)]"""
    out = []
    for c, kind, n_in, drange in targets:
        lay = LAYOUT[c]
        def W(what, spec, narrow=False):
            out.append(Want("B/%s/%d/%d/%s" % (name, c, kind, what), "B", what, spec, kind, c, strand=len(out) & 1, n_in=n_in, drange=drange, narrow=narrow))
        for run in B_RUNS:
            for order in ("ID", "DI"):
                W("run%d%s" % (run, order), two_gap(run, order, 40, 30))
        for g in B_GAPS[lay]:
            for op in "ID":
                W("gap%d%s" % (g, op), [("M", 100), (op, g), ("M", 100)])
        # along the band's low edge: an insertion that takes nearly the whole band
        lo = -de.ext_band(mo)[0] - 2 if kind else (drange or D_RANGE[c])[0] - 3
        W("lowedge", [("M", 40), ("I", lo), ("M", 110)], narrow=True)
    return out


def wants_c(name, mo, targets):
    out = []
    for c, kind, n_in in targets:
        def W(what, spec):
            out.append(Want("C/%s/%d/%d/%s" % (name, c, kind, what), "C", what, spec, kind, c, strand=len(out) & 1, n_in=n_in))
        for run in (1, 2, 3, 4, 5):
            for order in ("ID", "DI"):
                for t in range(8):
                    W("run%d%s+%d" % (run, order, t), two_gap(run, order, 40 + t, 20 + t))
        for op in "ID":
            W("gap20%s" % op, [("M", 40), (op, 20), ("M", 60)])
    return out


def wants_d(name, c, kind, n_in):
    out = []
    for t in range(8):
        for run, order in ((5, "ID"), (33, "DI")):
            out.append(Want("D/%s/%d/run%d%s+%d" % (name, c, run, order, t), "D", "run%d%s+%d" % (run, order, t),
                            two_gap(run, order, 30 + t, 50 - (run >> 1)), kind, c, strand=t & 1, n_in=n_in))
    return out


class Group:
    """one DP pass"""
    __slots__ = ("set", "fam", "name", "cases", "front", "enc")

    def __init__(self, set_name, fam, name, cases, front=(), enc=None):
        self.set, self.fam, self.name, self.cases, self.front, self.enc = set_name, fam, name, list(cases), list(front), enc

    def probs(self):
        return self.front + [c.prob for c in self.cases]


class Built:
    def __init__(self):
        self.sets = sets()
        self.lims = {n: Engine.dp_limits(mo) for n, mo in self.sets.items()}
        self.groups, self.dropped, self.narrow, self.cases = [], [], [], []

    def take(self, name, wants):
        cases, dropped, narrow = realise(self.sets[name], self.lims[name], wants)
        self.dropped += [(name, w) for w in dropped]
        self.narrow += [(name, w) for w in narrow]
        self.cases += [(name, c) for c in cases]
        return cases


_BUILT = None


def build():
    global _BUILT
    if _BUILT is not None:
        return _BUILT
    b = Built()
    G = b.groups
    # ---- A
    for name in A_SETS:
        mo, lim = b.sets[name], b.lims[name]
        cases = b.take(name, wants_a(name, mo))
        longs = {}
        for c in A_CLASSES:
            mine = [x for x in cases if x.want.cls == c and x.want.what != "long"]
            longs[c] = [x for x in cases if x.want.cls == c and x.want.what == "long"]
            G.append(Group(name, "A", "class %d" % c, mine))
            # plain flags: one long plain problem in front decides the cell of its wave (d_pk_cell); the wave's other problems are planted
            if not mo.cx_scale and c not in NIBBLE_BIT and lim["tag8_steps"] and lim["tag8_steps"] + 1 <= lim["pk_steps_limit"]:
                ppw = 64 // LANES[c]
                pick = mine[::max(1, len(mine) // (ppw - 1))][:ppw - 1]
                front = de.fill_steps(np.random.default_rng(c), de.UPPER_D[c], lim["tag8_steps"] + 1, "err", 0, tag="A:front")
                G.append(Group(name, "A", "class %d plain" % c, pick, [front], enc="plain"))
        for cnt in (63, 64, 65):
            ps = []
            for c in A_CLASSES:
                mine = [x for x in cases if x.want.cls == c and x.want.what != "long"]
                ps += longs[c] + mine[3::max(1, len(mine) // cnt)][:cnt - len(longs[c])]
            G.append(Group(name, "A", "waves of %d" % cnt, ps))
    # ---- B
    mo = b.sets["map-ont"]
    tb = [(c, 0, False, None) for c in (19, 20, 21)] + [(c, 0, True, None) for c in (7, 8, 9)] + [(4, 0, False, (1026, 1026)), (4, 0, False, (1028, 1028))]
    G.append(Group("map-ont", "B", "fills", b.take("map-ont", wants_b("map-ont", mo, tb))))
    for name, c in (("ext63", 1), ("ext65", 2), ("ext127", 2)):
        G.append(Group(name, "B", "extensions", b.take(name, wants_b(name, b.sets[name], [(c, 1, True, None), (c, 2, True, None)]))))
    # ---- C
    tc = [(18, 1, False), (18, 2, False), (0, 1, True), (0, 2, True), (5, 0, True), (6, 0, True)]
    G.append(Group("map-ont", "C", "lane walk", b.take("map-ont", wants_c("map-ont", mo, tc))))
    for name, c in (("ngmlr-ont", 23), ("ext63", 23), ("ext127", 24)):
        G.append(Group(name, "C", "tiled", b.take(name, wants_c(name, b.sets[name], [(c, 1, False), (c, 2, False)]))))
    # ---- D
    for name, c, kind, n_in in (("map-ont", 19, 0, False), ("map-ont", 7, 0, True), ("ext63", 1, 1, True)):
        cases = b.take(name, wants_d(name, c, kind, n_in))
        assert cases, "family D: nothing realised for class %d" % c
        many = [cases[x % len(cases)] for x in range(TBW_MAX + 1)]
        G.append(Group(name, "D", "%d of class %d" % (TBW_MAX, c), many[:TBW_MAX]))
        G.append(Group(name, "D", "%d of class %d" % (TBW_MAX + 1, c), many))
    _BUILT = b
    return b


# ---- the engine run ---------------------------------------------------------------------------------------------------------------
def run_all(eng, fams="ABCD"):
    """-> {family: (problem count, mismatches, [(set, group, cls, D, steps, tag)])}"""
    b = build()
    out = {f: [0, [], []] for f in fams}
    rng = np.random.default_rng(4242)
    for g in b.groups:
        if g.fam not in fams:
            continue
        probs = g.probs()
        if not probs:
            continue
        bad, seen = de.run_group(eng, b.sets[g.set], b.lims[g.set], probs, rng, "%s / %s %s" % (g.set, g.fam, g.name))
        r = out[g.fam]
        r[0] += len(probs)
        r[1] += bad
        r[2] += [(g.set, g.name) + s for s in seen]
    return {f: tuple(v) for f, v in out.items()}


def summary(res):
    lines = []
    for f, (n, bad, cov) in sorted(res.items()):
        per = {}
        for s, _, c, _, _, _ in cov:
            per.setdefault(s, []).append(c)
        lines.append("family %s: %6d problems; %s" % (f, n, "; ".join("%s %d, classes %s" % (s, len(c), " ".join(map(str, sorted(set(c))))) for s, c in sorted(per.items()))))
    return lines
