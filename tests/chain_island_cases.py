"""Sorted anchor lists aimed at the island walk of k_chain (kernels.hip.h: THE ISLAND WALK, d_chain_walk): the wave of a query takes
its list by windows of 64 anchors, chains the whole small islands of a window side by side (one island's t-th anchor pushed to its
own later lanes in sub-step t) and hands an island that does not fit a window to the loops for whole runs.  tests/chain_edges.py
aims at those loops; the lists here aim at where windows and islands begin and end.

A case is a dict as in tests/chain_edges.py (name, lists, mo, reach) with two claims more, which the CPU test of
tests/test_gpu_chain_islands.py checks with numpy on the keys themselves, so that a slip in a generator cannot quietly leave only
the serial loop under test:
  sizes   per list, the island sizes in order (an island head: the first anchor, and every anchor whose reference word -- strand in
          bit 31 -- lies more than max_gap beyond its predecessor's)
  walk    per list, the steps the wave takes: ("packed", pos, e) -- a window at pos whose first e anchors are whole islands -- and
          ("serial", pos, n) -- an island of n anchors from pos for the loops for whole runs; written out by hand per case and
          held against `walk_of`, the window rule restated on the sizes.
Every case is built for the look-backs 64, 128 and 256 and for chain_skip_q8 0 and 3 (chain_edges.SETTINGS), max_gap 5000, bw 500.

Run as a program this file is one process of the GPU tests (the engine reads TELR_AB and TELR_CHAIN_DENSE once per process):
  python tests/chain_island_cases.py                every case through telr_debug_chain against the oracle's tap, exactly
  python tests/chain_island_cases.py --map OUT.npz  the bundled 38-kb fixture mapped under map-ont and ngmlr-ont, records and CIGARs saved"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import chain_edges as E  # noqa: E402
from chain_edges import key, tie_list, link_score, lattice, G0, Q0  # noqa: E402

WINDOW = 64
MAX_GAP = 5000


# ---------------------------------------------------------------------------------------------------------------------
# the claims


def sizes_of(L, max_gap=MAX_GAP):
    """island sizes of one sorted list, from the keys alone"""
    if len(L) == 0:
        return []
    w = (np.asarray(L, np.uint64) >> np.uint64(32)).astype(np.int64)
    heads = np.concatenate(([0], 1 + np.flatnonzero(np.diff(w) > max_gap), [len(w)]))
    return [int(x) for x in np.diff(heads)]


def walk_of(sizes):
    """the window rule on a list's island sizes: at pos (an island head) the window holds anchors pos .. pos + 63; where the list ends
    inside it, all that is left is packed; otherwise everything before the last head among lanes 1 .. 63; without such a head the
    island at pos goes to the serial loops whole"""
    starts = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    n, pos, out = int(starts[-1]), 0, []
    while pos < n:
        assert pos in starts
        if n - pos <= WINDOW:
            e = n - pos
        else:
            hs = starts[(starts > pos) & (starts <= pos + WINDOW - 1)]
            if len(hs) == 0:
                end = int(starts[starts > pos].min())
                out.append(("serial", pos, end - pos))
                pos = end
                continue
            e = int(hs.max()) - pos
        out.append(("packed", pos, e))
        pos += e
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the generators


def islands(sizes, seed, g0=20000, rev_from=None, gap=MAX_GAP + 1):
    """one list of islands of these sizes, `gap` reference bases between the last anchor of one and the head of the next.  Inside an
    island the anchors step 1 .. 40 bases along the reference and -20 .. 60 along the query (seeded): links with and without a
    penalty, refused links, predecessors that are not the neighbour.  rev_from: the islands from that one on are on the reverse
    strand (coordinates start again)"""
    rng = np.random.RandomState(seed)
    L, g = [], g0
    for k, s in enumerate(sizes):
        rev = int(rev_from is not None and k >= rev_from)
        if rev_from is not None and k == rev_from:
            g = g0
        q = 3000 + int(rng.randint(0, 2000))
        for i in range(s):
            if i:
                g += int(rng.randint(1, 41))
                q += int(rng.randint(-20, 61))
            L.append(key(g, q, int(rng.choice((15, 15, 15, 9, 21))), rev=rev))
        g += gap
    return L


def make(name, lists, mo, sizes, walk, reach=None):
    c = E.make(name, lists, mo, reach or (lambda F, P: None))
    c["sizes"], c["walk"] = sizes, walk
    return c


def P_(pos, e):
    return ("packed", pos, e)


def S_(pos, n):
    return ("serial", pos, n)


# (name, island sizes of the one list, the walk) -- the walks are written by hand
SHAPES = [
    # islands of 1, 2, 16 and 17 anchors in one window that the list ends in
    ("sizes_1_2_16_17", [1, 2, 16, 17, 1], [P_(0, 37)]),
    # 63: the largest island that is packed where the list goes on -- the next head sits in lane 63
    ("size_63_head_at_lane_63", [63, 5], [P_(0, 63), P_(63, 5)]),
    ("singletons_head_at_lane_63", [1] * 63 + [3], [P_(0, 63), P_(63, 3)]),
    # 64: fills a window; packed where the list ends with it (63 sub-steps), serial where the list goes on
    ("size_64_list_ends_at_lane_64", [64], [P_(0, 64)]),
    ("size_64_then_list_ends_at_lane_1", [64, 1], [S_(0, 64), P_(64, 1)]),
    ("size_65_then_list_ends_at_lane_1", [65, 1], [S_(0, 65), P_(65, 1)]),
    ("size_65_alone", [65], [S_(0, 65)]),
    # a window of 64 singletons (no sub-step at all), and windows of singletons one after the other
    ("singletons_64", [1] * 64, [P_(0, 64)]),
    ("singletons_200", [1] * 200, [P_(0, 63), P_(63, 63), P_(126, 63), P_(189, 11)]),
    # the list ends at lane 63 and at lane 64 of its last window
    ("list_ends_at_lane_63", [5, 63], [P_(0, 5), P_(5, 63)]),
    ("list_ends_at_lane_64", [5, 64], [P_(0, 5), P_(5, 64)]),
    ("list_ends_at_lane_63_after_serial", [70, 63], [S_(0, 70), P_(70, 63)]),
    # an island across a window boundary: below 64 anchors it heads the next window, above it is serial
    ("straddle_below_64", [40, 40, 3], [P_(0, 40), P_(40, 43)]),
    ("straddle_63", [10, 63, 63, 2], [P_(0, 10), P_(10, 63), P_(73, 63), P_(136, 2)]),
    ("straddle_above_64", [40, 70, 3], [P_(0, 40), S_(40, 70), P_(110, 3)]),
    # packed windows directly before and directly after a serial island, twice over (no state may leak either way)
    ("packed_serial_packed", [3, 2, 100, 4, 1], [P_(0, 5), S_(5, 100), P_(105, 5)]),
    ("serial_packed_serial", [130, 2, 17, 1, 90, 66, 7], [S_(0, 130), P_(130, 20), S_(150, 90), S_(240, 66), P_(306, 7)]),
]


def cases_shapes(H, skip, tag):
    out = []
    for k, (name, sizes, walk) in enumerate(SHAPES):
        out.append(make(name + tag, [islands(sizes, 100 + k)], E.opts(H, skip), [sizes], [walk]))
    # the same on both strands: the strand change is a head like any other
    sizes = [1, 30, 2, 1, 1, 33, 4, 80, 1]
    out.append(make("two_strands" + tag, [islands(sizes, 7, rev_from=4)], E.opts(H, skip), [sizes], [[P_(0, 35), P_(35, 37), S_(72, 80), P_(152, 1)]]))
    return out


def case_breaks(H, skip, tag):
    """consecutive anchors exactly max_gap apart stay one island (and link), max_gap + 1 apart they do not"""
    mo = E.opts(H, skip)
    mg = mo.max_gap
    pts = [(G0 + 10 * i, Q0 + 10 * i) for i in range(5)]

    def add(dg, dq, n=1):
        for _ in range(n):
            pts.append((pts[-1][0] + dg, pts[-1][1] + dq))
    add(mg, mg - 400)           # 5: max_gap on, linked to 4
    add(10, 10, 4)              # 6 .. 9
    add(mg + 1, mg - 400)       # 10: a head
    add(10, 10, 4)              # 11 .. 14
    L = [key(g, q) for g, q in pts]

    def reach(F, P):
        w = np.diff((np.asarray(L, np.uint64) >> np.uint64(32)).astype(np.int64))
        assert w[4] == mg and w[9] == mg + 1
        assert P[0][5] == 4 and P[0][10] == -1 and F[0][10] == 15 and P[0][11] == 10
    return make("break_at_max_gap_plus_1" + tag, [L], mo, [[10, 5]], [[P_(0, 15)]], reach)


def case_strand_adjacent(H, skip, tag):
    """a strand change between adjacent positions: the reverse anchors continue the forward chain's coordinates one base on, and
    only bit 31 of the reference word makes the head"""
    mo = E.opts(H, skip)
    L = [key(G0 + 10 * i, Q0 + 10 * i) for i in range(20)] + [key(G0 + 191 + 10 * i, Q0 + 191 + 10 * i, rev=1) for i in range(20)]

    def reach(F, P):
        assert ((int(L[20]) >> 32) & 0x7fffffff) - ((int(L[19]) >> 32) & 0x7fffffff) == 1
        want = np.arange(-1, 39)
        want[20] = -1
        assert np.array_equal(P[0], want) and F[0][20] == 15
    return make("break_at_strand_change" + tag, [L], mo, [[20, 20]], [[P_(0, 40)]], reach)


def cases_tie(H, skip, tag):
    """equal-score predecessors inside a packed island (chain_edges.tie_list: X and Y give T the same score and cannot link to each
    other): pushes reach a lane in ascending order and `>=` keeps the larger index, Y.  Singleton islands in front shift the island's
    lanes; `late`: the island starts at lane 20 of the list's second window"""
    mo = E.opts(H, skip)
    X, Y, T = key(G0, Q0 + 20), key(G0 + 20, Q0), key(G0 + 120, Q0 + 120)
    out = []
    for what, lead, t, xi, yi in (("", 5, 40, 20, 30), ("_adjacent", 1, 12, 10, 11), ("_late", 83, 50, 3, 48)):
        # singletons in front and behind; the island's coordinates are moved up past the front ones (a link sees differences only)
        front = [key(20 + (MAX_GAP + 1) * i, 500 + i) for i in range(lead)]
        shift = (MAX_GAP + 1) * (lead + 2)
        isl = [k + (shift << 32) for k in tie_list(t, xi, yi, X, Y, T)]
        top = (int(isl[-1]) >> 32) & 0x7fffffff
        back = [key(top + (MAX_GAP + 1) * (i + 1), 700 + i) for i in range(3)]
        L = front + isl + back
        sizes = [1] * lead + [t + 1] + [1] * 3
        if lead == 83:
            walk = [P_(0, 63), P_(63, 20), P_(83, 54)]
        else:
            walk = [P_(0, len(L))]

        def reach(F, P, lead=lead, t=t, xi=xi, yi=yi):
            assert link_score(T, X, mo) == link_score(T, Y, mo)
            assert F[0][lead + xi] == F[0][lead + yi] == 15 and P[0][lead + xi] == P[0][lead + yi] == -1
            assert P[0][lead + t] == lead + yi and F[0][lead + t] == 15 + link_score(T, Y, mo)
        out.append(make("tie_in_packed_island" + what + tag, [L], mo, [sizes], [walk], reach))
    return out


def case_dense_serial(H, skip, tag):
    """a lattice of repeat copies (chain_edges.lattice: every link lies more than 64 back) as the serial island between two packed
    windows: under small thresholds of TELR_CHAIN_DENSE the run is sampled by itself and takes the push loop"""
    lat = [k + (60000 << 32) for k in lattice(200)]
    front = [key(20 + (MAX_GAP + 1) * i, 500 + i) for i in range(6)]
    top = (int(lat[-1]) >> 32) & 0x7fffffff
    back = islands([1, 4, 1], 5, g0=top + MAX_GAP + 1)
    L = front + lat + back

    def reach(F, P):
        p = P[0][6:206]
        behind = (np.arange(6, 206) - p)[p >= 0]
        if H >= 128:
            assert len(behind) > 100 and behind.min() > 64 and p[p >= 0].min() >= 6
        else:
            assert len(behind) == 0
    return make("dense_serial_island" + tag, [L], E.opts(H, skip), [[1] * 6 + [200, 1, 4, 1]], [[P_(0, 6), S_(6, 200), P_(206, 6)]], reach)


def case_queries(H, skip, tag):
    """three queries of one call, an empty one and one of a single anchor among them: a query is found only through q_aoff"""
    a = islands([2, 1, 70, 9], 31)
    lists = [[], a, [key(G0, Q0)]]
    return make("empty_and_single_anchor" + tag, lists, E.opts(H, skip), [[], [2, 1, 70, 9], [1]], [[], [P_(0, 3), S_(3, 70), P_(73, 9)], [P_(0, 1)]])


def case_random(H, skip, tag):
    """island sizes drawn like a read's (mostly singletons, a few chains), three queries of about 400 anchors"""
    rng = np.random.RandomState(1234)
    lists, sizes = [], []
    for q in range(3):
        s = []
        while sum(s) < 380:
            r = rng.rand()
            k = 1 if r < 0.55 else int(rng.randint(2, 5)) if r < 0.7 else int(rng.randint(5, 17)) if r < 0.85 else int(rng.randint(17, 65)) if r < 0.95 else int(rng.randint(65, 140))
            if sum(s) + k <= 400:
                s.append(k)
        sizes.append(s)
        lists.append(islands(s, 900 + q, rev_from=len(s) // 2))
    return make("random_islands" + tag, lists, E.opts(H, skip), sizes, [walk_of(s) for s in sizes])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for H, skip in E.SETTINGS:
        tag = "_h%d_s%d" % (H, skip)
        out += cases_shapes(H, skip, tag)
        out += [case_breaks(H, skip, tag), case_strand_adjacent(H, skip, tag)]
        out += cases_tie(H, skip, tag)
        out += [case_dense_serial(H, skip, tag), case_queries(H, skip, tag), case_random(H, skip, tag)]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# one process of the GPU tests


def child_cases():
    import torch  # noqa: F401  (its HIP runtime first, as in tests/conftest.py)
    from telr_amd.aligner import Engine
    eng = Engine(0)
    bad, n = [], 0
    for case in cases():
        ef, ep = E.oracle_out(case)
        keys, off = E.call_input(case)
        pk, s = E.poison_input(case, off)
        f, p = eng.debug_chain(pk, off, case["mo"])
        if not (np.all(f == s) and np.all(p == -1)):
            bad.append("%s: the poisoning call" % case["name"])
        f, p = eng.debug_chain(keys, off, case["mo"])
        n += 1
        if not (f.dtype == ef.dtype and p.dtype == ep.dtype and np.array_equal(f, ef) and np.array_equal(p, ep)):
            w = np.flatnonzero((f != ef) | (p != ep))
            bad.append("%s: %d anchors differ, the first at %d: f %d p %d, oracle f %d p %d"
                       % (case["name"], len(w), w[0], f[w[0]], p[w[0]], ef[w[0]], ep[w[0]]))
    if bad:
        print("\n".join(bad))
        print("chain islands child: %d of %d calls differ" % (len(bad), n))
        sys.exit(3)
    print("chain islands child ok (%d calls)" % n)


def child_map(out):
    import torch  # noqa: F401
    from telr_amd.aligner import Engine
    from telr_amd.fasta import read_fasta
    from telr_amd.presets import preset
    d = os.path.join(HERE, "data")
    _, ts = read_fasta(os.path.join(d, "ref_38kb.fasta"))
    _, qs = read_fasta(os.path.join(d, "reads.fasta"))
    eng = Engine(0)
    res = {}
    for pname in ("map-ont", "ngmlr-ont"):
        io, mo = preset(pname)
        r = eng.index(ts, io).map(qs, mo)
        res[pname + "_alns"] = np.asarray(r.alns)
        res[pname + "_cigars"] = np.asarray(r.cigars)
    np.savez(out, **res)
    print("chain islands map ok (%d + %d records)" % (len(res["map-ont_alns"]), len(res["ngmlr-ont_alns"])))


if __name__ == "__main__":
    if "--map" in sys.argv[1:]:
        child_map(sys.argv[sys.argv.index("--map") + 1])
    else:
        child_cases()
