"""Hand-built records and intervals for telr_depth_medians, one case per edge of k_depth_diff / k_depth_median, with the medians worked
out by hand (tests/test_depth_ref.py holds tests/depth_ref.py and the oracle to them; tests/test_gpu_depth_edges.py holds the engine
to both), and the malformed results the entry refuses.  Targets of a few hundred bases: every case is tiny."""
import numpy as np

import inscall_cases as ic

NAN = None                                   # in `want`: an empty interval
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SEC = 2                                      # TELR_F_SECONDARY


def M(n):
    return (n, "M")


def I(n):
    return (n, "I")


def D(n):
    return (n, "D")


def R(tid, ts, cig, flags=0, te=None, qid=0):
    """a record whose coordinates follow from its CIGAR (te: a lie about the end)"""
    ql = sum(n for n, o in cig if o in "MI")
    rl = sum(n for n, o in cig if o in "MD")
    return ic.rec(qid, ql, 0, ql, ts, ts + rl if te is None else te, cig, tid=tid, flags=flags)


def case(name, tlens, recs, iv, want):
    assert len(iv) == len(want)
    return dict(name=name, tlens=list(tlens), recs=recs, iv=iv, want=want)


def arrays(c):
    """-> (alns, cigars, tlens, iv_tid, iv_s, iv_e) of a case"""
    alns, cig = ic.pack(c["recs"])
    iv = np.array(c["iv"], np.int64).reshape(-1, 3)
    return alns, cig, np.array(c["tlens"], np.int32), iv[:, 0].astype(np.int32), iv[:, 1].astype(np.int32), iv[:, 2].astype(np.int32)


def want_array(c):
    return np.array([np.nan if w is None else w for w in c["want"]], np.float64)


def staircase(tid=0, at=10, steps=300):
    """depth(at + j) = j + 1 for j < steps, 0 from at + steps on"""
    return [R(tid, at + j, [M(steps - j)]) for j in range(steps)]


def cases():
    C = []
    # ---- the cap: positions 10 .. 13 covered by 7,999, 8,000, 8,001 and 20,000 one-op records
    recs = [R(0, 10, [M(4)])] * 7999 + [R(0, 11, [M(3)]), R(0, 12, [M(2)])] + [R(0, 13, [M(1)])] * 11999
    C.append(case("cap", [300], recs, [(0, 10, 10), (0, 11, 11), (0, 12, 12), (0, 13, 13), (0, 10, 11), (0, 12, 13), (0, 9, 9), (0, 11, 13), (0, 13, 14)],
                  [7999, 8000, 8000, 8000, 7999.5, 8000, 0, 8000, 4000]))
    # ---- order statistics: depths 1 2 3 4 at 20 .. 23 and 3 1 4 2 at 30 .. 33; the even intervals give the mean of the two middle values
    recs = [R(0, 20 + j, [M(4 - j)]) for j in range(4)] + [R(0, 30, [M(1)])] * 3 + [R(0, 31, [M(1)])] + [R(0, 32, [M(1)])] * 4 + [R(0, 33, [M(1)])] * 2
    C.append(case("order_statistics", [100], recs,
                  [(0, 20, 20), (0, 20, 21), (0, 20, 22), (0, 20, 23), (0, 21, 23), (0, 30, 33), (0, 30, 32), (0, 31, 32), (0, 30, 31), (0, 32, 33), (0, 23, 24)],
                  [1, 1.5, 2, 2.5, 3, 2.5, 3, 2.5, 2, 3, 2]))
    # ---- interval lengths around the 256 threads of k_depth_median, over depth(p) = p - 9 on [10, 310)
    C.append(case("interval_lengths", [600], staircase(),
                  [(0, 10, 264), (0, 10, 265), (0, 10, 266), (0, 11, 266), (0, 10, 521), (0, 10, 522), (0, 309, 310), (0, 310, 599)],
                  [128, 128.5, 129, 129.5, 44.5, 44, 150, 0]))        # 10 .. 521: 212 zeros below the 300 steps = 512 positions, the middle two 44 and 45
    # ---- the clamps of s and e, and the empty interval.  Depth 1 on [0, 40), 2 on [40, 50)
    recs = [R(0, 0, [M(50)]), R(0, 40, [M(10)])]
    C.append(case("clamps", [50], recs,
                  [(0, -5, 3), (0, 38, 60), (0, -100, 100), (0, 48, 49), (0, 39, 40), (0, 49, 49), (0, 49, I32_MAX), (0, I32_MIN, 0),
                   (0, 50, 60), (0, 10, 9), (0, 30, 5), (0, -10, -1), (0, I32_MIN, I32_MAX), (0, I32_MAX, I32_MIN), (0, I32_MAX, I32_MAX), (0, I32_MIN, I32_MIN),
                   (0, 50, 49), (0, 0, -1), (0, 0, 0)],
                  [1, 2, 1, 2, 1.5, 2, 2, 1,
                   NAN, NAN, NAN, NAN, 1, NAN, NAN, NAN,
                   NAN, NAN, 1]))
    # ---- the ops
    recs = [R(0, 10, [M(5), I(3), D(4), M(6)]),            # M [10, 15), D [15, 19), M [19, 25)
            R(0, 30, [I(2), M(5)]),                        # starts with I: M [30, 35)
            R(0, 40, [M(5), D(3)]),                        # ends with D: M [40, 45), te = 48
            R(0, 50, [M(3), M(4)]),                        # two adjacent M ops: [50, 57)
            R(0, 60, [M(2), M(0), M(2)]),                  # a 0M op: [60, 64)
            R(0, 70, []),                                  # no op
            R(0, 100, [M(1), D(1)] * 32 + [M(1)]),         # 65 ops: M at 100, 102, .. 164
            R(0, 180, [D(0), I(0), M(3), I(0), D(0)])]     # zero-length I and D: [180, 183)
    C.append(case("ops", [200], recs,
                  [(0, 10, 14), (0, 15, 18), (0, 19, 24), (0, 10, 24), (0, 14, 15), (0, 29, 35), (0, 40, 47), (0, 45, 47), (0, 50, 56), (0, 57, 57),
                   (0, 60, 63), (0, 62, 62), (0, 64, 64), (0, 70, 70), (0, 100, 164), (0, 100, 163), (0, 101, 101), (0, 164, 165), (0, 179, 183), (0, 180, 182)],
                  [1, 0, 1, 1, 0.5, 1, 1, 0, 1, 0,
                   1, 1, 0, 0, 1, 0.5, 0, 0.5, 1, 1]))
    # ---- the ends of a target.  Target 0 is covered to its last base by three records (their -1 goes into the slot between the targets),
    # target 1 starts uncovered, target 2 has one base, target 3 no record
    recs = [R(0, 0, [M(10)])] + [R(0, 30, [M(10)])] * 3 + [R(1, 5, [M(10)])] + [R(2, 0, [M(1)])] * 2
    C.append(case("ends", [40, 30, 1, 20], recs,
                  [(0, 0, 0), (0, 9, 10), (0, 39, 39), (0, 29, 30), (0, 30, 100), (1, 0, 0), (1, 0, 4), (1, 4, 5), (1, 14, 15), (1, -3, 40),
                   (2, 0, 0), (2, -1, 5), (2, 1, 1), (3, 0, 19), (3, 19, 19), (3, 20, 20)],
                  [1, 0.5, 3, 1.5, 3, 0, 0, 0.5, 0.5, 0,
                   2, 2, NAN, 0, 0, NAN]))
    # ---- flags: only TELR_F_SECONDARY takes a record out; a secondary record may even leave its target
    recs = [R(0, 10, [M(10)], flags=f) for f in range(16)] + [R(0, 10, [M(10)], flags=f) for f in (0x10, 0x20, 0x100, 0x102, 0x7ffffffd)] + [R(0, 45, [M(10)], flags=SEC)]
    C.append(case("flags", [50], recs, [(0, 10, 19), (0, 9, 10), (0, 45, 49)], [12, 6, 0]))
    C.append(case("all_secondary", [50], [R(0, 10, [M(10)], flags=SEC), R(0, 12, [M(3)], flags=SEC | 8)], [(0, 10, 19), (0, 0, 49)], [0, 0]))
    C.append(case("no_records", [50, 7], [], [(0, 0, 49), (1, 6, 6), (1, 7, 7)], [0, 0, NAN]))
    # ---- counts around the 64 threads of k_depth_diff: record i covers [i, i + 2)
    for n in (63, 64, 65):
        C.append(case("records_%d" % n, [100], [R(0, i, [M(2)]) for i in range(n)], [(0, 0, 0), (0, 1, n - 1), (0, n, n), (0, n - 1, n), (0, n + 1, 99), (0, 0, 1)],
                      [1, 2, 1, 1.5, 0, 1.5]))
    # ---- interval counts: none, one, 300 unordered ones with duplicates over depth(p) = p - 9 on [10, 310): median(s .. e) = (s + e) / 2 - 9
    C.append(case("intervals_0", [600], staircase(), [], []))
    C.append(case("intervals_1", [600], staircase(), [(0, 10, 309)], [150.5]))
    iv = [(0, 10 + (i * 37) % 200, 10 + (i * 37) % 200 + (i * 11) % 100) for i in range(300)]
    iv[150:160] = iv[:10]
    C.append(case("intervals_300", [600], staircase(), iv, [(s + e) / 2 - 9 for _, s, e in iv]))
    return C


def refusals():
    """-> [(name, tlens, records, intervals, a piece of the reason)]: results that would send k_depth_diff outside its target's slice, and
    an interval on no target.  Two targets, so that a write past the first would land in the second's slice."""
    good = [R(0, 5, [M(20)]), R(1, 0, [M(30)])]
    iv = [(0, 0, 49), (1, 0, 29)]
    out = []
    bad = R(0, 5, [M(5)]); bad["ts"] = -1
    out.append(("ts_negative", [50, 30], good + [bad], iv, "record 2: coordinates"))
    out.append(("te_before_ts", [50, 30], [R(0, 10, [M(5)], te=9)] + good, iv, "record 0: coordinates"))
    out.append(("te_beyond_tlen", [50, 30], good + [R(0, 45, [M(6)])], iv, "record 2: te beyond its target's end"))
    out.append(("te_beyond_tlen_last_target", [50, 30], good + [R(1, 0, [M(31)])], iv, "record 2: te beyond its target's end"))
    out.append(("cigar_beyond_te_M", [50, 30], good + [R(0, 45, [M(10)], te=50)], iv, "record's CIGAR leaves its target"))
    out.append(("cigar_beyond_te_D_then_M", [50, 30], good + [R(0, 45, [M(2), D(10), M(3)], te=50)], iv, "record's CIGAR leaves its target"))
    out.append(("cigar_beyond_te_huge_ops", [50, 30], good + [R(1, 0, [D((1 << 28) - 1)] * 20 + [M(1)], te=30)], iv, "record's CIGAR leaves its target"))
    out.append(("tid_outside", [50, 30], good + [R(2, 0, [M(5)])], iv, "record 2: tid outside n_targets"))
    out.append(("interval_tid_outside", [50, 30], good, iv + [(2, 0, 5)], "interval 2: tid outside n_targets"))
    out.append(("interval_tid_negative", [50, 30], good, [(-1, 0, 5)] + iv, "interval 0: tid outside n_targets"))
    return out


GOOD = case("after_a_refusal", [50, 30], [R(0, 5, [M(20)]), R(1, 0, [M(30)])], [(0, 0, 49), (1, 0, 29), (0, 24, 25)], [0, 1, 0.5])
