"""Hand-built records and sites for telr_call_at_sites, one case per rule of its definition, with the kept signatures and the calls
worked out by hand (tests/test_sitecall_ref.py holds tests/sitecall_ref.py to them; tests/test_gpu_sitecall.py holds the engine to
sitecall_ref on the same cases and on the generated one built here).  Records come from inscall_cases' rec / pack / simple."""
import numpy as np

from inscall_cases import rec, pack, simple, K
from sitecall_ref import E_ARG, E_RANGE, MAX_SITES

N_TARGETS = 3          # the cases use targets 0, 1 and 2


def clip(qid, ts, tid=0):
    """a read of 1,000 bases whose first 300 are unaligned: a clip signature (kind 2, len 300) at ts"""
    return rec(qid, 1000, 300, 1000, ts, ts + 700, [(700, "M")], tid=tid)


def hand_cases():
    """-> list of (name, records, sites, options, site options, kept: [(pos, qid, kind, len), ...] in sorted order, expected calls)"""
    C = []
    # |d| = reach (50) is near, reach + 1 is not, on either side.  Kept: 950 (q0, 70), 1050 (q2, 60): the median of (60, q2), (70, q0) is
    # the first = kept signature 1
    C.append(("reach_edge", [simple(0, 950, 70), simple(1, 949, 60), simple(2, 1050, 60), simple(3, 1051, 60)], [(0, 1000, 0)], {}, {},
              [(950, 0, 0, 70), (1050, 2, 0, 60)], [K(0, 1000, 60, 2, 2, 1, [0, 2])]))
    # two sites 40 apart (closer than reach).  1020 is 20 from both: the lower index.  1021: 21 and 19 -> site 1.  1045 is near both (45, 5)
    # -> site 1.  960: 40 from site 0, 80 from site 1.  Kept: 960 q3 | 1020 q0 | 1021 q1 | 1045 q2; all len 60: by qid q0 (kept 1) and q1 (kept 2)
    C.append(("equidistant_and_close_sites", [simple(0, 1020, 60), simple(1, 1021, 60), simple(2, 1045, 60), simple(3, 960, 60)],
              [(0, 1000, 0), (0, 1040, 0)], {}, {}, [(960, 3, 0, 60), (1020, 0, 0, 60), (1021, 1, 0, 60), (1045, 2, 0, 60)],
              [K(0, 1000, 60, 2, 2, 1, [0, 3]), K(0, 1040, 60, 2, 2, 2, [1, 2])]))
    # the same position on two targets; a signature at (1, 20) has the site of target 0 below its key and one 980 away above it: dropped
    C.append(("same_pos_two_targets", [simple(0, 1000, 60), simple(1, 1000, 70, tid=1), simple(2, 1010, 80, tid=1), simple(3, 20, 60, tid=1)],
              [(0, 1000, 0), (1, 1000, 0)], {}, {}, [(1000, 0, 0, 60), (1000, 1, 0, 70), (1010, 2, 0, 80)],
              [K(0, 1000, 60, 1, 1, 0, [0]), K(1, 1000, 70, 2, 2, 1, [1, 2])]))
    # a site at position 0: pos - reach is negative.  An I as the first op signs at 0.  Kept: 0 (q1, rec 1), 10 (q0, rec 0), both 60: q0 first
    C.append(("site_at_zero", [simple(0, 10, 60), rec(1, 80, 0, 80, 0, 20, [(60, "I"), (20, "M")]), simple(2, 51, 60)], [(0, 0, 0)], {}, {},
              [(0, 1, 0, 60), (10, 0, 0, 60)], [K(0, 0, 60, 2, 2, 1, [0, 1])]))
    # a site without a signature between two that have one: reported, empty
    C.append(("empty_site_between", [simple(0, 1000, 60), simple(1, 3000, 70)], [(0, 1000, 0), (0, 2000, 0), (0, 3000, 0)], {}, {},
              [(1000, 0, 0, 60), (3000, 1, 0, 70)], [K(0, 1000, 60, 1, 1, 0, [0]), K(0, 2000, 0, 0, 0, -1, []), K(0, 3000, 70, 1, 1, 1, [1])]))
    # one read with a clip (at 2000) and an I (at 2020) at one site counts once, and is sized
    C.append(("ins_and_clip_of_one_read", [rec(0, 1000, 300, 1000, 2000, 2640, [(20, "M"), (60, "I"), (620, "M")])], [(0, 2010, 0)], {}, {},
              [(2000, 0, 2, 300), (2020, 0, 0, 60)], [K(0, 2010, 60, 1, 1, 1, [0])]))
    # two records of one read sign at one site: one supporter
    C.append(("two_records_of_one_read", [simple(0, 1000, 60), simple(0, 1005, 70, flags=4)], [(0, 1000, 0)], {}, {},
              [(1000, 0, 0, 60), (1005, 0, 0, 70)], [K(0, 1000, 60, 1, 1, 0, [0])]))
    # clips only: no length, no representative
    C.append(("clips_only", [clip(q, 2000 + q) for q in range(3)], [(0, 2001, 0)], {}, {},
              [(2000, 0, 2, 300), (2001, 1, 2, 300), (2002, 2, 2, 300)], [K(0, 2001, 0, 3, 0, -1, [0, 1, 2])]))
    # four sized signatures of one length: the order is (len, qid, rec, mate) = (q3, rec 1), (q3, rec 3), (q4, rec 2), (q5, rec 0); the lower
    # median is the second = the signature at 1003 = kept 3
    C.append(("median_on_equal_len", [simple(5, 1000, 60), simple(3, 1001, 60), simple(4, 1002, 60), simple(3, 1003, 60, flags=4)], [(0, 1000, 0)], {}, {},
              [(1000, 5, 0, 60), (1001, 3, 0, 60), (1002, 4, 0, 60), (1003, 3, 0, 60)], [K(0, 1000, 60, 3, 3, 3, [3, 4, 5])]))
    # length test at len 200, 10 %: kept iff 100 * |d| <= 2000.  220 and 180 sit on the bound (kept), 221 and 179 one above (dropped)
    C.append(("len_test_edge", [simple(0, 1000, 220), simple(1, 1000, 221), simple(2, 1000, 180), simple(3, 1000, 179)], [(0, 1000, 200)], {}, dict(len_pct=10),
              [(1000, 0, 0, 220), (1000, 2, 0, 180)], [K(0, 1000, 180, 2, 2, 1, [0, 2])]))
    # 1010 is nearest to site 0 (10 against 20), whose length test rejects it; site 1 (len 0: no test) would have taken it, and does not get it
    C.append(("len_reject_is_not_handed_on", [simple(0, 1010, 60), simple(1, 1025, 60)], [(0, 1000, 200), (0, 1030, 0)], {}, dict(len_pct=10),
              [(1025, 1, 0, 60)], [K(0, 1000, 0, 0, 0, -1, []), K(0, 1030, 60, 1, 1, 0, [1])]))
    # a clip of 300 at a site of len 100 stays (clips are not tested); an I of 300 there goes
    C.append(("clips_exempt_from_len_test", [clip(0, 2000), simple(1, 2000, 300)], [(0, 2000, 100)], {}, dict(len_pct=10),
              [(2000, 0, 2, 300)], [K(0, 2000, 0, 1, 0, -1, [0])]))
    # len_pct > 0 at a site of unknown length: no test
    C.append(("len_pct_with_site_len_zero", [simple(0, 1000, 60), simple(1, 1000, 5000)], [(0, 1000, 0)], {}, dict(len_pct=1),
              [(1000, 0, 0, 60), (1000, 1, 0, 5000)], [K(0, 1000, 60, 2, 2, 0, [0, 1])]))
    # mapq below min_mapq and a secondary record give nothing
    C.append(("ineligible_records", [simple(0, 1000, 60, mapq=19), simple(1, 1000, 60, flags=2), simple(2, 1000, 60)], [(0, 1000, 0)], {}, {},
              [(1000, 2, 0, 60)], [K(0, 1000, 60, 1, 1, 0, [2])]))
    # a wider reach and another min_len come from the options: the I of 40 signs at min_len 40, 120 away is near at reach 120
    C.append(("options_are_read", [simple(0, 1120, 40), simple(1, 1121, 40)], [(0, 1000, 0)], dict(min_len=40), dict(reach=120),
              [(1120, 0, 0, 40)], [K(0, 1000, 40, 1, 1, 0, [0])]))
    # min_support, min_sized and cluster_dist are not read: values telr_call_insertions refuses change nothing
    C.append(("cluster_options_not_read", [simple(0, 1000, 60)], [(0, 1000, 0)], dict(min_support=-1, min_sized=5, cluster_dist=-7), {},
              [(1000, 0, 0, 60)], [K(0, 1000, 60, 1, 1, 0, [0])]))
    # zero sites: an empty result; zero eligible records, or eligible ones without a signature: a call per site, all empty
    C.append(("zero_sites", [simple(0, 1000, 60)], [], {}, {}, [], []))
    C.append(("zero_records", [], [(0, 5, 0)], {}, {}, [], [K(0, 5, 0, 0, 0, -1, [])]))
    C.append(("zero_eligible_records", [simple(0, 1000, 60, mapq=3), simple(1, 1000, 60, flags=2)], [(0, 1000, 0), (2, 7, 9)], {}, {},
              [], [K(0, 1000, 0, 0, 0, -1, []), K(2, 7, 0, 0, 0, -1, [])]))
    C.append(("no_signature", [simple(0, 1000, 20)], [(0, 1000, 0), (1, 1000, 0)], {}, {}, [], [K(0, 1000, 0, 0, 0, -1, []), K(1, 1000, 0, 0, 0, -1, [])]))
    # signatures, none of them near a site
    C.append(("nothing_kept", [simple(0, 1000, 60), simple(1, 5000, 60, tid=1)], [(0, 2000, 0), (2, 1000, 0)], {}, {},
              [], [K(0, 2000, 0, 0, 0, -1, []), K(2, 1000, 0, 0, 0, -1, [])]))
    return C


def refusals():
    """-> list of (name, records, sites, options, site options, n_sites or None (= len(sites); sites None: a null pointer), code)"""
    ok, one = [simple(0, 1000, 60)], [(0, 1000, 0)]
    R = [("opt_" + k, ok, one, {k: -1}, {}, None, E_ARG) for k in ("min_len", "min_mapq", "min_clip", "max_ref_gap")]
    R += [("record_tid", [simple(0, 1000, 60, tid=N_TARGETS)], one, {}, {}, None, E_ARG),
          ("record_coordinates", [rec(0, 80, 0, 80, 990, 980, [(10, "M")])], one, {}, {}, None, E_ARG),
          ("sites_equal", ok, [(0, 1000, 0), (0, 1000, 5)], {}, {}, None, E_ARG),
          ("sites_descend_pos", ok, [(0, 1000, 0), (0, 999, 0)], {}, {}, None, E_ARG),
          ("sites_descend_tid", ok, [(1, 5, 0), (0, 1000, 0)], {}, {}, None, E_ARG),
          ("site_tid_high", ok, [(N_TARGETS, 1000, 0)], {}, {}, None, E_ARG),
          ("site_tid_negative", ok, [(-1, 1000, 0)], {}, {}, None, E_ARG),
          ("site_pos_negative", ok, [(0, -1, 0)], {}, {}, None, E_ARG),
          ("site_len_negative", ok, [(0, 1000, -1)], {}, {}, None, E_ARG),
          ("reach_negative", ok, one, {}, dict(reach=-1), None, E_ARG),
          ("len_pct_negative", ok, one, {}, dict(len_pct=-1), None, E_ARG),
          ("len_pct_101", ok, one, {}, dict(len_pct=101), None, E_ARG),
          ("reserved0", ok, one, {}, dict(reserved0=1), None, E_ARG),
          ("reserved1", ok, one, {}, dict(reserved1=1), None, E_ARG),
          ("n_sites_negative", ok, one, {}, {}, -1, E_ARG),
          ("sites_null", ok, None, {}, {}, 1, E_ARG),
          ("too_many_sites", ok, one, {}, {}, MAX_SITES, E_RANGE)]       # refused by its count: the array is never read
    return R


def multi(qid, pos, lens, gaps, tid=0, flags=0, mapq=60, clipped=False):
    """a forward record with an I of lens[k] after every M: 10M I gaps[0]M I ... 10M, the first I at `pos`; clipped: 250 bases in front"""
    cig, q, t = [(10, "M")], 10, 10
    for k, ln in enumerate(lens):
        g = gaps[k] if k < len(lens) - 1 else 10
        cig += [(ln, "I"), (g, "M")]
        q += ln + g; t += g
    qs = 250 if clipped else 0
    return rec(qid, qs + q, qs, qs + q, pos - 10, pos - 10 + t, cig, tid=tid, flags=flags, mapq=mapq)


def generated():
    """-> (records, sites, options, site options): three targets, 700 sites, 3,000 records of three I runs each (a tenth with a clip too):
    about 9,000 signatures, more than 4,096 of them kept (a scan tile, and many 256-lane blocks), the sites around one position with some 1,800 between them (a run
    crosses several blocks), and 300 records in a stretch without a site: some 900 consecutive signatures, so whole blocks, keep nothing."""
    rng = np.random.default_rng(20261021)
    sites = []
    for tid, n in ((0, 300), (1, 250), (2, 150)):
        pos = 500 + np.cumsum(rng.integers(20, 400, size=n))          # some closer together than reach
        if tid == 1:
            pos[125:] += 200000                                       # the stretch without a site
        sites += [(tid, int(p), int(rng.choice((0, 0, 200)))) for p in pos]
    hot = sites[40]
    hole = sites[300 + 124][1] + 50000
    recs = []
    for i in range(3000):
        share = i % 10 == 9                                           # a second record of the read before
        qid = len(recs) - 1 if share else len(recs)
        lens = [int(x) for x in rng.integers(60, 400, size=3)]
        gaps = [int(x) for x in rng.integers(1, 40, size=2)]
        if i < 600:
            tid, pos = hot[0], hot[1] + int(rng.integers(-45, 30))
        elif i < 900:
            tid, pos = 1, hole + int(rng.integers(0, 5000))
        else:
            s = sites[int(rng.integers(0, len(sites)))]
            tid, pos = s[0], max(20, s[1] + int(rng.integers(-90, 70)))
        recs.append(multi(qid, pos, lens, gaps, tid=tid, flags=4 if share else 0, mapq=5 if i % 37 == 0 else 60, clipped=i % 10 == 3))
    return recs, sites, {}, dict(reach=50, len_pct=50)
