"""Hand-built records and calls for the genotyping step, one case per rule of its definition, with the reference and ambiguous
reads worked out by hand (tests/test_genotype_ref.py holds tests/genotype_ref.py to them; tests/test_gpu_genotype.py holds the engine
to genotype_ref on the same input and on the larger ones built here)."""
import numpy as np

from inscall_cases import rec, pack, simple, ops_record, OPS  # noqa: F401  (pack / simple / ops_record: for the tests)


def grec(qid, ts, cig, tid=0, flags=0, mapq=60, te=None):
    """a record at ts whose read is its CIGAR's query bases end to end; te from the CIGAR unless given (a record without ops)"""
    q = sum(n for n, o in cig if o in "MI")
    t = sum(n for n, o in cig if o in "MD")
    return rec(qid, q, 0, q, ts, ts + t if te is None else te, cig, tid=tid, flags=flags, mapq=mapq)


def flat(qid, ts, te, **kw):
    """one M from ts to te"""
    return grec(qid, ts, [(te - ts, "M")], **kw)


def with_ins(qid, ts, te, at, n, **kw):
    """ts .. te with an I of n bases at reference position `at`"""
    return grec(qid, ts, [(at - ts, "M"), (n, "I"), (te - at, "M")], **kw)


def with_del(qid, ts, te, at, n, **kw):
    """ts .. te with a D of n bases covering [at, at + n)"""
    return grec(qid, ts, [(at - ts, "M"), (n, "D"), (te - at - n, "M")], **kw)


def call(tid, pos, reads, support=None):
    reads = sorted(reads)
    return dict(tid=tid, pos=pos, len=0, support=len(reads) if support is None else support, n_sized=0, rep=-1, reads=reads)


def G(ref_reads, ambig_reads, alt, gt):
    return dict(ref=len(ref_reads), ambig=len(ambig_reads), alt=alt, gt=gt, ref_reads=ref_reads, ambig_reads=ambig_reads)


SUP = [900, 901, 902]           # supporters that have no record at all: alt = 3


def hand_cases():
    """-> list of (name, records, calls, options, expected: one G per call).  Defaults: flank 50, so the window of a call at 1000
    is [950, 1050]; max_window_indel 20; hom 80 %, het 30 %"""
    C = []
    # ts == pos - flank spans, one base past it does not.  alt 3, ref 1: 300 >= 80 * 4 fails, 300 >= 30 * 4 -> 0/1
    C.append(("ts_edge", [flat(0, 950, 1200), flat(1, 951, 1200)], [call(0, 1000, SUP)], {}, [G([0], [], 3, 1)]))
    # te == pos + flank spans, one base short of it does not
    C.append(("te_edge", [flat(0, 800, 1050), flat(1, 800, 1049)], [call(0, 1000, SUP)], {}, [G([0], [], 3, 1)]))
    # pos < flank: max(0, 30 - 50) = 0, so only a record that starts at 0 spans; te >= 80 is still asked
    C.append(("pos_below_flank", [flat(0, 0, 80), flat(1, 1, 200), flat(2, 0, 79)], [call(0, 30, SUP)], {}, [G([0], [], 3, 1)]))
    # flank 0: ts <= pos <= te, and only an I at p == pos lies in the window.  Read 0: I of 21 at 1000 -> unclean; read 1: the same I
    # at 999 -> clean; read 2 starts at 1001, read 3 ends at 999: no span; read 4 ends at 1000: spans
    C.append(("flank_zero", [with_ins(0, 900, 1100, 1000, 21), with_ins(1, 900, 1100, 999, 21), flat(2, 1001, 1100), flat(3, 900, 999), flat(4, 900, 1000)],
              [call(0, 1000, SUP)], dict(flank=0), [G([1, 4], [0], 3, 1)]))
    # an I of 21 at p = pos - flank - 1 and pos + flank + 1 is outside (clean), at pos - flank and pos + flank inside (unclean)
    C.append(("ins_at_window_edges", [with_ins(0, 900, 1100, 949, 21), with_ins(1, 900, 1100, 950, 21), with_ins(2, 900, 1100, 1050, 21), with_ins(3, 900, 1100, 1051, 21)],
              [call(0, 1000, SUP)], {}, [G([0, 3], [1, 2], 3, 1)]))
    # a D across the left edge counts its bases from pos - flank on: [940, 970) -> 20 (clean), [940, 971) -> 21 (unclean); across the
    # right edge up to pos + flank: [1030, 1070) -> 20 (clean), [1029, 1069) -> 21 (unclean)
    C.append(("del_across_window_edges", [with_del(0, 900, 1100, 940, 30), with_del(1, 900, 1100, 940, 31), with_del(2, 900, 1100, 1030, 40), with_del(3, 900, 1100, 1029, 40)],
              [call(0, 1000, SUP)], {}, [G([0, 2], [1, 3], 3, 1)]))
    # window indel == max_window_indel is clean, one more is not: an I alone, and an I and a D added up
    C.append(("indel_at_threshold", [with_ins(0, 900, 1100, 1000, 20), with_ins(1, 900, 1100, 1000, 21),
                                     grec(2, 900, [(80, "M"), (10, "I"), (40, "M"), (10, "D"), (70, "M")]), grec(3, 900, [(80, "M"), (10, "I"), (40, "M"), (11, "D"), (69, "M")])],
              [call(0, 1000, SUP)], {}, [G([0, 2], [1, 3], 3, 1)]))
    # a supporter that spans is neither a reference nor an ambiguous read.  alt 2, ref 1: 200 >= 240 fails -> 0/1
    C.append(("supporter_spans", [flat(0, 900, 1100), with_ins(1, 900, 1100, 1000, 40), flat(2, 900, 1100)], [call(0, 1000, [0, 1])], {}, [G([2], [], 2, 1)]))
    # two spanning records of a read: clean + unclean -> reference; unclean + unclean -> ambiguous, once
    C.append(("two_records_of_a_read", [with_ins(0, 900, 1100, 1000, 40), flat(0, 800, 1200, flags=4), with_ins(1, 900, 1100, 1000, 40), with_del(1, 800, 1200, 990, 30, flags=4)],
              [call(0, 1000, SUP)], {}, [G([0], [1], 3, 1)]))
    # a secondary record is no evidence
    C.append(("secondary", [flat(0, 900, 1100, flags=2), flat(1, 900, 1100)], [call(0, 1000, SUP)], {}, [G([1], [], 3, 1)]))
    # mapq 19 is out, 20 is in
    C.append(("mapq_edge", [flat(0, 900, 1100, mapq=19), flat(1, 900, 1100, mapq=20)], [call(0, 1000, SUP)], {}, [G([1], [], 3, 1)]))
    # a record on another target spans nothing here; the same position on its own target has it.  alt 3, ref 0 -> 1/1
    C.append(("other_tid", [flat(0, 900, 1100, tid=1)], [call(0, 1000, SUP), call(1, 1000, SUP)], {}, [G([], [], 3, 2), G([0], [], 3, 1)]))
    # GT: hom 80 % with alt 4: ref 0 -> 400 >= 320, ref 1 -> 400 >= 400 (equality) 1/1, ref 2 -> 400 < 480 -> 0/1;
    #     het 30 % with alt 3: ref 6 -> 300 >= 270, ref 7 -> 300 >= 300 (equality) 0/1, ref 8 -> 300 < 330 -> 0/0
    recs, calls, want = [], [], []
    for k, (alt, ref, gt) in enumerate(((4, 0, 2), (4, 1, 2), (4, 2, 1), (3, 6, 1), (3, 7, 1), (3, 8, 0))):
        pos = 10000 * (k + 1)
        rr = [100 * k + j for j in range(ref)]
        recs += [flat(q, pos - 100, pos + 100) for q in rr]
        calls.append(call(0, pos, [900 + j for j in range(alt)]))
        want.append(G(rr, [], alt, gt))
    C.append(("gt_thresholds", recs, calls, {}, want))
    # a record without CIGAR ops has window indel 0
    C.append(("no_cigar", [grec(0, 900, [], te=1100)], [call(0, 1000, SUP)], {}, [G([0], [], 3, 1)]))
    return C


def ref_pos(r):
    """reference position before every op of a record with CIGAR words, and after the last"""
    w = np.asarray(r["cig"], np.uint32)
    ln, op = (w >> 4).astype(np.int64), w & 15
    return r["ts"] + np.concatenate([[0], np.cumsum(np.where((op == 0) | (op == 2), ln, 0))])


def gpu_cases():
    """-> list of (name, records, calls, options): shapes at which the device code takes another path (the checker supplies the answer)"""
    C = []
    # a record that spans 1, 64, 65 and more than 4,096 calls (a scan tile) 200 bases apart; read 1 has an I next to the first call
    # only, read 2 spans the first ten calls and supports the first
    for n in (1, 64, 65, 4100):
        end = 1000 + 200 * n + 100
        recs = [flat(0, 0, end), with_ins(1, 0, end, 1010, 30), flat(2, 500, 1000 + 200 * 9 + 50), flat(3, 0, end, tid=1)]
        C.append(("span_%d" % n, recs, [call(0, 1000 + 200 * k, [2] if k == 0 else [901, 902]) for k in range(n)], {}))
    # one call with more than 2,048 spanning reads (a sort tile): every third unclean, every seventh with a second (clean) record, the
    # first ten supporters
    recs = []
    for q in range(2100):
        recs.append(with_ins(q, 4000 + q % 50, 6000 + q % 50, 5000 + q % 13, 25) if q % 3 == 0 else flat(q, 4000 + q % 50, 6000 + q % 50))
        if q % 7 == 0:
            recs.append(flat(q, 3000, 7000, flags=4))
    C.append(("reads_2100", recs, [call(0, 5000, range(10))], {}))
    # a CIGAR of 63 / 64 / 65 ops: calls along it, flank 20
    for n in (63, 64, 65):
        r = ops_record(0, n, 1000, [])
        p = ref_pos(r)
        C.append(("ops_%d" % n, [r], [call(0, int(x), SUP) for x in sorted(set([1020, int(p[n // 2]), int(p[n - 1]), int(p[-1]) - 20]))], dict(flank=20)))
    # 100,000 ops: the window in the first step of 64 ops, across the boundaries of a step, and in the last step
    big = ops_record(0, 100001, 1000, [])
    p = ref_pos(big)
    C.append(("ops_100k", [big, flat(1, 0, 2000)], [call(0, int(x), SUP) for x in (1060, int(p[64]), int(p[64 * 700]) + 1, int(p[64 * 1500 - 1]), int(p[-1]) - 60)], {}))
    # a window wholly inside one long D
    C.append(("inside_long_del", [with_del(0, 0, 2000, 500, 1000), flat(1, 0, 2000)], [call(0, 1000, SUP)], {}))
    # the records of a result need not be in read order
    C.append(("not_in_read_order", [flat(5, 900, 1100), with_ins(3, 900, 1100, 1000, 40), flat(4, 900, 1100), flat(3, 800, 1300, flags=4), with_ins(1, 900, 1100, 990, 21),
                                    flat(5, 0, 5000, flags=4), flat(0, 900, 1100)], [call(0, 1000, [4]), call(0, 1200, [0])], {}))
    # calls on two targets where the first target has none
    C.append(("first_target_without_calls", [flat(0, 900, 1100), flat(1, 900, 1100, tid=1), with_ins(2, 900, 2100, 2000, 21, tid=1)],
              [call(1, 1000, SUP), call(1, 2000, SUP)], {}))
    return C


def many_pairs():
    """more than 65,536 pairs: 300 calls, each spanned by 230 records (every read spans every call; every fifth read carries an I of
    25 next to the calls whose number is its own modulo 7, read 3 has a second record)"""
    calls = [call(0, 5000 + 300 * k, [1, 2] if k % 2 else [229]) for k in range(300)]
    end = 5000 + 300 * 300 + 100
    recs = []
    for q in range(230):
        if q % 5 == 0:
            cig, at = [], 0
            for k in range(q % 7, 300, 7):
                pos = 5000 + 300 * k + 3
                cig += [(pos - at, "M"), (25, "I")]
                at = pos
            recs.append(grec(q, 0, cig + [(end - at, "M")]))
        else:
            recs.append(flat(q, 0, end))
    recs.append(flat(3, 100, end + 100, flags=4))
    return recs, calls, {}
