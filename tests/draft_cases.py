"""Hand-built records for the draft step (telr_draft_contigs): one case per rule of its definition with the answer
worked out by hand (tests/test_draft_ref.py holds tests/draft_ref.py to them), and the tables of shapes at which the device code takes
another path (tests/test_gpu_draft.py holds the engine to draft_ref on them; every case names the edge it claims)."""
import numpy as np

import inscall_ref as iref
from inscall_cases import rec, pack

NO_CLIP = dict(min_clip=1 << 30, min_mapq=0)
SMALL = dict(flank=20, min_flank=5)


def sigs_of(alns, cig, min_len=50):
    return iref.signatures(alns, cig, dict(NO_CLIP, min_len=min_len))


def call(tid, pos, ln, reads):
    return dict(tid=tid, pos=pos, len=ln, support=len(reads), n_sized=len(reads), rep=-1, reads=sorted(reads))


def S(tid, pos, ln, qid, kind, rec_, mate, seg_start, seg_len):
    return dict(tid=tid, pos=pos, len=ln, qid=qid, kind=kind, rec=rec_, mate=mate, seg_start=seg_start, seg_len=seg_len)


def D(sig, qid, start, ln, rc, ins_off, ins_len, set_index):
    return dict(sig=sig, qid=qid, start=start, len=ln, rc=rc, ins_off=ins_off, ins_len=ins_len, set_index=set_index)


NONE = D(-1, 0, 0, 0, 0, 0, 0, -1)


def ins_rec(qid, pos, ins, left=20, right=20, tid=0, flags=0):
    """a read aligned end to end: <left>M <ins>I <right>M with the insertion at `pos`"""
    return rec(qid, left + ins + right, 0, left + ins + right, pos - left, pos + right, [(left, "M"), (ins, "I"), (right, "M")], tid=tid, flags=flags)


def hand_cases():
    """-> list of (name, records, calls, signatures (None: the caller's own, min_len 50), options, expected drafts)"""
    C = []
    # flank 20 reaches past both ends: xL = ts = 100 -> lo = qs' = 0, xR = te = 120 -> hi = 70.  The segment starts at 10: ins_off 10.
    C.append(("ends_at_ts_te", [rec(0, 70, 0, 70, 100, 120, [(10, "M"), (50, "I"), (10, "M")])], [call(0, 110, 50, [0])], None, SMALL,
              [D(0, 0, 0, 70, 0, 10, 50, 0)]))
    # 10M 2D 10M 50I 10M 3I 10M from 100: the I of 50 at 122 after 20 read bases.  flank 10: xL = 112 is where the D ends and the next M
    # starts: one state, (112, 10).  xR = 132 is where an M ends and the I of 3 sits: states (132, 80) and (132, 83), hi = 83 -- the I is
    # inside the draft.  n = 73, ins_off = 20 - 10.
    C.append(("op_boundary_and_I_at_xR", [rec(0, 93, 0, 93, 100, 142, [(10, "M"), (2, "D"), (10, "M"), (50, "I"), (10, "M"), (3, "I"), (10, "M")])],
              [call(0, 122, 50, [0])], None, dict(flank=10, min_flank=5), [D(0, 0, 10, 73, 0, 10, 50, 0)]))
    # 10M 3I 10M 50I 20M from 100: the I of 50 at 120 after 23 read bases.  flank 10: xL = 110 holds the states (110, 10) and (110, 13);
    # lo is the smaller one, so the draft starts at base 10, before the I of 3 (a draft begins at lo and ends at hi: an I that sits exactly
    # on either end coordinate is inside it).  xR = 130 inside the last M: hi = 73 + 10.  n = 73, ins_off = 23 - 10.
    C.append(("I_at_xL", [rec(0, 93, 0, 93, 100, 140, [(10, "M"), (3, "I"), (10, "M"), (50, "I"), (20, "M")])],
              [call(0, 120, 50, [0])], None, dict(flank=10, min_flank=5), [D(0, 0, 10, 73, 0, 13, 50, 0)]))
    # 10M 20D 10M 50I 30M from 100: the I at 140 after 20 read bases.  flank 25: xL = 115 inside the D over [110, 130): lo = hi = 10.
    # xR = min(170, 165) = 165, 25 bases into the last M that starts at (140, 70): hi = 95.  n = 85, ins_off = 10.
    C.append(("xL_inside_D", [rec(0, 100, 0, 100, 100, 170, [(10, "M"), (20, "D"), (10, "M"), (50, "I"), (30, "M")])],
              [call(0, 140, 50, [0])], None, dict(flank=25, min_flank=5), [D(0, 0, 10, 85, 0, 10, 50, 0)]))
    # a split with b.ts < a.te (tgap -50): a = [0, 100) at 1000-1100, b = [600, 700) at 1050-1150.  len = 500 + 50, segment [100, 600).
    # flank 40: xL = 1060 -> lo_a = 60; rpos = b.ts = 1050, xR = 1090 -> hi_b = 640.  n = 580, ins_off = 40; both flanks 40.
    C.append(("split_negative_tgap", [rec(0, 1000, 0, 100, 1000, 1100, [(100, "M")]), rec(0, 1000, 600, 700, 1050, 1150, [(100, "M")], flags=4)],
              [call(0, 1100, 550, [0])], None, dict(flank=40, min_flank=40), [D(0, 0, 60, 580, 0, 40, 500, 0)]))
    # reverse strand (inscall_cases "reverse"): forward [250, 700) of 1,000, qs' = 300; 200M 100I 150M from 1000: the I at 1200 = strand
    # [500, 600) = forward [400, 500).  flank 50: xL = 1150 -> lo = 450, xR = 1250 -> hi = 650.  On the forward read start = 1000 - 650, rc.
    # The two clip signatures (kind 2) around it are no candidates: the I is signature 1 of (1000 clip, 1200 I, 1350 clip).
    C.append(("reverse", [rec(0, 1000, 250, 700, 1000, 1350, [(200, "M"), (100, "I"), (150, "M")], flags=8)], [call(0, 1200, 100, [0])],
              [S(0, 1000, 300, 0, 2, 0, -1, 700, 300), S(0, 1200, 100, 0, 0, 0, -1, 400, 100), S(0, 1350, 250, 0, 2, 0, -1, 0, 250)],
              dict(flank=50, min_flank=50), [D(1, 0, 350, 200, 1, 50, 100, 0)]))
    # the key, field by field (call at 1000 of length 60, flank 20):
    # |len - 60| first: read 1's I of 62 with flanks of 6 beats read 0's I of 70 with flanks of 20
    C.append(("key_len", [ins_rec(0, 1000, 70), ins_rec(1, 1000, 62, 6, 6)], [call(0, 1000, 60, [0, 1])], None, SMALL, [D(1, 1, 0, 74, 0, 6, 62, 0)]))
    # then the larger of the smaller flanks: 62 with flanks (6, 20) loses to 58 with flanks (20, 20)
    C.append(("key_flank", [ins_rec(0, 1000, 62, 6, 20), ins_rec(1, 1000, 58)], [call(0, 1000, 60, [0, 1])], None, SMALL, [D(1, 1, 0, 98, 0, 20, 58, 0)]))
    # then the smaller read id: records 0 and 1 are alike, read 2 (record 1) beats read 3 (record 0) although its signature comes second
    C.append(("key_qid", [ins_rec(3, 1000, 62), ins_rec(2, 1000, 62)], [call(0, 1000, 60, [2, 3])], None, SMALL, [D(1, 2, 0, 102, 0, 20, 62, 0)]))
    # then the smaller record: two records of read 0 alike but for one base of position; record 1 sorts first in the array (pos 999),
    # record 0 (pos 1000) wins
    C.append(("key_rec", [ins_rec(0, 1000, 62), ins_rec(0, 999, 62, flags=4)], [call(0, 1000, 60, [0])], None, SMALL, [D(1, 0, 0, 102, 0, 20, 62, 0)]))
    # then the smaller mate: a = record 0, mates 2 and 1 give the same length (b later on the read by as much as on the reference) and
    # the same flanks; the signature of mate 2 is put first in the array, mate 1 wins.  lo_a(1080) = 80, hi_b(1120): record 1 starts at
    # (1100, 600) -> 620, record 2 at (1150, 650) -> xR = 1170 -> 670.
    split3 = [rec(0, 2000, 0, 100, 1000, 1100, [(100, "M")]), rec(0, 2000, 600, 700, 1100, 1200, [(100, "M")], flags=4),
              rec(0, 2000, 650, 750, 1150, 1250, [(100, "M")], flags=4)]
    C.append(("key_mate", split3, [call(0, 1100, 500, [0])], [S(0, 1100, 500, 0, 1, 0, 2, 100, 550), S(0, 1100, 500, 0, 1, 0, 1, 100, 500)], SMALL,
              [D(1, 0, 80, 540, 0, 20, 500, 0)]))
    # min_flank at its edge: a left flank of 5 passes min_flank 5 and fails 6; so does a right flank of 5
    for side, r in (("left", ins_rec(0, 1000, 60, 5, 20)), ("right", ins_rec(0, 1000, 60, 20, 5))):
        for mf, want in ((4, D(0, 0, 0, 85, 0, r["cig"][0][0], 60, 0)), (5, D(0, 0, 0, 85, 0, r["cig"][0][0], 60, 0)), (6, NONE)):
            C.append(("min_flank_%s_%d" % (side, mf), [r], [call(0, 1000, 60, [0])], None, dict(flank=20, min_flank=mf), [want]))
    # max_len at its edge: the piece is 20 + 60 + 20 = 100 bases
    for ml, want in ((99, NONE), (100, D(0, 0, 0, 100, 0, 20, 60, 0)), (101, D(0, 0, 0, 100, 0, 20, 60, 0))):
        C.append(("max_len_%d" % ml, [ins_rec(0, 1000, 60)], [call(0, 1000, 60, [0])], None, dict(SMALL, max_len=ml), [want]))
    # reach: 50 away is a candidate, 51 is not
    C.append(("reach_edge", [ins_rec(0, 1050, 60), ins_rec(1, 2051, 60)], [call(0, 1000, 60, [0]), call(0, 2000, 60, [1])], None, SMALL,
              [D(0, 0, 0, 100, 0, 20, 60, 0), NONE]))
    # one signature within reach of two calls, its read a supporter of both: both calls get its piece, the set holds it twice
    C.append(("two_calls_one_signature", [ins_rec(0, 1020, 60)], [call(0, 1000, 60, [0]), call(0, 1040, 60, [0])], None, SMALL,
              [D(0, 0, 0, 100, 0, 20, 60, 0), D(0, 0, 0, 100, 0, 20, 60, 1)]))
    # no valid candidate: the read is no supporter of the call | another target | a record without CIGAR ops | only a clip
    C.append(("not_a_supporter", [ins_rec(0, 1000, 60)], [call(0, 1000, 60, [1])], None, SMALL, [NONE]))
    C.append(("other_target", [ins_rec(0, 1000, 60, tid=1)], [call(0, 1000, 60, [0])], None, SMALL, [NONE]))
    C.append(("no_cigar", [rec(0, 1000, 0, 100, 1000, 1100, []), rec(0, 1000, 600, 700, 1100, 1200, [(100, "M")], flags=4)],
              [call(0, 1100, 500, [0])], None, SMALL, [NONE]))
    C.append(("clip_only", [ins_rec(0, 1000, 60)], [call(0, 980, 0, [0])], [S(0, 980, 300, 0, 2, 0, -1, 0, 300)], SMALL, [NONE]))
    return C


# ---- the device tables -----------------------------------------------------------------------------------------------------------
F = 2000          # the default flank
WALK_OPT = dict(min_flank=1)          # the walk cases keep the default flank; their short records have short flanks
PIECE_OPT = dict(min_flank=0)         # a piece may start or end on its insertion


def walk_words(n, h=None, iL=None, dL=0, iR=None, dR=0, mid_m=0):
    """n CIGAR words: M of 1..5 at the even places, at the odd places a D of 2 or (every other one) an I of 3; place h holds an I of 60
    (the signature).  Place iL < h is made an M so long that the reference bases of places [iL, h) are F + dL: xL = pos - F then lies dL
    bases into place iL (dL = 0: on the seam before it).  Place iR > h likewise: the reference bases of places (h, iR] are F + dR, xR
    lies dR bases before the end of place iR.  Without h (a record of a split): iL counts up to the end of the record, iR from its start."""
    k = np.arange(n)
    ln = (k % 5 + 1).astype(np.int64); op = np.zeros(n, np.int64)
    odd = k % 2 == 1
    ln[odd] = 2; op[odd] = 2
    ln[odd & (k % 4 == 3)] = 3; op[odd & (k % 4 == 3)] = 1
    if h is not None:
        ln[h] = 60; op[h] = 1
    ref = lambda: np.where(op != 1, ln, 0)
    if iL is not None:
        op[iL] = 0; ln[iL] = 0
        ln[iL] = F + dL - int(ref()[iL:(n if h is None else h)].sum())
        assert ln[iL] > dL
    if iR is not None:
        op[iR] = 0; ln[iR] = 0
        ln[iR] = F + dR - int(ref()[(0 if h is None else h + 1):iR + 1].sum())
        assert ln[iR] > dR
    return ((ln << 4) | op).astype(np.uint32)


def words_rec(qid, w, ts, qs=0, tail=0, flags=0):
    """a record over CIGAR words w at ts whose read has qs bases before and `tail` bases behind the aligned part (strand coordinates)"""
    ln, op = (w >> 4).astype(np.int64), w & 15
    q = int(ln[(op == 0) | (op == 1)].sum()); t = int(ln[(op == 0) | (op == 2)].sum())
    qlen = qs + q + tail
    fqs, fqe = (qlen - qs - q, qlen - qs) if flags & 8 else (qs, qs + q)
    return rec(qid, qlen, fqs, fqe, ts, ts + t, w, flags=flags)


def op_places(a, cig, x):
    """(first, last) place among the CIGAR words of record a whose reference interval [p, p + r] holds x"""
    w = cig[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])].astype(np.int64)
    r = np.where((w & 15) != 1, w >> 4, 0)
    p = int(a["ts"]) + np.concatenate([[0], np.cumsum(r)[:-1]])
    hit = np.nonzero((p <= x) & (x <= p + r))[0]
    return int(hit[0]), int(hit[-1])


def claim_holds(claim, places, n_words):
    """("first",): x in the first word; ("last",): in the last; ("in", w): strictly inside word w; ("seam", s): on the seam before word s"""
    f, l = places
    if claim[0] == "first":
        return f == 0
    if claim[0] == "last":
        return l == n_words - 1
    if claim[0] == "in":
        return f == l == claim[1]
    return f < claim[1] <= l


def walk_cases():
    """-> (records, calls, claims): one locus per case, 100,000 apart; claims[k] = (name, claim about xL, claim about xR) of call k (claim_holds):
    CIGARs of 3 .. 129 words (a record needs three for M I M) with xL / xR in the first word, the last word and on each side of the
    64-word step seams, one record of more than 100,000 words, and splits over records of 1, 63, 64, 65, 128 and 129 words in either
    record order"""
    recs, calls, claims = [], [], []

    def locus():
        return 100000 * (len(calls) + 1)

    def intra(name, n, h, iL, dL, iR, dR, wantL, wantR, flags=0):
        w = walk_words(n, h, iL, dL, iR, dR)
        q = len(calls)
        r = words_rec(q, w, locus(), qs=7, tail=9, flags=flags)
        pos = r["ts"] + int(np.where((w[:h] & 15) != 1, w[:h] >> 4, 0).sum())
        recs.append(r); calls.append(call(0, pos, 60, [q])); claims.append((name, wantL, wantR))

    intra("3_words_ts_te", 3, 1, None, 0, None, 0, ("first",), ("last",))
    for n in (63, 64, 65, 128, 129):
        h = n // 2 | 1
        intra("%d_first_last" % n, n, h, None, 0, None, 0, ("first",), ("last",))             # short flanks: xL = ts in the first word, xR = te in the last
        intra("%d_inside" % n, n, h, 2, 1, n - 1, 1, ("in", 2), ("in", n - 1))                    # one base into word 2 | one base before the end of the last word
        intra("%d_first_word" % n, n, h, 0, 3, h + 1, 0, ("in", 0), ("seam", h + 2), flags=8 if n == 65 else 0)
    # the seams of the 64-word steps, from either side: xL on the seam 63 | 64 (the first word that holds it is 63, its end), one base into
    # word 64, one base before the end of word 63; xR the same around 63 | 64 and 127 | 128
    intra("129_xL_seam_64", 129, 97, 64, 0, 128, 0, ("seam", 64), ("last",))
    intra("129_xL_in_64", 129, 97, 64, 1, 127, 1, ("in", 64), ("in", 127))
    intra("129_xL_in_63", 129, 97, 63, 1, 127, 0, ("in", 63), ("seam", 128))
    intra("129_xR_seam_64", 129, 31, 0, 0, 63, 0, ("first",), ("seam", 64))
    intra("129_xR_in_63", 129, 31, 1, 0, 63, 1, ("seam", 1), ("in", 63))
    intra("129_xR_in_64", 129, 31, 2, 0, 64, 2, ("seam", 2), ("in", 64), flags=8)
    intra("65_xR_last_seam", 65, 31, 0, 1, 64, 0, ("in", 0), ("last",))

    def split(name, na, nb, a_first, iL, iR, wantL, wantR):
        """a: na words ending at the locus, b: nb words starting 10 after it, 500 read bases apart"""
        q = len(calls)
        wa = walk_words(na, None, iL, 1 if iL is not None else 0) if na > 1 else np.array([(3000 << 4)], np.uint32)
        wb = walk_words(nb, None, None, 0, iR, 1 if iR is not None else 0) if nb > 1 else np.array([(3000 << 4)], np.uint32)
        ta = int(np.where((wa & 15) != 1, wa >> 4, 0).sum())
        qa = int(np.where((wa & 15) != 2, wa >> 4, 0).sum())
        qb = int(np.where((wb & 15) != 2, wb >> 4, 0).sum())
        pos = locus() + 50000
        a = words_rec(q, wa, pos - ta, qs=3, tail=500 + qb + 4)
        b = words_rec(q, wb, pos + 10, qs=3 + qa + 500, tail=4, flags=4)
        assert a["qlen"] == b["qlen"]
        recs.extend([a, b] if a_first else [b, a])
        calls.append(call(0, pos, 490, [q])); claims.append((name, wantL, wantR))

    split("split_1_1", 1, 1, True, None, None, ("in", 0), ("in", 0))
    split("split_63_65", 63, 65, False, 0, 64, ("in", 0), ("in", 64))
    split("split_64_64", 64, 64, True, None, None, ("first",), ("last",))
    split("split_65_63", 65, 63, True, 64, 0, ("in", 64), ("in", 0))
    split("split_128_129", 128, 129, False, 63, 64, ("in", 63), ("in", 64))
    split("split_129_128", 129, 128, True, 64, 127, ("in", 64), ("in", 127))
    # (last: its record covers a quarter of a million reference bases)
    intra("100k_words", 100003, 99999, 99937, 1, 100002, 1, ("in", 99937), ("in", 100002))
    return recs, calls, claims


def piece_cases(seed=11):
    """-> (records, calls, signatures, reads, claims): one read and one locus per piece, the piece = forward bases [start, start + len) of
    its read, forward or reverse strand: start = 0 and start = 32 + (0, 1, 15, 16, 31), lengths 1 .. 65, with bases behind it or ending on
    the read's last base; every rc piece (and every fourth forward one) has an N on both of its ends.  More than 150 calls."""
    rng = np.random.default_rng(seed)
    recs, calls, sigs, reads, claims = [], [], [], [], []
    for start in (0, 32, 33, 47, 48, 63):
        for ln in (1, 15, 16, 17, 63, 64, 65):
            for rev in (0, 1):
                for tail in ((5, 0) if start else (3,)):
                    q = len(reads)
                    qlen = start + ln + tail
                    s = rng.choice(list("ACGT"), qlen)
                    s[rng.random(qlen) < 0.08] = "N"
                    if rev or q % 4 == 0:
                        s[start] = "N"; s[start + ln - 1] = "N"
                    reads.append("".join(s))
                    left = (ln - 1) // 3; ins = max(1, ln // 3); right = ln - left - ins
                    cig = [(n, o) for n, o in ((left, "M"), (ins, "I"), (right, "M")) if n]
                    pos = 1000 * (q + 1)
                    recs.append(rec(q, qlen, start, start + ln, pos - left, pos + right, cig, flags=8 if rev else 0))
                    fwd_seg = start + (right if rev else left)
                    sigs.append(S(0, pos, ins, q, 0, q, -1, fwd_seg, ins))
                    calls.append(call(0, pos, ins, [q]))
                    claims.append(dict(start=start, len=ln, rc=rev, ends_on_last_base=tail == 0))
    return recs, calls, sigs, reads, claims


def many_candidates():
    """one call with 70 candidates (more than a wave holds), no two keys alike; read 69 alone has the call's length"""
    recs = [ins_rec(q, 1000 + q % 3, 90 - q // 3, 20 - q % 5, 20) for q in range(70)]
    return recs, [call(0, 1001, 67, list(range(70)))]


def random_reads(recs, calls=(), seed=3):
    """made-up reads of the records' lengths with some N; a read that only a call's supporter list names (no record) gets five bases"""
    rng = np.random.default_rng(seed)
    qlen = {}
    for r in recs:
        qlen[r["qid"]] = r["qlen"]
    last = max(list(qlen) + [q for c in calls for q in c["reads"]])
    out = []
    for q in range(last + 1):
        s = rng.choice(list("ACGTN"), qlen.get(q, 5), p=[0.24, 0.24, 0.24, 0.24, 0.04])
        out.append("".join(s))
    return out
