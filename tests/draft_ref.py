"""The definition of telr_draft_contigs (include/telr_hip.h) as plain Python over records, CIGAR words, the calls and
signatures of the insertion caller and the reads as strings: the checker of the device code, written for reading, not for speed.
It is not an assembler: one supporting read per call is the backbone, a piece of it is the draft."""

DEFAULTS = dict(flank=2000, min_flank=500, reach=50, max_len=100000)
DRAFT_FIELDS = ("sig", "qid", "start", "len", "rc", "ins_off", "ins_len", "set_index")
F_REV = 8
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "T", "c": "G", "g": "C", "t": "A", "U": "A", "u": "A"}


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("no option %r" % k)
        o[k] = v
    return o


def revcomp(s):
    """what the packed form holds of the reverse complement: A C G T, anything else N"""
    return "".join(_COMP.get(c, "N") for c in reversed(s))


def strand_start(a):
    """qs' of a record"""
    return int(a["qlen"]) - int(a["qe"]) if int(a["flags"]) & F_REV else int(a["qs"])


def lo_hi(a, cigars, x):
    """(lo(x), hi(x)) of record a, or None when no state of its walk has p == x.  The walk is linear in the record: ops are run-length
    coded, so the states with p == x are found per op (an M or D of length l holds the coordinates p .. p + l)."""
    p, u = int(a["ts"]), strand_start(a)
    off = int(a["cigar_off"])
    words = cigars[off:off + int(a["n_cigar"])]
    lo = hi = None

    def see(v):
        nonlocal lo, hi
        lo = v if lo is None else min(lo, v)
        hi = v if hi is None else max(hi, v)

    if p == x:
        see(u)                                          # the start state
    for w in (words.tolist() if hasattr(words, "tolist") else words):
        op, l = w & 15, w >> 4
        if op == 0:                                     # M: (p + t, u + t), t = 1 .. l
            if p < x <= p + l:
                see(u + (x - p))
            p += l; u += l
        elif op == 1:                                   # I: one step to (p, u + l)
            u += l
            if p == x:
                see(u)
        elif op == 2:                                   # D: (p + t, u), t = 1 .. l
            if p < x <= p + l:
                see(u)
            p += l
        if p > x:
            break
    return None if lo is None else (lo, hi)


def candidate(alns, cigars, s, call, o):
    """the candidate signature s makes for `call` (membership and reach are the caller's to test) -> dict(lo, hi, fl) or None"""
    a = alns[s["rec"]]
    b = a if s["kind"] == 0 else alns[s["mate"]]
    lpos = s["pos"]
    rpos = s["pos"] if s["kind"] == 0 else int(b["ts"])
    xL = max(int(a["ts"]), lpos - o["flank"])
    xR = min(int(b["te"]), rpos + o["flank"])
    if int(a["n_cigar"]) == 0 or int(b["n_cigar"]) == 0:
        return None
    if lpos - xL < o["min_flank"] or xR - rpos < o["min_flank"]:
        return None
    left, right = lo_hi(a, cigars, xL), lo_hi(b, cigars, xR)
    if left is None or right is None:
        return None
    lo, hi = left[0], right[1]
    if not 1 <= hi - lo <= o["max_len"]:
        return None
    if lo < 0 or hi > int(a["qlen"]):
        return None
    return dict(lo=lo, hi=hi, fl=min(lpos - xL, xR - rpos))


def drafts(alns, cigars, calls, sigs, reads=None, opt=None):
    """calls: dicts with tid, pos, len, reads (inscall_ref.calls); sigs: the sorted signature dicts; reads: the read strings (None: no
    sequences) -> (list of dicts (DRAFT_FIELDS + n_candidates, n_valid), list of the drafts' strings in call order)"""
    o = options(**(opt or {}))
    out, seqs = [], []
    for c in calls:
        members = set(c["reads"])
        best = None
        n_cand = n_valid = 0
        for j, s in enumerate(sigs):
            if s["kind"] not in (0, 1) or s["tid"] != c["tid"] or abs(s["pos"] - c["pos"]) > o["reach"] or s["qid"] not in members:
                continue
            n_cand += 1
            v = candidate(alns, cigars, s, c, o)
            if v is None:
                continue
            n_valid += 1
            key = (abs(s["len"] - c["len"]), -v["fl"], s["qid"], s["rec"], s["mate"], j)
            if best is None or key < best[0]:
                best = (key, j, v)
        if best is None:
            out.append(dict(sig=-1, qid=0, start=0, len=0, rc=0, ins_off=0, ins_len=0, set_index=-1, n_candidates=n_cand, n_valid=n_valid))
            continue
        _, j, v = best
        s = sigs[j]
        a = alns[s["rec"]]
        qlen, rev = int(a["qlen"]), 1 if int(a["flags"]) & F_REV else 0
        lo, hi = v["lo"], v["hi"]
        seg = qlen - (s["seg_start"] + s["seg_len"]) if rev else s["seg_start"]          # the segment's strand coordinate
        d = dict(sig=j, qid=s["qid"], start=qlen - hi if rev else lo, len=hi - lo, rc=rev, ins_off=seg - lo, ins_len=s["seg_len"],
                 set_index=len(seqs), n_candidates=n_cand, n_valid=n_valid)
        out.append(d)
        if reads is not None:
            piece = reads[d["qid"]][d["start"]:d["start"] + d["len"]]
            seqs.append(revcomp(piece) if rev else "".join(ch.upper() if ch in "ACGTacgt" else ("T" if ch in "Uu" else "N") for ch in piece))
        else:
            seqs.append(None)
    return out, seqs
