"""The definitions of telr_seqset_join and telr_bridge_contigs (include/telr_hip.h) as plain Python over records, CIGAR
words, the calls and signatures of the insertion caller and the reads as strings: the checker of the device code, written for reading,
not for speed.  The bridge is not an assembler, and not wtdbg2 or flye: a read that enters the insertion from the left and one that enters
it from the right are joined at one shared k-mer; no consensus is formed."""
import draft_ref as dref

DEFAULTS = dict(flank=2000, min_flank=500, reach=50, max_len=100000, k=13, window=4096, min_votes=8, pairs=4)
BRIDGE_FIELDS = ("sig_l", "sig_r", "qid_l", "start_l", "len_l", "rc_l", "qid_r", "start_r", "len_r", "rc_r",
                 "votes", "diag", "ins_off", "ins_len", "n_left", "n_right")
BIN = 128
F_REV = 8


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("no option %r" % k)
        o[k] = v
    return o


def norm(s):
    """what the packed form holds of a string: A C G T (U reads as T), anything else N"""
    return "".join(ch.upper() if ch in "ACGTacgt" else ("T" if ch in "Uu" else "N") for ch in s)


# ---- telr_seqset_join ---------------------------------------------------------------------------------------------------------------
def join(seqs, piece_off, idx, start, length, rc=None):
    """sequence o = pieces piece_off[o] .. piece_off[o + 1] one after the other; a piece = bases [start, start + length) of seqs[idx],
    reverse-complemented where rc != 0 -> list of strings"""
    out = []
    for o in range(len(piece_off) - 1):
        s = ""
        for g in range(piece_off[o], piece_off[o + 1]):
            p = seqs[idx[g]][start[g]:start[g] + length[g]]
            s += dref.revcomp(p) if rc is not None and rc[g] else norm(p)
        out.append(s)
    return out


# ---- telr_bridge_contigs ------------------------------------------------------------------------------------------------------------
def strand_coords(a):
    """(qs', qe') of a record"""
    qlen, qs, qe = int(a["qlen"]), int(a["qs"]), int(a["qe"])
    return (qlen - qe, qlen - qs) if int(a["flags"]) & F_REV else (qs, qe)


def strand_bases(a, reads):
    """the read as record a aligns it"""
    s = reads[int(a["qid"])]
    return dref.revcomp(s) if int(a["flags"]) & F_REV else norm(s)


def left_candidate(alns, cigars, s, o):
    """the tail clip s of record a as a left candidate -> dict(clip, fl, lo, qe) or None"""
    a = alns[s["rec"]]
    if s["pos"] != int(a["te"]):
        return None
    qe = strand_coords(a)[1]
    cL = int(a["qlen"]) - qe
    xL = max(int(a["ts"]), s["pos"] - o["flank"])
    if int(a["n_cigar"]) == 0 or s["pos"] - xL < o["min_flank"] or cL < o["k"]:
        return None
    lh = dref.lo_hi(a, cigars, xL)
    if lh is None or lh[0] < 0:
        return None
    return dict(clip=cL, fl=s["pos"] - xL, lo=lh[0], qe=qe)


def right_candidate(alns, cigars, s, o):
    """the head clip s of record b as a right candidate -> dict(clip, fl, hi) or None"""
    b = alns[s["rec"]]
    if s["pos"] != int(b["ts"]):
        return None
    cR = strand_coords(b)[0]
    xR = min(int(b["te"]), s["pos"] + o["flank"])
    if int(b["n_cigar"]) == 0 or xR - s["pos"] < o["min_flank"] or cR < o["k"]:
        return None
    lh = dref.lo_hi(b, cigars, xR)
    if lh is None or lh[1] > int(b["qlen"]):
        return None
    return dict(clip=cR, fl=xR - s["pos"], hi=lh[1])


def matches(U, V, o):
    """the matches (i, j) of the vote, ascending by j: U the left read's clip, V the right read's"""
    k = o["k"]
    cL, cR = len(U), len(V)
    Wn = min(o["window"], cL)
    where = {}
    for i in range(cL - Wn, cL - k + 1):                  # the k-mers wholly inside the window
        w = U[i:i + k]
        if "N" not in w:
            where.setdefault(w, []).append(i)
    usable = {w: p[0] for w, p in where.items() if len(p) == 1}
    out = []
    for j in range(0, cR - k + 1):
        w = V[j:j + k]
        if "N" not in w and w in usable:
            out.append((usable[w], j))
    return out


def vote(U, V, o):
    """-> dict(votes, i, j, diag, n_matches, best_bin): votes 0 without a match (i = j = diag = 0)"""
    m = matches(U, V, o)
    if not m:
        return dict(votes=0, i=0, j=0, diag=0, n_matches=0, best_bin=None)
    count = {}
    for i, j in m:
        b = (i - j) // BIN                                # Python's // floors towards minus infinity
        count[b] = count.get(b, 0) + 1
    best = None
    for b in sorted(set(count) | set(x - 1 for x in count)):
        sc = count.get(b, 0) + count.get(b + 1, 0)
        if best is None or sc > best[0]:
            best = (sc, b)
    votes, bs = best
    band = [(i, j) for i, j in m if (i - j) // BIN in (bs, bs + 1)]
    assert len(band) == votes
    i, j = band[(len(band) - 1) // 2]                     # the lower median by j
    return dict(votes=votes, i=i, j=j, diag=i - j, n_matches=len(m), best_bin=bs)


NONE = dict(sig_l=-1, sig_r=-1, qid_l=0, start_l=0, len_l=0, rc_l=0, qid_r=0, start_r=0, len_r=0, rc_r=0, votes=0, diag=0, ins_off=0, ins_len=0)


def bridges(alns, cigars, calls, sigs, reads, opt=None, want=None):
    """calls: dicts with tid, pos, reads (inscall_ref.calls); sigs: the sorted signature dicts; reads: the read strings ->
    (list of dicts (BRIDGE_FIELDS + n_voted), list of the contigs' strings (None for a call without a bridge))"""
    o = options(**(opt or {}))
    out, seqs = [], []
    for kc, c in enumerate(calls):
        members = set(c["reads"])
        left, right = [], []
        for j, s in enumerate(sigs):
            if s["kind"] != 2 or s["tid"] != c["tid"] or abs(s["pos"] - c["pos"]) > o["reach"] or s["qid"] not in members:
                continue
            v = left_candidate(alns, cigars, s, o)
            if v is not None:
                left.append(((-v["clip"], -v["fl"], s["qid"], s["rec"], j), j, v))
            v = right_candidate(alns, cigars, s, o)
            if v is not None:
                right.append(((-v["clip"], -v["fl"], s["qid"], s["rec"], j), j, v))
        left.sort(key=lambda x: x[0]); right.sort(key=lambda x: x[0])
        d = dict(NONE, n_left=len(left), n_right=len(right), n_voted=0)
        out.append(d); seqs.append(None)
        if want is not None and not want[kc]:
            continue
        best = None
        for rl, (_, jl, vl) in enumerate(left[:o["pairs"]]):
            for rr, (_, jr, vr) in enumerate(right[:o["pairs"]]):
                if sigs[jl]["qid"] == sigs[jr]["qid"]:
                    continue
                a, b = alns[sigs[jl]["rec"]], alns[sigs[jr]["rec"]]
                U = strand_bases(a, reads)[vl["qe"]:]
                V = strand_bases(b, reads)[:vr["clip"]]
                v = vote(U, V, o)
                d["n_voted"] += 1
                if best is None or v["votes"] > best[0]["votes"]:          # ranks ascend: a tie keeps the smaller left rank, then right
                    best = (v, jl, vl, jr, vr)
        if best is None:
            continue
        v, jl, vl, jr, vr = best
        a, b = alns[sigs[jl]["rec"]], alns[sigs[jr]["rec"]]
        lo_l, hi_l = vl["lo"], vl["qe"] + v["i"]
        lo_r, hi_r = v["j"], vr["hi"]
        len_l, len_r = hi_l - lo_l, hi_r - lo_r
        if v["votes"] < o["min_votes"] or not 1 <= len_l + len_r <= o["max_len"]:
            continue
        rev_l, rev_r = (1 if int(a["flags"]) & F_REV else 0), (1 if int(b["flags"]) & F_REV else 0)
        d.update(sig_l=jl, sig_r=jr, qid_l=sigs[jl]["qid"], start_l=int(a["qlen"]) - hi_l if rev_l else lo_l, len_l=len_l, rc_l=rev_l,
                 qid_r=sigs[jr]["qid"], start_r=int(b["qlen"]) - hi_r if rev_r else lo_r, len_r=len_r, rc_r=rev_r,
                 votes=v["votes"], diag=v["diag"], ins_off=vl["qe"] - vl["lo"], ins_len=v["i"] + (vr["clip"] - v["j"]))
        seqs[-1] = join(reads, [0, 2], [d["qid_l"], d["qid_r"]], [d["start_l"], d["start_r"]], [d["len_l"], d["len_r"]], [rev_l, rev_r])[0]
    return out, seqs
