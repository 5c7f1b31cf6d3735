"""The definition of telr_genotype_insertions (include/telr_hip.h) as plain Python over records, CIGAR words and
calls: the checker of the device code, written for reading, not for speed."""

DEFAULTS = dict(flank=50, min_mapq=20, max_window_indel=20, het_pct=30, hom_pct=80)
GT_FIELDS = ("ref", "ambig", "alt", "gt")
F_SECONDARY = 2


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("no option %r" % k)
        o[k] = v
    return o


def spans(a, tid, pos, flank):
    return int(a["tid"]) == tid and int(a["ts"]) <= max(0, pos - flank) and int(a["te"]) >= pos + flank


def window_indel(a, cigars, pos, flank):
    """the I and D bases of record a inside [pos - flank, pos + flank]"""
    lo, hi = pos - flank, pos + flank
    p, total = int(a["ts"]), 0
    off = int(a["cigar_off"])
    words = cigars[off:off + int(a["n_cigar"])]
    for w in (words.tolist() if hasattr(words, "tolist") else words):
        op, n = w & 15, w >> 4
        if op == 0:
            p += n
        elif op == 1:
            if lo <= p <= hi:
                total += n
        elif op == 2:
            total += max(0, min(p + n, hi) - max(p, lo))
            p += n
        if p > hi:                  # nothing after this point can lie in the window (an I at p > hi does not count)
            break
    return total


def gt_of(alt, ref, het_pct, hom_pct):
    if 100 * alt >= hom_pct * (alt + ref):
        return 2
    if 100 * alt >= het_pct * (alt + ref):
        return 1
    return 0


def genotype(alns, cigars, calls, opt=None):
    """calls: dicts with tid, pos, support and reads (inscall_ref.calls gives them) -> one dict per call: GT_FIELDS, ref_reads and
    ambig_reads (ascending), and indels: {read: [window indel of every spanning record]} of the reads that are no supporters"""
    o = options(**(opt or {}))
    elig = [i for i in range(len(alns)) if not int(alns[i]["flags"]) & F_SECONDARY and int(alns[i]["mapq"]) >= o["min_mapq"]]
    out = []
    for c in calls:
        supporters = set(c["reads"])
        clean, indels = {}, {}
        for i in elig:
            a = alns[i]
            q = int(a["qid"])
            if q in supporters or not spans(a, c["tid"], c["pos"], o["flank"]):
                continue
            w = window_indel(a, cigars, c["pos"], o["flank"])
            indels.setdefault(q, []).append(w)
            clean[q] = clean.get(q, False) or w <= o["max_window_indel"]
        ref_reads = sorted(q for q, ok in clean.items() if ok)
        ambig_reads = sorted(q for q, ok in clean.items() if not ok)
        alt = c["support"]
        out.append(dict(ref=len(ref_reads), ambig=len(ambig_reads), alt=alt, gt=gt_of(alt, len(ref_reads), o["het_pct"], o["hom_pct"]),
                        ref_reads=ref_reads, ambig_reads=ambig_reads, indels=indels))
    return out
