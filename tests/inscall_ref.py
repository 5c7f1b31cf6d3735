"""The definition of telr_call_insertions (include/telr_hip.h) as plain Python over records and CIGAR words:
the checker of the device code, written for reading, not for speed."""

DEFAULTS = dict(min_len=50, min_mapq=20, min_clip=200, max_ref_gap=200, cluster_dist=50, min_support=10, min_sized=1)
SIG_FIELDS = ("tid", "pos", "len", "qid", "kind", "rec", "mate", "seg_start", "seg_len")
CALL_FIELDS = ("tid", "pos", "len", "support", "n_sized", "rep")
F_SECONDARY, F_REV = 2, 8


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError("no option %r" % k)
        o[k] = v
    return o


def _strand(a):
    """(qs', qe', reverse) of a record"""
    qlen, qs, qe = int(a["qlen"]), int(a["qs"]), int(a["qe"])
    if int(a["flags"]) & F_REV:
        return qlen - qe, qlen - qs, True
    return qs, qe, False


def _forward(qlen, rev, s, n):
    """bases [s, s + n) of the record's strand -> their start on the forward read"""
    return qlen - (s + n) if rev else s


def signatures(alns, cigars, opt=None):
    """-> list of dicts (SIG_FIELDS) sorted by (tid, pos, rec, kind, len, mate)"""
    o = options(**(opt or {}))
    elig = [i for i in range(len(alns)) if not int(alns[i]["flags"]) & F_SECONDARY and int(alns[i]["mapq"]) >= o["min_mapq"]]
    sigs = []

    def add(a, i, pos, ln, kind, mate, seg_start, seg_len):
        sigs.append(dict(tid=int(a["tid"]), pos=pos, len=ln, qid=int(a["qid"]), kind=kind, rec=i, mate=mate, seg_start=seg_start, seg_len=seg_len))

    for i in elig:
        a = alns[i]
        qlen, ts, te = int(a["qlen"]), int(a["ts"]), int(a["te"])
        qs, qe, rev = _strand(a)
        # intra: the I ops
        t, q = ts, qs
        off = int(a["cigar_off"])
        words = cigars[off:off + int(a["n_cigar"])]
        for w in (words.tolist() if hasattr(words, "tolist") else words):      # (plain ints: a numpy scalar per op is ten times slower)
            op, n = w & 15, w >> 4
            if op == 1 and n >= o["min_len"]:
                add(a, i, t, n, 0, -1, _forward(qlen, rev, q, n), n)
            if op == 0 or op == 2:
                t += n
            if op == 0 or op == 1:
                q += n
        # clips
        if qs >= o["min_clip"]:
            add(a, i, ts, qs, 2, -1, _forward(qlen, rev, 0, qs), qs)
        if qlen - qe >= o["min_clip"]:
            add(a, i, te, qlen - qe, 2, -1, _forward(qlen, rev, qe, qlen - qe), qlen - qe)
    # splits: every ordered pair of one query
    by_q = {}
    for i in elig:
        by_q.setdefault(int(alns[i]["qid"]), []).append(i)
    for recs in by_q.values():
        for i in recs:
            for j in recs:
                if i == j:
                    continue
                a, b = alns[i], alns[j]
                aqs, aqe, arev = _strand(a)
                bqs, bqe, brev = _strand(b)
                if int(a["tid"]) != int(b["tid"]) or arev != brev:
                    continue
                qgap, tgap = bqs - aqe, int(b["ts"]) - int(a["te"])
                if qgap >= 0 and abs(tgap) <= o["max_ref_gap"] and qgap - tgap >= o["min_len"]:
                    add(a, i, int(a["te"]), qgap - tgap, 1, j, _forward(int(a["qlen"]), arev, aqe, qgap), qgap)
    sigs.sort(key=lambda s: (s["tid"], s["pos"], s["rec"], s["kind"], s["len"], s["mate"]))
    return sigs


def lower_median_index(n):
    return (n - 1) // 2


def calls(sigs, opt=None):
    """sorted signatures -> list of dicts (CALL_FIELDS + reads: the ascending distinct read ids)"""
    o = options(**(opt or {}))
    clusters, cur = [], []
    for k, s in enumerate(sigs):
        if cur and (sigs[cur[-1]]["tid"] != s["tid"] or s["pos"] - sigs[cur[-1]]["pos"] > o["cluster_dist"]):
            clusters.append(cur)
            cur = []
        cur.append(k)
    if cur:
        clusters.append(cur)
    out = []
    for cl in clusters:
        reads = sorted(set(sigs[k]["qid"] for k in cl))
        sized = [k for k in cl if sigs[k]["kind"] != 2]
        n_sized = len(set(sigs[k]["qid"] for k in sized))
        if len(reads) < o["min_support"] or n_sized < o["min_sized"]:
            continue
        pos = sigs[cl[lower_median_index(len(cl))]]["pos"]
        if sized:
            order = sorted(sized, key=lambda k: (sigs[k]["len"], sigs[k]["qid"], sigs[k]["rec"], sigs[k]["mate"]))
            rep = order[lower_median_index(len(order))]
            ln = sigs[rep]["len"]
        else:
            rep, ln = -1, 0
        out.append(dict(tid=sigs[cl[0]]["tid"], pos=pos, len=ln, support=len(reads), n_sized=n_sized, rep=rep, reads=reads))
    return out


def call_insertions(alns, cigars, opt=None):
    s = signatures(alns, cigars, opt)
    return s, calls(s, opt)
