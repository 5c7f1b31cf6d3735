"""The definition of telr_call_at_sites (include/telr_hip.h) as plain Python over records, CIGAR words and sites: the
checker of the device code, written for reading, not for speed.  The signatures are inscall_ref's; a site is (tid, pos, len)."""
import bisect

import inscall_ref as iref

SITE_DEFAULTS = dict(reach=50, len_pct=0)
E_ARG, E_RANGE = -3, -4
MAX_SITES = (1 << 31) - 16


class _Keyed(list):
    """a site list with its (tid, pos) keys made once"""
    def __init__(self, sites):
        list.__init__(self, (tuple(int(v) for v in s) for s in sites))
        self.keys = [s[:2] for s in self]


def site_options(**kw):
    o = dict(SITE_DEFAULTS)
    for k, v in kw.items():
        if k not in o and k not in ("reserved0", "reserved1"):
            raise TypeError("no site option %r" % k)
        o[k] = v
    return o


def refusal(alns, n_cigar_words, n_targets, sites, opt=None, site_opt=None, n_sites=None):
    """-> None, or (code, reason) of the first thing telr_call_at_sites refuses, in its order: n_targets, the signature options it
    reads, the records, the site options, the site count (n_sites: a count other than len(sites)), the sites"""
    o = iref.options(**(opt or {}))
    so = site_options(**(site_opt or {}))
    if n_targets <= 0:
        return E_ARG, "n_targets must be positive"
    if any(o[k] < 0 for k in ("min_len", "min_mapq", "min_clip", "max_ref_gap")):      # min_support, min_sized, cluster_dist are not read
        return E_ARG, "negative option"
    for i, a in enumerate(alns):
        tid, qid, qlen, qs, qe, ts, te = (int(a[f]) for f in ("tid", "qid", "qlen", "qs", "qe", "ts", "te"))
        if tid < 0 or tid >= n_targets:
            return E_ARG, "record %d: tid outside n_targets" % i
        if qid < 0 or qlen < 0 or qs < 0 or qe < qs or qe > qlen or ts < 0 or te < ts:
            return E_ARG, "record %d: coordinates" % i
        if int(a["n_cigar"]) < 0 or int(a["cigar_off"]) < 0 or int(a["cigar_off"]) + int(a["n_cigar"]) > n_cigar_words:
            return E_ARG, "record %d: CIGAR range outside the result's array" % i
    if so["reach"] < 0:
        return E_ARG, "negative reach"
    if not 0 <= so["len_pct"] <= 100:
        return E_ARG, "len_pct outside 0..100"
    if so.get("reserved0", 0) or so.get("reserved1", 0):
        return E_ARG, "non-zero reserved field"
    n = len(sites) if n_sites is None else n_sites
    if n < 0:
        return E_ARG, "negative n_sites"
    if n > 0 and sites is None:
        return E_ARG, "null sites"
    if n >= MAX_SITES:
        return E_RANGE, "too many sites"
    for c, (tid, pos, ln) in enumerate(sites):
        if tid < 0 or tid >= n_targets:
            return E_ARG, "site %d: tid outside n_targets" % c
        if pos < 0:
            return E_ARG, "site %d: negative pos" % c
        if ln < 0:
            return E_ARG, "site %d: negative len" % c
        if c > 0 and (tid, pos) <= tuple(sites[c - 1][:2]):
            return E_ARG, "site %d: sites not strictly ascending by (tid, pos)" % c
    return None


def assign(s, sites, so):
    """the site index signature s is kept at, or -1: the nearest site within reach on its target, the smaller index on equal distance,
    then the length test at THAT site (a signature it rejects is not offered to another)"""
    # every site near s: those with (tid, pos) in [(s.tid, s.pos - reach), (s.tid, s.pos + reach)], a run of the ascending list
    keys = sites.keys if isinstance(sites, _Keyed) else [tuple(c[:2]) for c in sites]
    near = range(bisect.bisect_left(keys, (s["tid"], s["pos"] - so["reach"])), bisect.bisect_right(keys, (s["tid"], s["pos"] + so["reach"])))
    best = min(near, key=lambda c: (abs(s["pos"] - sites[c][1]), c), default=-1)
    if best >= 0 and s["kind"] != 2 and so["len_pct"] > 0 and sites[best][2] > 0:
        if 100 * abs(s["len"] - sites[best][2]) > so["len_pct"] * sites[best][2]:
            return -1
    return best


def calls_at_sites(sigs, sites, site_opt=None):
    """sorted signatures (inscall_ref.signatures), sites [(tid, pos, len), ...] strictly ascending -> (the kept signatures in their
    sorted order, one dict per site: inscall_ref.CALL_FIELDS + reads; rep indexes the kept signatures)"""
    so = site_options(**(site_opt or {}))
    sites = _Keyed(sites)
    kept, runs = [], [[] for _ in sites]
    for s in sigs:
        c = assign(s, sites, so)
        if c >= 0:
            runs[c].append(len(kept))
            kept.append(s)
    out = []
    for c, (tid, pos, _) in enumerate(sites):
        mine = runs[c]
        reads = sorted(set(kept[k]["qid"] for k in mine))
        sized = [k for k in mine if kept[k]["kind"] != 2]
        if sized:
            order = sorted(sized, key=lambda k: (kept[k]["len"], kept[k]["qid"], kept[k]["rec"], kept[k]["mate"]))
            rep = order[iref.lower_median_index(len(order))]
            ln = kept[rep]["len"]
        else:
            rep, ln = -1, 0
        out.append(dict(tid=tid, pos=pos, len=ln, support=len(reads), n_sized=len(set(kept[k]["qid"] for k in sized)), rep=rep, reads=reads))
    return kept, out


def call_at_sites(alns, cigars, sites, opt=None, site_opt=None):
    return calls_at_sites(iref.signatures(alns, cigars, opt), sites, site_opt)
