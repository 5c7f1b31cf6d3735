"""minimap2's high-occurrence seed rescue (TELR_MF_SEED_RESCUE = the oracle's 0x2000; seed.c: mm_seed_select) restated in numpy from
its definition, not from the engine:

  * the minimizers of one query in query order; occ[i] = occurrences of minimizer i in the index (0 = absent);
  * a stretch is a maximal run with occ > mid_occ;
  * ps = query position of the minimizer before the stretch (0 if the stretch opens the query), pe = that of the minimizer after it
    (qlen if it closes the query);
  * k = (int)((pe - ps) / 500.0 + .499);
  * the k minimizers of the stretch with the smallest occ among those with occ < 4095 are rescued, the earlier one on a tie (fewer
    if the stretch has fewer candidates); a rescued minimizer is seeded with all its occurrences."""
import numpy as np

DIST = 500
MAX_OCC = 4095
KEY_REV = 1 << 63


def k_float(d):
    """the definition: (int)(d / 500.0 + .499), in double precision as minimap2 computes it"""
    return int(float(d) / float(DIST) + .499)


def k_int(d):
    """the device's integer form"""
    return (1000 * int(d) + 249500) // 500000


def stretches(occ, mid_occ):
    """-> [(first, end)) of every maximal run with occ > mid_occ"""
    hi = np.asarray(occ, np.int64) > mid_occ
    out = []
    i, n = 0, len(hi)
    while i < n:
        if not hi[i]:
            i += 1
            continue
        j = i
        while j < n and hi[j]:
            j += 1
        out.append((i, j))
        i = j
    return out


def stretch_bounds(pos, qlen, s, e):
    """(ps, pe) of the stretch [s, e)"""
    return (int(pos[s - 1]) if s > 0 else 0), (int(pos[e]) if e < len(pos) else int(qlen))


def rescued(occ, pos, qlen, mid_occ):
    """-> ascending list of the rescued minimizers' indices.  occ, pos: per minimizer, in query order"""
    occ = np.asarray(occ, np.int64)
    out = []
    for s, e in stretches(occ, mid_occ):
        ps, pe = stretch_bounds(pos, qlen, s, e)
        k = k_float(pe - ps)
        cand = [i for i in range(s, e) if occ[i] < MAX_OCC]
        cand.sort(key=lambda i: (occ[i], i))
        out.extend(cand[:k])
    return sorted(out)


class IndexCounts:
    """occurrence lists of an oracle index (oracle.binding.OracleIndex.dump): hash -> (global position << 1 | strand) values"""

    def __init__(self, oix):
        h, y = oix.dump()
        o = np.argsort(h, kind="stable")
        self.h, self.y = h[o], y[o]

    def span_of(self, hashes):
        hashes = np.asarray(hashes, np.uint64)
        return np.searchsorted(self.h, hashes, "left"), np.searchsorted(self.h, hashes, "right")

    def occ(self, hashes):
        lo, hi = self.span_of(hashes)
        return (hi - lo).astype(np.int64)

    def hits(self, h):
        lo, hi = self.span_of([h])
        return self.y[lo[0]:hi[0]]


def query_minimizers(seq, k, w):
    """-> (hash, span, position, strand) arrays of the query's minimizers in query order (the oracle's sketch)"""
    from oracle import binding as ob
    x, y = ob.sketch(seq, k, w)
    return x >> np.uint64(8), (x & np.uint64(0xff)).astype(np.int64), (y >> 1).astype(np.int64), (y & 1).astype(np.int64)


def rescued_of_query(seq, io, counts, mid_occ):
    """-> (rescued indices, occ, pos) of one query against an index"""
    h, _, pos, _ = query_minimizers(seq, io.k, io.w)
    occ = counts.occ(h)
    return rescued(occ, pos, len(seq), mid_occ), occ, pos


def anchor_keys(seq, io, counts, which):
    """the anchor keys (the oracle's layout) of the minimizers `which` of a query, each with all its occurrences"""
    h, span, pos, strand = query_minimizers(seq, io.k, io.w)
    qlen = len(seq)
    out = []
    for i in which:
        for yy in counts.hits(h[i]):
            g, tz = int(yy) >> 1, int(yy) & 1
            if tz == int(strand[i]):
                out.append(g << 32 | int(pos[i]) << 8 | int(span[i]))
            else:
                out.append(KEY_REV | g << 32 | (qlen - (int(pos[i]) + 1 - int(span[i])) - 1) << 8 | int(span[i]))
    return np.array(sorted(out), np.uint64)
