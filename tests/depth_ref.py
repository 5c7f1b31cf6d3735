"""telr_depth_medians in plain numpy: the definition the engine (k_depth_diff, the inclusive scan, k_depth_median) and the oracle
(tor_depth_medians) are held to at the edges of tests/depth_cases.py.  `samtools depth -aa -r | statistics.median` restated: the
depth of a position is the number of M columns of records that are not secondary; D advances the position without counting, I and
zero-length ops do nothing; a depth above 8,000 reads 8,000; an interval is clamped to [0, tlen - 1], an empty one gives NaN."""
import numpy as np

DEPTH_CAP = 8000
F_SECONDARY = 2


def depths(alns, cigars, tlens):
    """-> one int64 depth array per target (uncapped)"""
    d = [np.zeros(int(L), np.int64) for L in tlens]
    for a in alns:
        if int(a["flags"]) & F_SECONDARY:
            continue
        t = int(a["ts"])
        off = int(a["cigar_off"])
        for w in cigars[off:off + int(a["n_cigar"])]:
            op, l = int(w) & 0xf, int(w) >> 4
            if op == 0:
                np.add.at(d[int(a["tid"])], np.arange(t, t + l), 1)
                t += l
            elif op == 2:
                t += l
    return d


def depth_medians(alns, cigars, tlens, iv_tid, iv_s, iv_e):
    d = depths(alns, cigars, tlens)
    out = np.zeros(len(iv_tid), np.float64)
    for v, (tid, s, e) in enumerate(zip(iv_tid, iv_s, iv_e)):
        L = int(tlens[int(tid)])
        s, e = max(int(s), 0), min(int(e), L - 1)
        out[v] = np.nan if e < s else np.median(np.minimum(d[int(tid)][s:e + 1], DEPTH_CAP))
    return out
