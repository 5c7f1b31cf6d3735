"""The merge of a multi-part index in plain Python (include/telr_hip.h states the same definition): the twin of
telr_merge_parts, and the part planner's.  Integers throughout; the three float32 expressions of the engine's selection and its MAPQ
are evaluated operation by operation in numpy float32, the logarithm by the C library's logf (what the engine's host code calls).

A part is (alns, cigars): an ALN_DTYPE array ordered by qid and the uint32 CIGAR words its cigar_off index."""
import ctypes as C
import ctypes.util

import numpy as np

from telr_amd._abi import ALN_DTYPE, MF_MM2_MAPQ, MF_PER_TARGET

F_PRIMARY, F_SECONDARY, F_SUPPL, F_REV = 1, 2, 4, 8
CLASS = F_PRIMARY | F_SECONDARY | F_SUPPL
TPAD = 16384
INDEX_LIMIT = 1 << 31
f32 = np.float32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def logf(x):
    return f32(_libm.logf(float(f32(x))))


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def extent_next(g, n):
    """the global offset behind a target of n bases that starts at offset g (telr_index_build's layout)"""
    return (g + n + TPAD + 63) & ~63


def index_accepts(lengths, limit=INDEX_LIMIT):
    """would an index over these targets stay below `limit` (telr_index_build refuses an extent that reaches 2^31)"""
    g = 0
    for n in lengths:
        g = extent_next(g, n)
        if g >= limit:
            return False
    return True


def part_plan(lengths, max_bases=0):
    """-> part_of, one part number per target.  ValueError: a negative argument; OverflowError: a target that alone reaches the limit"""
    if max_bases < 0 or any(n < 0 for n in lengths):
        raise ValueError("negative argument")
    limit = INDEX_LIMIT if max_bases == 0 or max_bases > INDEX_LIMIT else max_bases
    part_of, part, g = [], 0, 0
    for t, n in enumerate(lengths):
        g2 = extent_next(g, n)
        if g2 >= limit and g > 0:
            part += 1
            g2 = extent_next(0, n)
        if g2 >= limit:
            raise OverflowError("target %d alone reaches the limit" % t)
        part_of.append(part)
        g = g2
    return part_of


# ---- the merge --------------------------------------------------------------------------------------------------------------------------
def mapq_of(r, mo):
    """the engine's MAPQ of a finished record (telr_engine.hip: mapq_of), either formula as TELR_MF_MM2_MAPQ says"""
    if not r["flags"] & (F_PRIMARY | F_SUPPL):
        return 0
    score, subsc, cnt = int(r["score"]), int(r["subsc"]), int(r["cnt"])
    pen_cm = f32(1.0) if cnt > 10 else f32(0.1) * f32(cnt)
    sub = f32(max(subsc, int(mo.min_chain_score)))
    with np.errstate(all="ignore"):
        if mo.flags & MF_MM2_MAPQ:
            pen_s1 = f32(1.0) if score > 100 else f32(0.01) * f32(score)
            if pen_s1 < pen_cm:
                pen_cm = pen_s1
            identity = f32(int(r["mlen"])) / f32(int(r["blen"])) if r["blen"] > 0 else f32(0.0)
            x = sub / f32(score)
            v = identity * pen_cm * f32(40.0) * (f32(1.0) - x) * logf(f32(int(r["dp_score"])) / f32(int(mo.a)))
            mq = _trunc(v) - _trunc(f32(4.343) * logf(f32(int(r["n_sub"])) + f32(1.0)) + f32(.499))
        else:
            x = sub / f32(score)
            if x > f32(1.0):
                x = f32(1.0)
            mq = _trunc(f32(40.0) * (f32(1.0) - x) * pen_cm * logf(f32(score)))
    return min(60, max(0, mq))


def _trunc(v):
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        return -(1 << 31)                 # what the conversion of the engine's host gives (x86: the integer indefinite value)
    return int(v)


def masks(qs_i, qe_i, qs_j, qe_j, mask_level):
    ol = max(0, min(qe_i, qe_j) - max(qs_i, qs_j))
    mn = min(qe_i - qs_i, qe_j - qs_j)
    return bool(f32(ol) > f32(mask_level) * f32(mn))


def check(parts, tid_maps, n_queries):
    """what telr_merge_parts refuses with TELR_E_ARG -> ValueError"""
    for p, (alns, cig) in enumerate(parts):
        q = alns["qid"].astype(np.int64)
        if len(q) and (q.min() < 0 or q.max() >= n_queries):
            raise ValueError("part %d: qid outside n_queries" % p)
        if (np.diff(q) < 0).any():
            raise ValueError("part %d: not ordered by qid" % p)
        per_q = np.bincount(q, minlength=max(n_queries, 1)) if len(q) else np.zeros(1, np.int64)
        for k, r in enumerate(alns):
            if not 0 <= r["tid"] < len(tid_maps[p]):
                raise ValueError("part %d record %d: tid" % (p, k))
            if r["n_cigar"] < 0 or r["cigar_off"] < 0 or int(r["cigar_off"]) + int(r["n_cigar"]) > len(cig):
                raise ValueError("part %d record %d: CIGAR range" % (p, k))
            if not 0 <= r["parent"] < per_q[r["qid"]]:
                raise ValueError("part %d record %d: parent" % (p, k))
            if int(r["flags"]) & CLASS not in (F_PRIMARY, F_SECONDARY, F_SUPPL):
                raise ValueError("part %d record %d: class bits" % (p, k))


def merge(parts, tid_maps, n_queries, mo):
    """parts: [(alns, cigars)], tid_maps: [part-local tid -> global tid] -> (alns, cigars) of the merged result"""
    if mo.flags & MF_PER_TARGET:
        raise ValueError("TELR_MF_PER_TARGET")
    check(parts, tid_maps, n_queries)
    pool = [[] for _ in range(n_queries)]                    # per query: (part, rank, index in the part)
    for p, (alns, _) in enumerate(parts):
        rank, last = 0, -1
        for k, q in enumerate(alns["qid"]):
            rank = rank + 1 if q == last else 0
            last = q
            pool[int(q)].append((p, rank, k))
    out, words = [], []
    n_words = 0
    for q in range(n_queries):
        recs = [(p, rank, parts[p][0][k]) for p, rank, k in pool[q]]
        recs.sort(key=lambda x: (-int(x[2]["dp_score"]), x[0], x[1]))
        n = len(recs)
        parent = list(range(n))
        subsc = [0 if r["flags"] & F_SECONDARY else int(r["subsc"]) for _, _, r in recs]
        n_sub = [0 if r["flags"] & F_SECONDARY else int(r["n_sub"]) for _, _, r in recs]
        for i in range(n):
            pi, _, ri = recs[i]
            for j in range(i):
                if parent[j] != j:
                    continue
                pj, rank_j, rj = recs[j]
                if masks(int(ri["qs"]), int(ri["qe"]), int(rj["qs"]), int(rj["qe"]), mo.mask_level):
                    parent[i] = j
                    if not (pi == pj and ri["flags"] & F_SECONDARY and int(ri["parent"]) == rank_j):
                        subsc[j] = max(subsc[j], int(ri["score"]))
                        n_sub[j] += 1
                    break
        keep, n_sec = [], 0
        for i in range(n):
            if parent[i] == i:
                keep.append(True)
                continue
            ok = bool(mo.secondary) and bool(f32(int(recs[i][2]["dp_score"])) >= f32(int(recs[parent[i]][2]["dp_score"])) * f32(mo.pri_ratio)) and n_sec < mo.best_n
            n_sec += ok
            keep.append(ok)
        new = {}
        for i in range(n):
            if keep[i]:
                new[i] = len(new)
        seen_primary = False
        for i in range(n):
            if not keep[i]:
                continue
            p, _, src = recs[i]
            r = src.copy()
            own = parent[i] == i
            cls = (F_SUPPL if seen_primary else F_PRIMARY) if own else F_SECONDARY
            seen_primary = seen_primary or own
            r["flags"] = (int(r["flags"]) & ~CLASS) | cls
            r["parent"] = new[parent[i]]
            r["subsc"] = subsc[i] if own else 0
            r["n_sub"] = n_sub[i] if own else 0
            r["tid"] = int(tid_maps[p][int(src["tid"])])
            r["cigar_off"] = n_words
            r["mapq"] = mapq_of(r, mo)
            o, c = int(src["cigar_off"]), int(src["n_cigar"])
            words.append(np.asarray(parts[p][1][o:o + c], np.uint32))
            n_words += c
            out.append(r)
    alns = np.array(out, dtype=ALN_DTYPE) if out else np.zeros(0, ALN_DTYPE)
    return alns, (np.concatenate(words) if words else np.zeros(0, np.uint32)).astype(np.uint32)


def records_equal(a, ca, b, cb):
    """every field and every record's CIGAR words (cigar_off itself may differ: a mapped result's array holds unreferenced words)"""
    if len(a) != len(b):
        return False
    for f in ALN_DTYPE.names:
        if f != "cigar_off" and not np.array_equal(a[f], b[f]):
            return False
    return all(np.array_equal(ca[int(x["cigar_off"]):int(x["cigar_off"]) + int(x["n_cigar"])],
                              cb[int(y["cigar_off"]):int(y["cigar_off"]) + int(y["n_cigar"])]) for x, y in zip(a, b))

