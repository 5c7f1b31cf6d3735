"""The reference TE annotation in plain Python (include/telr_hip.h: telr_tile_plan, telr_annotate_hits): the checker of
tests/test_refte_ref.py and tests/test_gpu_refte.py.  Sequential code on Python lists; nothing here is shared with the engine.

  tile_plan(lengths, tile, stride)   -> [(tid, start, len)] in (tid, start) order
  hits(alns, tiles, opt)             -> [(tid, start, end, family, strand, score)] in record order
  features(hits, opt)                -> [(tid, start, end, family, strand, score, n_hits)] in (tid, start, end, family, strand) order

opt: a dict with min_len, min_mapq, join_gap (DEFAULTS).  What the engine refuses raises ValueError."""

DEFAULTS = dict(min_len=100, min_mapq=0, join_gap=0)
F_SECONDARY, F_REV = 2, 8


def tile_plan(lengths, tile, stride):
    if tile < 1 or stride < 1 or stride > tile or tile >= 1 << 24:
        raise ValueError("tile / stride")
    out = []
    for tid, n in enumerate(lengths):
        n = int(n)
        if n < 0:
            raise ValueError("negative length")
        if n == 0:
            continue
        if n <= tile:
            out.append((tid, 0, n))
            continue
        count = 1 + -(-(n - tile) // stride)
        for j in range(count):
            out.append((tid, j * stride, min(tile, n - j * stride)))
    return out


def hits(alns, tiles, opt=None):
    """alns: records with the fields of telr_aln (a structured array or dicts); tiles: [(tid, start, len)]"""
    o = dict(DEFAULTS, **(opt or {}))
    out = []
    for a in alns:
        qid, qs, qe = int(a["qid"]), int(a["qs"]), int(a["qe"])
        if qid < 0 or qid >= len(tiles):
            raise ValueError("qid outside the tiles")
        if qs < 0 or qe < qs:
            raise ValueError("coordinates")
        tid, t0, tlen = (int(x) for x in tiles[qid])
        if qe > tlen:
            raise ValueError("qe beyond its tile")
        if int(a["flags"]) & F_SECONDARY or int(a["mapq"]) < o["min_mapq"] or qe - qs < o["min_len"]:
            continue
        out.append((tid, t0 + qs, t0 + qe, int(a["tid"]), 1 if int(a["flags"]) & F_REV else 0, int(a["dp_score"])))
    return out


def features(hit_list, opt=None):
    """one sequential sweep over the hits in (tid, family, strand, start, end) order with a running maximum of end"""
    o = dict(DEFAULTS, **(opt or {}))
    feats = []
    run, m, cur = None, 0, None
    for tid, start, end, family, strand, score in sorted(hit_list, key=lambda h: (h[0], h[3], h[4], h[1], h[2])):
        if run != (tid, family, strand) or start >= m + o["join_gap"]:
            if cur is not None:
                feats.append(tuple(cur))
            cur = [tid, start, end, family, strand, score, 0]
            if run != (tid, family, strand):
                run, m = (tid, family, strand), end
        m = max(m, end)
        cur[2] = max(cur[2], end); cur[5] = max(cur[5], score); cur[6] += 1
    if cur is not None:
        feats.append(tuple(cur))
    return sorted(feats, key=lambda f: (f[0], f[1], f[2], f[3], f[4]))


def features_previous_end(hit_list, opt=None):
    """the WRONG rule -- the previous hit's end in place of the running maximum -- that the running-maximum case tells apart"""
    o = dict(DEFAULTS, **(opt or {}))
    n, run, prev = 0, None, 0
    for tid, start, end, family, strand, score in sorted(hit_list, key=lambda h: (h[0], h[3], h[4], h[1], h[2])):
        if run != (tid, family, strand) or start >= prev + o["join_gap"]:
            n += 1
        run, prev = (tid, family, strand), end
    return n
