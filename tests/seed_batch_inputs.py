"""Inputs of tests/test_gpu_seed_batch.py and tests/seed_batch_child.py: the key writer of the seeding routine (d_seed_query<1>) takes
SEED_PROBE_BATCH = 4 minimizers per thread and round and reads an occurrence list four occurrences at a time, so the inputs sit on the
edges of those groups.  Preset map-ont (k = 15, w = 10), seeded, cached, and every claim is checked here on the CPU (brute_minimizers
of tests/sketch_edges.py, numpy): no GPU and no oracle in this file.

  count_queries()    pieces of an 80-kb random genome trimmed to EXACT minimizer counts around the round of 256 threads x U
                     (COUNTS), and one 30-kb query for the 1,024-thread sort tier
  tile_queries(w)    queries whose minimizers of one thread and round fall into 1, 2, 3 and more 1,024-slot sketch tiles, with an
                     empty tile between (an all-N stretch) and with a run of empty tiles longer than the offsets read ahead
  family_case()      a 90-kb genome with repeat families planted in 1, 2, 3, 4, 5, 7, 8, 9 copies and one query per family
  home_slots(eh)     d_ht_slot of kernels.hip.h restated: the home slot of every index entry"""
import functools

import numpy as np

from telr_amd import synth
from telr_amd.presets import preset
import sketch_edges as SE

U = 4                    # SEED_PROBE_BATCH, the default the library is built with
NTHR = 256               # threads of k_seed (the fused sort fills with 64 .. 1,024)
TILE = SE.TILE
K, W = 15, 10
COUNTS = (0, 1, 255, 256, 257, 256 * U - 1, 256 * U, 256 * U + 1, 512 * U + 3)
FAMILY_COPIES = (1, 2, 3, 4, 5, 7, 8, 9)
FAMILY_LEN = 600
TILE_WIN = 8             # SEED_TILE_WIN: tile offsets a round reads ahead


def _s(a):
    return bytes(np.asarray(a, np.uint8)).decode()


@functools.lru_cache(maxsize=None)
def genome():
    return synth.random_seq(np.random.default_rng(20261101), 80_000)


def n_minimizers(seq, k=K, w=W):
    return len(SE.brute_minimizers(seq, k, w))


def _trim_to(seq, n):
    """the longest prefix of seq with exactly n (w,k)-minimizers"""
    if n == 0:
        return seq[:K - 1]
    full = SE.brute_minimizers(seq, K, W)
    assert len(full) > n
    # minimizer j ends at base y >> 1: a prefix that stops there no longer holds it.  A shorter prefix may also lose the window that
    # selected minimizer n - 1, so the count is checked and the prefix shortened until it fits.
    hi, lo = full[n][1] >> 1, (full[n - 1][1] >> 1) + 1
    for L in range(hi, lo - 1, -1):
        if n_minimizers(seq[:L]) == n:
            return seq[:L]
    raise AssertionError("no prefix with %d minimizers" % n)


@functools.lru_cache(maxsize=None)
def count_queries():
    """-> (targets, queries, counts): queries[i] has counts[i] minimizers; the last query is the long one"""
    g = genome()
    qs, cnt = [], []
    at = 1000
    for i, n in enumerate(COUNTS):
        piece = _s(g[at:at + 6 * n + 400])         # (~5.5 bases per minimizer)
        q = _trim_to(piece, n)
        at += 2500
        qs.append(q); cnt.append(n)
    rng = np.random.default_rng(20261102)
    long_q = _s(synth.mutate(rng, g[40_000:70_000], 0.002, 0.0005, 0.0005))
    qs.append(long_q); cnt.append(n_minimizers(long_q))
    for q, n in zip(qs, cnt):
        assert n_minimizers(q) == n
    assert tuple(cnt[:-1]) == COUNTS and cnt[-1] > 4096
    return [_s(g)], qs, cnt


def tiles_of(seq, k=K, w=W):
    """the sketch tile of every minimizer of a query: k-mer slot u = (y >> 1) - k + 1, tile u // 1,024"""
    return np.array([((y >> 1) - k + 1) // TILE for _, y in SE.brute_minimizers(seq, k, w)], np.int64)


def round_tile_counts(tiles, nthr=NTHR):
    """how many different tiles the live indices g = gb + tid + u * nthr (u < U) of one thread and round fall into, with the number of
    live indices: the set of (live, tiles) over all threads and rounds"""
    n = len(tiles)
    out = set()
    for gb in range(0, n, U * nthr):
        for tid in range(nthr):
            idx = [gb + tid + u * nthr for u in range(U) if gb + tid + u * nthr < n]
            if idx:
                out.add((len(idx), len(set(tiles[idx].tolist()))))
    return out


@functools.lru_cache(maxsize=None)
def tile_queries(w=W):
    """-> (targets, queries, tiles): tiles[i] = tiles_of(queries[i]).  Queries: one inside a single tile; 7 kb with bases 2,000 ..
    3,200 replaced by N (tile 2 holds nothing); 20 kb with 9,500 N (more empty tiles in a row than a round reads ahead); 13.5 kb plain"""
    g = genome()
    a = g[3000:3900]
    b = g[10_000:17_000].copy(); b[2000:3200] = ord("N")
    c = g[20_000:40_000].copy(); c[5000:14_500] = ord("N")
    d = g[45_000:58_500]
    qs = [_s(x) for x in (a, b, c, d)]
    tl = [tiles_of(q, K, w) for q in qs]
    assert set(tl[0].tolist()) == {0}
    assert 2 not in tl[1] and 1 in tl[1] and 3 in tl[1]
    gap = np.diff(np.unique(tl[2])).max() - 1
    assert gap > TILE_WIN, gap
    seen = set().union(*[round_tile_counts(t) for t in tl])
    if w == W:
        # ~190 minimizers a tile: four indices 256 apart lie in four tiles or more; the rounds at a query's end hold 1, 2, 3 live indices
        assert {(1, 1), (2, 2), (3, 3)} <= seen and any(nt >= 4 for _, nt in seen), seen
    else:
        # w = 1: every k-mer is a minimizer, ~1,000 a tile: all four indices of a thread in ONE tile, and in two
        assert {(4, 1), (4, 2)} <= seen, seen
    return [_s(g)], qs, tl


@functools.lru_cache(maxsize=None)
def family_case():
    """-> (targets3, queries, fams): a 90-kb genome cut into three targets; family i (FAMILY_LEN bases) planted FAMILY_COPIES[i]
    times on a 2,200-base grid in shuffled order, so that the copies of a family spread over the targets.  Query i runs across the first copy of
    family i with 300-base flanks, error-free, every second one reverse-complemented.  fams = the families' sequences."""
    rng = np.random.default_rng(20261103)
    g = synth.random_seq(rng, 90_000)
    fams = [synth.random_seq(rng, FAMILY_LEN) for _ in FAMILY_COPIES]
    owner = np.repeat(np.arange(len(FAMILY_COPIES)), FAMILY_COPIES)
    owner = owner[rng.permutation(len(owner))]
    first = {}
    for slot, f in enumerate(owner.tolist()):
        p = 1000 + slot * 2200
        g[p:p + FAMILY_LEN] = fams[f]
        first.setdefault(f, p)
    qs = []
    for f in range(len(FAMILY_COPIES)):
        q = g[first[f] - 300:first[f] + FAMILY_LEN + 300]
        qs.append(_s(synth.revcomp_arr(q) if f % 2 else q))
    cut = (29_100, 59_900)
    targets = [_s(g[:cut[0]]), _s(g[cut[0]:cut[1]]), _s(g[cut[1]:])]
    for c in cut:                                  # (no copy lies across a cut)
        assert all(not (1000 + s * 2200 - K < c < 1000 + s * 2200 + FAMILY_LEN + K) for s in range(len(owner)))
    return targets, qs, [_s(f) for f in fams]


def family_opts(cutoff):
    """map-ont with the occurrence cut-off clamped to at most `cutoff` (the upper clamp applies only above the lower one; the
    genome's own quantile lies above every family)"""
    io, mo = preset("map-ont")
    mo.min_mid_occ = 1; mo.max_mid_occ = cutoff
    return io, mo


def query_occurrences(index_hashes, query, k=K, w=W):
    """occurrence count in the index (its sorted per-occurrence hash array) of every minimizer of `query`"""
    qh = np.array([x >> 8 for x, _ in SE.brute_minimizers(query, k, w)], np.uint64)
    ih = np.asarray(index_hashes, np.uint64)
    return (np.searchsorted(ih, qh, side="right") - np.searchsorted(ih, qh, side="left")).astype(np.int64)


def home_slots(ent_hash):
    """d_ht_slot (telr_amd/csrc/kernels.hip.h) for a table of the size index_build_impl chooses: a power of two, at least 16 slots
    and at least twice the entries; slot = top bits of hash * 0x9E3779B97F4A7C15 mod 2^64"""
    eh = np.asarray(ent_hash, np.uint64)
    hb = 4
    while (1 << hb) < 2 * len(eh) and hb < 30:
        hb += 1
    with np.errstate(over="ignore"):
        return ((eh * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - hb)).astype(np.int64) & ((1 << hb) - 1)
