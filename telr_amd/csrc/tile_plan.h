// tile_plan.h — the host side of the reference TE annotation.  It holds two things: how a set of targets is cut into
// overlapping tiles (tile_plan, behind telr_tile_plan), and the argument checks telr_annotate_hits makes on its records, tiles and
// options before anything reaches the device (refte_check, on the C ABI's telr_aln / telr_tile / telr_refte_opt, with the reason as a
// std::string).  Plain C++: no HIP call and no type of the engine's own, so both are pinned on a CPU (tests/test_refte_ref.py) and
// run under the sanitizers from a stand-alone program (tools/refte_check.cpp).
//
// Tiles.  A target of length n gets no tile when n == 0, one tile when n <= tile, else 1 + ceil((n - tile) / stride) tiles; tile j
// is (tid, j * stride, min(tile, n - j * stride)); the tiles are listed in (tid, start) order.  Consequences: every interval of a
// target that is no longer than tile - stride + 1 bases lies whole inside at least one tile (an interval [a, b) with
// j = floor(a / stride), clamped to the last tile, starts at most stride - 1 bases into tile j, so it ends at most
// stride - 1 + tile - stride + 1 = tile bases into it -- and the last tile ends with the target); and no tile lies inside another
// (starts ascend by stride, and a tile shorter than `tile` is the last of its target, ending where the one before it cannot reach).
#ifndef TELR_TILE_PLAN_H
#define TELR_TILE_PLAN_H
#include <cstdint>
#include <string>
#include "../../include/telr_hip.h"

#define TILE_MAX_QUERY (1 << 24)             /* the query limit of telr_map: a tile is a query */
#define TILE_MAX_COUNT 0x7ffffff0LL           /* 2^31 - 16 tiles (or records) and more: TELR_E_RANGE */

// the number of tiles of a target of length n (arguments checked by the caller)
static inline int64_t tile_count(int64_t n, int64_t tile, int64_t stride)
{
    if (n == 0) return 0;
    if (n <= tile) return 1;
    return 1 + (n - tile + stride - 1) / stride;
}

// *needed = the number of tiles; when it exceeds cap nothing is copied and TELR_E_RANGE is returned: call again with cap >= *needed
static inline int tile_plan(int32_t n_targets, const int32_t *target_len, int32_t tile, int32_t stride, telr_tile *out, int64_t cap, int64_t *needed)
{
    if (n_targets < 0 || (n_targets > 0 && !target_len) || !needed || cap < 0 || (cap > 0 && !out)) return TELR_E_ARG;
    if (tile < 1 || tile >= TILE_MAX_QUERY || stride < 1 || stride > tile) return TELR_E_ARG;
    int64_t total = 0;
    for (int32_t t = 0; t < n_targets; ++t) if (target_len[t] < 0) return TELR_E_ARG;
    for (int32_t t = 0; t < n_targets; ++t) {
        total += tile_count(target_len[t], tile, stride);
        if (total >= TILE_MAX_COUNT) return TELR_E_RANGE;
    }
    *needed = total;
    if (total > cap) return TELR_E_RANGE;
    int64_t k = 0;
    for (int32_t t = 0; t < n_targets; ++t) {
        const int64_t n = target_len[t], c = tile_count(n, tile, stride);
        for (int64_t j = 0; j < c; ++j) {
            const int64_t s = j * stride;
            telr_tile &o = out[k++];
            o.tid = t; o.start = (int32_t)s; o.len = (int32_t)(n - s < tile ? n - s : tile);
        }
    }
    return TELR_OK;
}

// What telr_annotate_hits refuses, checked on every record (eligible or not) before a kernel is launched: TELR_OK, or TELR_E_ARG /
// TELR_E_RANGE with the reason in *why.  *max_end = the largest target length (the sort keys' coordinate bits).
static inline int refte_check(const telr_aln *alns, int64_t n, int64_t n_tiles, const telr_tile *tiles, int32_t n_targets, const int32_t *target_len,
                              int32_t n_families, const telr_refte_opt *O, int32_t *max_end, std::string *why)
{
    auto bad = [&](const std::string &w) { *why = w; return TELR_E_ARG; };
    if (n < 0 || (n > 0 && !alns)) return bad("null records");
    if (n_tiles < 0 || (n_tiles > 0 && !tiles)) return bad("null tiles");
    if (n_targets < 0 || (n_targets > 0 && !target_len)) return bad("null target lengths");
    if (n_families < 0) return bad("negative n_families");
    if (O->min_len < 0 || O->min_mapq < 0 || O->join_gap < 0 || O->reserved < 0) return bad("negative option");
    if (n >= TILE_MAX_COUNT) { *why = "too many records"; return TELR_E_RANGE; }
    if (n_tiles >= TILE_MAX_COUNT) { *why = "too many tiles"; return TELR_E_RANGE; }
    int32_t mx = 0;
    for (int32_t t = 0; t < n_targets; ++t) {
        if (target_len[t] < 0) return bad("target " + std::to_string(t) + ": negative length");
        if (target_len[t] > mx) mx = target_len[t];
    }
    for (int64_t k = 0; k < n_tiles; ++k) {
        const telr_tile &t = tiles[k];
        if (t.tid < 0 || t.tid >= n_targets || t.start < 0 || t.len < 0 || (int64_t)t.start + t.len > target_len[t.tid])
            return bad("tile " + std::to_string(k) + ": outside its target");
    }
    for (int64_t i = 0; i < n; ++i) {
        const telr_aln &a = alns[i];
        const std::string who = "record " + std::to_string(i);
        if (a.qid < 0 || a.qid >= n_tiles) return bad(who + ": qid outside the tiles");
        if (a.tid < 0 || a.tid >= n_families) return bad(who + ": tid outside n_families");
        if (a.qs < 0 || a.qe < a.qs) return bad(who + ": coordinates");
        if (a.qe > tiles[a.qid].len) return bad(who + ": qe beyond its tile");
    }
    *max_end = mx;
    return TELR_OK;
}
#endif /* TELR_TILE_PLAN_H */
