// part_plan.h — the host side of the multi-part index.  It holds three things: the one expression by which an index
// lays its targets out in global coordinates (index_extent_next, used by telr_index_build for `goff` and by the planner), how a target
// set is cut into parts that each fit an index (part_plan, behind telr_part_plan), and the checks telr_merge_parts makes on every
// record of every part before anything reaches the device (part_merge_check).  Plain C++: no HIP call and no type of the engine's own,
// so all of it is pinned on a CPU (tests/test_part_merge_ref.py) and runs under the sanitizers from a stand-alone program
// (tools/part_plan_check.cpp).
//
// Parts.  Contiguous runs of targets in target order, chosen greedily: a part's extent starts at 0 and advances target by target with
// index_extent_next; a target whose addition would make the extent REACH the limit starts the next part.  The limit is max_bases, 0
// meaning the engine's own (2^31: telr_index_build refuses an extent that reaches it), and never more than that.  Consequences: every
// part is accepted by the index rule, and no part would still be accepted with its successor's first target added.  A target that
// alone reaches the limit has no part: TELR_E_RANGE.
#ifndef TELR_PART_PLAN_H
#define TELR_PART_PLAN_H
#include <cstdint>
#include <string>
#include "../../include/telr_hip.h"

#define TELR_TPAD       16384                 /* padding between targets in global coordinates (tests/sketch_edges.py mirrors it: TPAD) */
#define PART_INDEX_LIMIT (1ULL << 31)         /* an index holds global coordinates below this */
#define PART_MAX_POOL   0x7ffffff0LL          /* 2^31 - 16 pooled records and more: TELR_E_RANGE */

// the global offset behind a target of `len` bases that starts at global offset g
static inline uint64_t index_extent_next(uint64_t g, uint64_t len) { return (g + len + TELR_TPAD + 63) & ~63ULL; }

// part_of[t] = the part of target t, *n_parts = their number; *why (nullable) = the reason of a refusal
static inline int part_plan(int32_t n_targets, const int32_t *target_len, int64_t max_bases, int32_t *part_of, int32_t *n_parts, std::string *why)
{
    auto fail = [&](int code, const std::string &w) { if (why) *why = w; return code; };
    if (n_targets < 0 || max_bases < 0 || !n_parts || (n_targets > 0 && (!target_len || !part_of))) return fail(TELR_E_ARG, "telr_part_plan: a null pointer or a negative argument");
    for (int32_t t = 0; t < n_targets; ++t) if (target_len[t] < 0) return fail(TELR_E_ARG, "telr_part_plan: target " + std::to_string(t) + " has a negative length");
    const uint64_t limit = max_bases == 0 || (uint64_t)max_bases > PART_INDEX_LIMIT ? PART_INDEX_LIMIT : (uint64_t)max_bases;
    int32_t part = 0; uint64_t g = 0; bool empty = true;
    for (int32_t t = 0; t < n_targets; ++t) {
        uint64_t g2 = index_extent_next(g, (uint64_t)target_len[t]);
        if (g2 >= limit && !empty) { ++part; g2 = index_extent_next(0, (uint64_t)target_len[t]); }
        if (g2 >= limit)
            return fail(TELR_E_RANGE, "telr_part_plan: target " + std::to_string(t) + " (" + std::to_string(target_len[t]) + " bases) alone reaches the limit of " +
                        std::to_string(limit) + " bases per part");
        part_of[t] = part; g = g2; empty = false;
    }
    *n_parts = n_targets > 0 ? part + 1 : 0;
    return TELR_OK;
}

// What telr_merge_parts refuses, checked on every record of every part before a kernel is launched: TELR_OK, or TELR_E_ARG /
// TELR_E_RANGE with the reason in *why.  Part p: alns[p][0 .. n[p]) with n_words[p] CIGAR words behind them, tid_map[p][0 .. n_pt[p]).
static inline int part_merge_check(int32_t n_parts, const telr_aln *const *alns, const int64_t *n, const int64_t *n_words, const int32_t *const *tid_map,
                                   const int32_t *n_pt, int32_t n_queries, std::string *why)
{
    auto bad = [&](const std::string &w) { *why = "telr_merge_parts: " + w; return TELR_E_ARG; };
    if (n_parts < 0 || n_queries < 0) return bad("a negative count");
    if (n_parts > 0 && (!alns || !n || !n_words || !tid_map || !n_pt)) return bad("a null pointer");
    int64_t pool = 0;
    for (int32_t p = 0; p < n_parts; ++p) {
        if (n[p] < 0 || n_words[p] < 0 || n_pt[p] < 0 || (n[p] > 0 && !alns[p]) || (n_pt[p] > 0 && !tid_map[p])) return bad("part " + std::to_string(p) + ": a null pointer or a negative count");
        pool += n[p];
        if (pool >= PART_MAX_POOL) { *why = "telr_merge_parts: too many records"; return TELR_E_RANGE; }
    }
    for (int32_t p = 0; p < n_parts; ++p) {
        const telr_aln *a = alns[p];
        for (int64_t i = 0; i < n[p]; ) {
            int64_t j = i;
            while (j < n[p] && a[j].qid == a[i].qid) ++j;
            for (int64_t k = i; k < j; ++k) {
                const telr_aln &r = a[k];
                const std::string who = "part " + std::to_string(p) + ", record " + std::to_string(k);
                if (r.qid < 0 || r.qid >= n_queries) return bad(who + ": qid outside n_queries");
                if (k > 0 && a[k - 1].qid > r.qid) return bad(who + ": the records are not ordered by qid");
                if (r.tid < 0 || r.tid >= n_pt[p]) return bad(who + ": tid outside the part's targets");
                if (r.n_cigar < 0 || r.cigar_off < 0 || (uint64_t)r.cigar_off + (uint64_t)r.n_cigar > (uint64_t)n_words[p]) return bad(who + ": CIGAR range outside the part's array");
                if (r.parent < 0 || r.parent >= j - i) return bad(who + ": parent outside the query's records");
                const int32_t cls = r.flags & (TELR_F_PRIMARY | TELR_F_SECONDARY | TELR_F_SUPPL);
                if (cls != TELR_F_PRIMARY && cls != TELR_F_SECONDARY && cls != TELR_F_SUPPL) return bad(who + ": flags without exactly one class bit");
            }
            i = j;
        }
    }
    return TELR_OK;
}
#endif /* TELR_PART_PLAN_H */
