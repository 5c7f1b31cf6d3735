// range_plan.h — how telr_map cuts a read set into ranges and how the ranges run.  Plain C++ on read lengths: no HIP call, no
// engine type, so the thresholds are pinned on a CPU (telr_debug_map_plan, tests/test_map_plan.py).
#ifndef TELR_RANGE_PLAN_H
#define TELR_RANGE_PLAN_H
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

enum { RANGE_SERIAL = 0,      // one range at a time, under a limit that follows the anchor density the call measures
       RANGE_IN_TURN = 1,     // per-query targets: ONE range when the device has room for it, else the plan's ranges in turn
       RANGE_TWO = 2 };       // two ranges in flight on two slots

struct RangePlan {
    int mode = RANGE_SERIAL;
    int64_t batch_bases = 0, total_bases = 0;
    bool fixed = false;                                          // the range size comes from the environment
    std::vector<std::pair<int32_t, int32_t>> ranges;             // [q0, q1) cut under batch_bases
};

// the end of the range that starts at q0 and holds at most `limit` bases (greedy; a read longer than the limit is a range of its own)
static inline int32_t range_cut(const int32_t *len, int32_t n, int32_t q0, int64_t limit)
{
    int32_t q1 = q0; int64_t b = 0;
    while (q1 < n && (q1 == q0 || b + len[q1] <= limit)) { b += len[q1]; ++q1; }
    return q1;
}

// TELR_BATCH_MBP / TELR_BATCH_KBP (tests) fix the range size: -> whether one is set; *batch_bases is left alone when none is
static inline bool range_size_from_env(int64_t *batch_bases)
{
    bool fixed = false;
    if (const char *e = getenv("TELR_BATCH_MBP")) { long v = atol(e); if (v > 0) { *batch_bases = (int64_t)v << 20; fixed = true; } }
    if (const char *e = getenv("TELR_BATCH_KBP")) { long v = atol(e); if (v > 0) { *batch_bases = (int64_t)v << 10; fixed = true; } }
    return fixed;
}

// the serial executor's limit at `per_base` anchors per read base: a range holds at most 1.6 G anchors (int32 offsets, ~50 B each)
static inline int64_t range_density_limit(int64_t batch_bases, double per_base)
{
    return std::min<int64_t>(batch_bases, std::max<int64_t>(256LL << 20, (int64_t)(1.6e9 / per_base)));
}

// Ranges bounded by bases: a read set of any size streams through as consecutive ranges.  HBM is 288 GB and a range
// needs ~75 B of scratch per read base at 0.25 anchors per base: a read set of up to 1.6 Gbp is ONE range (configs[2]
// reads alone in ranges of 0.5 / 1 / 1.4 / 2.1 Gbp: 13.7 / 14.9 / 15.3 / 15.5 Gbp/s -- fewer synchronisation points and
// tails; 151 GB in use at 2.1), a larger one is cut into ranges of at most 1.4 Gbp that run two at a time (the
// scratch of context and second slot is grow-only: ~115 + ~100 GB at this density).  What really bounds a range is its
// anchors: ranges hold at most 1.6 G anchors (0.8 G each when two are in flight) at the density the last call on the index
// has seen (`per_base`; before any call, an upper bound computed from the index's occurrence counts; 0: unknown) -- a range
// that overflows all the same is halved by map_range.  The environment is read per call.
static inline RangePlan plan_ranges(const int32_t *len, int32_t n, int32_t max_len, double per_base, bool has_qtarget, bool vote, int debug, bool pipe_nomem)
{
    RangePlan P;
    for (int32_t i = 0; i < n; ++i) P.total_bases += len[i];
    const int64_t total_bases = P.total_bases;
    int64_t batch_bases = 1600LL << 20;
    const bool fixed = range_size_from_env(&batch_bases);
    // Range pipelining: a read set that needs more than one range runs TWO ranges at a time on two slots (the context and
    // a second one of the same kind), so the host work between the stages of a range -- synchronisations, the second
    // selection pass, the record assembly -- and its latency-bound stretches are covered by the other range's kernels;
    // results are appended in range order through the turn gate of the result (round 2: configs[2] from 15.7 to 16.5-17.4 Gbp/s,
    // ranges of 0.7-1.6 Gbp: flat).  A read set that fits ONE range is halved when it holds 0.67 Gbp or more (below that the halves lose: 5-17 % at
    // 0.4-0.5 Gbp).  TELR_PIPELINE=1 switches it off; =force pipelines any multi-range call (tests).
    int pipe = 2; bool force = false;
    if (const char *e = getenv("TELR_PIPELINE")) { force = !strcmp(e, "force"); pipe = force || atoi(e) >= 2 ? 2 : 1; }
    // Round 6: a call with per-query targets (S6: every window read against the forward and the reverse-complement contig of its locus,
    // 0.75-0.9 Gbp; the polishing map) runs its ranges one at a time: it shares the device with the other calls of the loci pass already,
    // and on the hard genome its ranges are a few long chaining / sorting kernels on reads that bring 10^6 anchors each -- two in flight took
    // 0.96 or 1.45 s per 1,000 c2r loci from pass to pass, one at a time 0.89; configs[2]: 96 -> 90 ms (profiles/r06_chain_loop_choice_ab.txt, part 8).
    if (pipe_nomem || (!force && (debug || n < 4000))) pipe = 1;
    const bool in_turn = pipe == 2 && has_qtarget && !force;          // one range, or the ranges of the plan below in turn (no more scratch per range than two in flight took)
    if (pipe == 2 && !fixed) {
        // ranges of at most 1.4 Gbp (two in flight: ~200 GB of scratch at configs[2]'s anchor density) and at most 1.6 G
        // anchors at the density seen by the last call on this index; a read set within one such range is not split
        int64_t cap = 1400LL << 20;
        // sub-read voting carries ~25 B per query base more (hits staged at 8 B each, compacted minimizers): two 1.4-Gbp
        // ranges in flight fill the device (2 x 152 GB measured at configs[3]) and leave the BAM writer nothing
        if (vote) cap = 1100LL << 20;
        if (per_base > 0) cap = std::min<int64_t>(cap, std::max<int64_t>(256LL << 20, (int64_t)(0.8e9 / per_base)));      // two in flight: half the anchor budget each
        // ... or that is large enough for two halves in flight to win: measured on configs[2] reads, two ranges against one:
        // 0.40 Gbp 30.7 / 27.4 ms, 0.51 Gbp 32.9 / 33.9, 0.81 Gbp 47.2 / 51.3, 1.01 Gbp 57.3 / 63.2 (the shard of a 4-rank run)
        if (total_bases > std::min<int64_t>(batch_bases, (int64_t)(per_base > 0 ? 1.6e9 / per_base : 1e18)) || total_bases >= (640LL << 20) || force) {
            int64_t nr = std::max<int64_t>(2, (total_bases + cap - 1) / cap);
            nr += nr & 1;          // an even number of equal ranges keeps both slots busy to the end (configs[2]: 3 ranges 215 ms, 4 ranges 205 ms per step)
            batch_bases = (total_bases + nr - 1) / nr + max_len + 1;      // the slack keeps the greedy cut below from leaving a stub range behind
        } else pipe = 1;
    }
    for (int32_t q0 = 0; q0 < n; ) {
        const int32_t q1 = range_cut(len, n, q0, batch_bases);
        P.ranges.push_back(std::make_pair(q0, q1));
        q0 = q1;
    }
    P.mode = P.ranges.size() < 2 ? RANGE_SERIAL : in_turn ? RANGE_IN_TURN : pipe == 2 ? RANGE_TWO : RANGE_SERIAL;
    P.batch_bases = batch_bases; P.fixed = fixed;
    return P;
}
#endif /* TELR_RANGE_PLAN_H */
