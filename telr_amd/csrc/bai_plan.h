// bai_plan.h — the host side of the region load (behind telr_bai_plan and telr_bam_load_regions): the region normaliser,
// the .bai reader, reg2bins, the linear-index cut, and the sort and merge of the bins' chunks into intervals.  Plain C++: no HIP call and
// no type of the engine's own, so all of it is pinned on a CPU (tests/test_bam_region_ref.py against tests/bam_region_ref.py) and runs
// under the sanitizers from a stand-alone program (tools/ubench/bai_plan_host.cpp).
//
// Regions.  (tid, beg, end), 0-based, half-open, in any order, overlapping or touching.  `end` is clipped to the target's length where
// the lengths are known and to 2^29 (the reach of a .bai's bins) always; refused: a tid outside the targets, beg < 0, end <= beg after
// clipping, a non-zero reserved field.  They are sorted by (tid, beg) and merged where they overlap or touch.
//
// Index.  SAM specification 5.2: "BAI\1", n_ref, per reference { n_bin, per bin { bin, n_chunk, n_chunk x (beg, end) }, n_intv, n_intv x
// ioffset }, then optionally n_no_coor.  All offsets are virtual: coffset << 16 | uoffset.  Pseudo-bin 37450 is skipped.  Every count and
// every array is held to the file's end before it is read.
//
// Intervals.  Per merged region: the chunks of the bins of reg2bins(beg, end), without the empty ones (beg >= end) and without those that
// end at or below the linear index's entry for beg >> 14 (an entry of 0, or a window behind the last entry, drops nothing).  All regions'
// chunks are sorted by start; two neighbours become one interval when the next starts in, or before, the BGZF member in which the
// current one ends (coffset(next.beg) <= coffset(cur.end)).  So no member belongs to two intervals.
#ifndef TELR_BAI_PLAN_H
#define TELR_BAI_PLAN_H
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/telr_hip.h"

#define BAI_MAX_COOR   (1 << 29)      /* a .bai's bins reach this far */
#define BAI_PSEUDO_BIN 37450u

struct BaiRegion { int32_t tid, beg, end; };

// regions -> disjoint ascending regions per target.  tlens: nullable (no clip to the targets' lengths then)
static inline int bai_regions(int32_t n_ref, const int32_t *tlens, int64_t n_regions, const telr_region *regions, std::vector<BaiRegion> &out, std::string *why)
{
    auto bad = [&](const std::string &w) { if (why) *why = w; return TELR_E_ARG; };
    out.clear();
    if (n_regions < 0) return bad("a negative number of regions");
    if (n_regions > 0 && !regions) return bad("null regions");
    std::vector<BaiRegion> v;
    for (int64_t i = 0; i < n_regions; ++i) {
        const telr_region &r = regions[i];
        const std::string who = "region " + std::to_string(i);
        if (r.reserved != 0) return bad(who + ": the reserved field is not 0");
        if (r.tid < 0 || r.tid >= n_ref) return bad(who + ": tid outside the header's targets");
        if (r.beg < 0) return bad(who + ": beg below 0");
        int32_t end = std::min<int32_t>(r.end, BAI_MAX_COOR);
        if (tlens) end = std::min(end, tlens[r.tid]);
        if (end <= r.beg) return bad(who + ": end at or below beg" + (end != r.end ? " (after clipping to the target)" : ""));
        v.push_back(BaiRegion{r.tid, r.beg, end});
    }
    std::sort(v.begin(), v.end(), [](const BaiRegion &a, const BaiRegion &b) { return a.tid != b.tid ? a.tid < b.tid : a.beg != b.beg ? a.beg < b.beg : a.end < b.end; });
    for (const BaiRegion &r : v) {
        if (!out.empty() && out.back().tid == r.tid && r.beg <= out.back().end) out.back().end = std::max(out.back().end, r.end);
        else out.push_back(r);
    }
    return TELR_OK;
}

// the bins that may hold a record overlapping [beg, end), 0 <= beg < end <= 2^29 (SAM specification 5.3)
static inline void bai_reg2bins(int32_t beg, int32_t end, std::vector<uint32_t> &bins)
{
    bins.clear();
    --end;
    bins.push_back(0);
    for (int32_t k = 1 + (beg >> 26); k <= 1 + (end >> 26); ++k) bins.push_back((uint32_t)k);
    for (int32_t k = 9 + (beg >> 23); k <= 9 + (end >> 23); ++k) bins.push_back((uint32_t)k);
    for (int32_t k = 73 + (beg >> 20); k <= 73 + (end >> 20); ++k) bins.push_back((uint32_t)k);
    for (int32_t k = 585 + (beg >> 17); k <= 585 + (end >> 17); ++k) bins.push_back((uint32_t)k);
    for (int32_t k = 4681 + (beg >> 14); k <= 4681 + (end >> 14); ++k) bins.push_back((uint32_t)k);
}

struct BaiBin { uint32_t bin; int32_t n_chunk; size_t at; };      // at: where its chunks start in the file's bytes
struct BaiRef { std::vector<BaiBin> bins; size_t lin_at = 0; int32_t n_intv = 0; };

static inline uint32_t bai_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline uint64_t bai_ld64(const uint8_t *p) { return (uint64_t)bai_ld32(p) | (uint64_t)bai_ld32(p + 4) << 32; }

// the index's tables of contents; nothing beyond n bytes is read
static inline int bai_parse(const uint8_t *d, size_t n, int32_t n_ref, std::vector<BaiRef> &refs, std::string *why)
{
    auto bad = [&](const std::string &w) { if (why) *why = w; return TELR_E_ARG; };
    refs.clear();
    if (n < 8) return bad("the index is shorter than its magic and reference count");
    if (memcmp(d, "BAI\1", 4)) return bad("no BAI magic");
    const int32_t have = (int32_t)bai_ld32(d + 4);
    if (have != n_ref) return bad("the index holds " + std::to_string(have) + " references, the BAM's header " + std::to_string(n_ref));
    size_t p = 8;
    if ((uint64_t)n_ref * 8 > n - p) return bad("the references run past the index's end");      // (each holds two counts at the least)
    refs.resize((size_t)n_ref);
    for (int32_t t = 0; t < n_ref; ++t) {
        const std::string who = "reference " + std::to_string(t);
        if (n - p < 4) return bad(who + ": the bin count runs past the index's end");
        const int32_t n_bin = (int32_t)bai_ld32(d + p); p += 4;
        if (n_bin < 0 || (uint64_t)n_bin * 8 > n - p) return bad(who + ": the bins run past the index's end");
        BaiRef &R = refs[(size_t)t];
        R.bins.reserve((size_t)n_bin);
        for (int32_t b = 0; b < n_bin; ++b) {
            if (n - p < 8) return bad(who + ": a bin runs past the index's end");
            BaiBin B; B.bin = bai_ld32(d + p); B.n_chunk = (int32_t)bai_ld32(d + p + 4); p += 8;
            if (B.n_chunk < 0 || (uint64_t)B.n_chunk * 16 > n - p) return bad(who + ": the chunks of bin " + std::to_string(B.bin) + " run past the index's end");
            B.at = p; p += (size_t)B.n_chunk * 16;
            if (B.bin != BAI_PSEUDO_BIN) R.bins.push_back(B);
        }
        if (n - p < 4) return bad(who + ": the linear index's count runs past the index's end");
        R.n_intv = (int32_t)bai_ld32(d + p); p += 4;
        if (R.n_intv < 0 || (uint64_t)R.n_intv * 8 > n - p) return bad(who + ": the linear index runs past the index's end");
        R.lin_at = p; p += (size_t)R.n_intv * 8;
        std::stable_sort(R.bins.begin(), R.bins.end(), [](const BaiBin &a, const BaiBin &b) { return a.bin < b.bin; });
    }
    return TELR_OK;      // (n_no_coor, or nothing, follows)
}

// the intervals of merged regions over an index of n bytes: vbeg[i] < vend[i], ascending, no member in two of them
static inline int bai_plan(const uint8_t *d, size_t n, int32_t n_ref, const std::vector<BaiRegion> &merged, std::vector<uint64_t> &vbeg, std::vector<uint64_t> &vend, std::string *why)
{
    vbeg.clear(); vend.clear();
    std::vector<BaiRef> refs;
    const int rc = bai_parse(d, n, n_ref, refs, why);
    if (rc != TELR_OK) return rc;
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    std::vector<uint32_t> bins;
    for (const BaiRegion &r : merged) {
        if (r.tid < 0 || r.tid >= n_ref || r.beg < 0 || r.end <= r.beg || r.end > BAI_MAX_COOR) { if (why) *why = "a region outside the index's references or reach"; return TELR_E_ARG; }
        const BaiRef &R = refs[(size_t)r.tid];
        const int32_t w = r.beg >> 14;
        const uint64_t min_off = w < R.n_intv ? bai_ld64(d + R.lin_at + (size_t)w * 8) : 0;
        bai_reg2bins(r.beg, r.end, bins);
        for (uint32_t b : bins) {
            auto it = std::lower_bound(R.bins.begin(), R.bins.end(), b, [](const BaiBin &x, uint32_t v) { return x.bin < v; });
            for (; it != R.bins.end() && it->bin == b; ++it)
                for (int32_t c = 0; c < it->n_chunk; ++c) {
                    const uint64_t cb = bai_ld64(d + it->at + (size_t)c * 16), ce = bai_ld64(d + it->at + (size_t)c * 16 + 8);
                    if (cb >= ce || ce <= min_off) continue;
                    ch.emplace_back(cb, ce);
                }
        }
    }
    std::sort(ch.begin(), ch.end());
    for (const auto &c : ch) {
        if (!vbeg.empty() && (c.first >> 16) <= (vend.back() >> 16)) vend.back() = std::max(vend.back(), c.second);
        else { vbeg.push_back(c.first); vend.push_back(c.second); }
    }
    return TELR_OK;
}

// a file's bytes; TELR_E_IO when it cannot be read
static inline int bai_read_file(const char *path, std::vector<uint8_t> &out, std::string *why)
{
    out.clear();
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) { if (why) *why = std::string("cannot open the index ") + (path ? path : "(null)"); return TELR_E_IO; }
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + k);
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) { if (why) *why = std::string("cannot read the index ") + path; return TELR_E_IO; }
    return TELR_OK;
}

// what telr_bai_plan does: regions (not clipped to target lengths: it knows none) and an index file -> intervals
static inline int bai_plan_file(const char *bai_path, int32_t n_ref, int64_t n_regions, const telr_region *regions, uint64_t *vbeg, uint64_t *vend, int64_t cap,
                                int64_t *n_intervals, std::string *why)
{
    if (!n_intervals || cap < 0 || n_ref < 0 || (cap > 0 && (!vbeg || !vend))) { if (why) *why = "a null pointer or a negative count"; return TELR_E_ARG; }
    std::vector<BaiRegion> merged;
    int rc = bai_regions(n_ref, nullptr, n_regions, regions, merged, why);
    if (rc != TELR_OK) return rc;
    std::vector<uint8_t> bytes;
    if ((rc = bai_read_file(bai_path, bytes, why)) != TELR_OK) return rc;
    std::vector<uint64_t> b, e;
    if ((rc = bai_plan(bytes.data(), bytes.size(), n_ref, merged, b, e, why)) != TELR_OK) return rc;
    *n_intervals = (int64_t)b.size();
    for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t)b.size()); ++i) { vbeg[i] = b[(size_t)i]; vend[i] = e[(size_t)i]; }
    if ((int64_t)b.size() > cap) { if (why) *why = "more intervals than cap"; return TELR_E_RANGE; }
    return TELR_OK;
}
#endif /* TELR_BAI_PLAN_H */
