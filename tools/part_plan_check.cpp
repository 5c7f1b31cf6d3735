// telr_amd/csrc/part_plan.h alone -- the part planner of the multi-part index and the host checks of telr_merge_parts -- as a program of
// its own for a sanitizer build (the Python tests load the engine library, which a sanitizer does not see into):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/part_plan_check tools/part_plan_check.cpp && tools/part_plan_check
// The exact-fit boundaries, the greedy property by brute force (every part is accepted by the index rule, no part would be with its
// successor's first target added), the error codes, and every refusal of the record check.  Exit status 0 and "part_plan: N checks
// ok" when every one is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../telr_amd/csrc/part_plan.h"

static int n_checks = 0, n_bad = 0;
static void expect(const char *what, long long got, long long want)
{
    ++n_checks;
    if (got != want) { ++n_bad; fprintf(stderr, "%s: got %lld, want %lld\n", what, got, want); }
}

// the index rule on a run of targets: does the extent stay below `limit`
static bool accepts(const std::vector<int32_t> &len, size_t a, size_t b, uint64_t limit)
{
    uint64_t g = 0;
    for (size_t i = a; i < b; ++i) { g = index_extent_next(g, (uint64_t)len[i]); if (g >= limit) return false; }
    return true;
}

static std::vector<int32_t> plan(const std::vector<int32_t> &len, int64_t max_bases, int *code, int32_t *n_parts)
{
    std::vector<int32_t> part_of(len.size());                  // exactly n: a store past it is the sanitizer's to find
    std::string why;
    *n_parts = -7;
    *code = part_plan((int32_t)len.size(), len.data(), max_bases, part_of.data(), n_parts, &why);
    return part_of;
}

static telr_aln rec(int qid, int tid, int parent, int flags, int64_t off, int n)
{
    telr_aln a; memset(&a, 0, sizeof(a));
    a.qid = qid; a.tid = tid; a.parent = parent; a.flags = flags; a.cigar_off = off; a.n_cigar = n;
    return a;
}

int main()
{
    int code = 0; int32_t np = 0;
    // a target of n bases takes (n + 16384 + 63) & ~63 bases: 1,000 -> 17,408.  Limit 34,816 = two of them exactly: the second REACHES it
    expect("extent of 1000", (long long)index_extent_next(0, 1000), 17408);
    {
        std::vector<int32_t> p = plan({1000, 1000, 1000}, 34816, &code, &np);
        expect("exact fit code", code, TELR_OK); expect("exact fit parts", np, 3);
        p = plan({1000, 1000, 1000}, 34817, &code, &np);
        expect("one base more: parts", np, 2); expect("part of 1", p[1], 0); expect("part of 2", p[2], 1);
        p = plan({1000}, 17408, &code, &np);
        expect("alone reaches the limit", code, TELR_E_RANGE);
        p = plan({1000}, 17409, &code, &np);
        expect("alone below the limit", code, TELR_OK); expect("one part", np, 1);
        p = plan({1000, 5000, 1000}, 17409, &code, &np);
        expect("second target alone reaches the limit", code, TELR_E_RANGE);
    }
    // the engine's own limit: 2^31 - 16384 - 63 bases still fit (extent 2^31 - 64), one base more does not
    {
        plan({(int32_t)((1LL << 31) - 16384 - 64)}, 0, &code, &np);
        expect("largest single target", code, TELR_OK);
        plan({(int32_t)((1LL << 31) - 16384 - 63)}, 0, &code, &np);
        expect("one base more", code, TELR_E_RANGE);
        std::vector<int32_t> p = plan({1 << 30, 1 << 30, 1 << 30, 5}, 0, &code, &np);
        expect("3 Gbp: code", code, TELR_OK); expect("3 Gbp: parts", np, 3); expect("3 Gbp: last", p[3], 2);
        p = plan({1 << 30, 1 << 30, 1 << 30, 5}, (int64_t)1 << 40, &code, &np);
        expect("a limit above the engine's is the engine's", np, 3);
    }
    // the greedy property by brute force
    {
        const int64_t limits[] = {20000, 34816, 34817, 50000, 100000, 0};
        const std::vector<std::vector<int32_t>> sets = {{1000, 1000, 1000, 1000, 1000}, {0, 0, 0}, {3000, 1, 15000, 2, 2, 9000, 64, 63, 65}, {100}, {}};
        for (int64_t lim : limits)
            for (const auto &len : sets) {
                const uint64_t L = lim == 0 ? PART_INDEX_LIMIT : (uint64_t)lim;
                std::vector<int32_t> p = plan(len, lim, &code, &np);
                bool single = false;
                for (size_t i = 0; i < len.size(); ++i) if (!accepts(len, i, i + 1, L)) single = true;
                expect("code", code, single ? TELR_E_RANGE : TELR_OK);
                if (code != TELR_OK) continue;
                expect("count", np, len.empty() ? 0 : p.back() + 1);
                long long bad = 0;
                for (size_t a = 0; a < len.size(); ) {
                    size_t b = a;
                    while (b < len.size() && p[b] == p[a]) ++b;
                    if (a > 0 && p[a] != p[a - 1] + 1) ++bad;                        // contiguous runs, numbered in order
                    if (!accepts(len, a, b, L)) ++bad;                              // the part fits
                    if (b < len.size() && accepts(len, a, b + 1, L)) ++bad;         // and would not with its next target
                    a = b;
                }
                if (!len.empty() && p[0] != 0) ++bad;
                expect("greedy property", bad, 0);
            }
    }
    // error codes
    {
        const int32_t one[1] = {100}, neg[2] = {100, -1};
        int32_t out[2]; std::string why;
        expect("negative length", part_plan(2, neg, 0, out, &np, &why), TELR_E_ARG);
        expect("negative max_bases", part_plan(1, one, -1, out, &np, &why), TELR_E_ARG);
        expect("negative n", part_plan(-1, one, 0, out, &np, &why), TELR_E_ARG);
        expect("null lengths", part_plan(1, nullptr, 0, out, &np, &why), TELR_E_ARG);
        expect("null part_of", part_plan(1, one, 0, nullptr, &np, &why), TELR_E_ARG);
        expect("null n_parts", part_plan(1, one, 0, out, nullptr, &why), TELR_E_ARG);
        expect("null reason is fine", part_plan(1, one, 16000, out, &np, nullptr), TELR_E_RANGE);
        np = -7;
        expect("no targets", part_plan(0, nullptr, 0, nullptr, &np, &why), TELR_OK); expect("no parts", np, 0);
        const int32_t big[2] = {5, 100000};
        expect("the text names the target", part_plan(2, big, 50000, out, &np, &why) == TELR_E_RANGE && why.find("target 1") != std::string::npos, 1);
    }
    // the record check of telr_merge_parts: two parts, three queries
    {
        const int P = TELR_F_PRIMARY, S = TELR_F_SECONDARY, U = TELR_F_SUPPL, R = TELR_F_REV;
        const std::vector<telr_aln> a0 = {rec(0, 0, 0, P, 0, 3), rec(0, 1, 0, S | R, 3, 2), rec(2, 1, 0, P, 5, 0)}, a1 = {rec(1, 0, 0, P | R, 0, 4), rec(1, 0, 1, U, 4, 1)};
        const int32_t m0[2] = {0, 1}, m1[1] = {2};
        const int32_t *maps[2] = {m0, m1}; const int32_t npt[2] = {2, 1};
        std::string why;
        auto run = [&](const std::vector<telr_aln> &x0, const std::vector<telr_aln> &x1, int64_t w0, int64_t w1, int nq) {
            const telr_aln *al[2] = {x0.data(), x1.data()}; const int64_t n[2] = {(int64_t)x0.size(), (int64_t)x1.size()}, w[2] = {w0, w1};
            return part_merge_check(2, al, n, w, maps, npt, nq, &why);
        };
        expect("records ok", run(a0, a1, 5, 5, 3), TELR_OK);
        expect("an empty part", run(a0, {}, 5, 0, 3), TELR_OK);
        expect("no parts", part_merge_check(0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &why), TELR_OK);
        expect("qid = n_queries", run(a0, a1, 5, 5, 2), TELR_E_ARG);
        std::vector<telr_aln> b = a0; b[0].qid = -1;
        expect("qid -1", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a0; b[2].qid = 0; b[1].qid = 1;
        expect("not ordered by qid", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a0; b[1].tid = 2;
        expect("tid outside its map", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a1; b[0].tid = -1;
        expect("tid -1", run(a0, b, 5, 5, 3), TELR_E_ARG);
        expect("words beyond the array", run(a0, a1, 4, 5, 3), TELR_E_ARG);
        b = a0; b[1].n_cigar = -1;
        expect("negative n_cigar", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a0; b[1].cigar_off = -1;
        expect("negative cigar_off", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a0; b[2].parent = 1;
        expect("parent outside the query's records", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a1; b[1].parent = 2;
        expect("parent = count", run(a0, b, 5, 5, 3), TELR_E_ARG);
        b = a0; b[0].flags = P | U;
        expect("two class bits", run(b, a1, 5, 5, 3), TELR_E_ARG);
        b = a0; b[0].flags = R;
        expect("no class bit", run(b, a1, 5, 5, 3), TELR_E_ARG);
        { const telr_aln *al[2] = {a0.data(), a1.data()}; const int64_t n[2] = {0x40000000LL, 0x3ffffff0LL}, w[2] = {5, 5};
          expect("2^31 - 16 pooled records", part_merge_check(2, al, n, w, maps, npt, 3, &why), TELR_E_RANGE); }
        { const telr_aln *al[2] = {nullptr, a1.data()}; const int64_t n[2] = {3, 2}, w[2] = {5, 5};
          expect("null records", part_merge_check(2, al, n, w, maps, npt, 3, &why), TELR_E_ARG); }
    }
    if (n_bad) { fprintf(stderr, "part_plan: %d of %d checks FAILED\n", n_bad, n_checks); return 1; }
    printf("part_plan: %d checks ok\n", n_checks);
    return 0;
}
