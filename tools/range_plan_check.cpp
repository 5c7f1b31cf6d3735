// The cases of tests/test_map_plan.py on range_plan.h alone, as a program of its own for a sanitizer build (the Python test
// loads the engine library, which a sanitizer does not see into):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/range_plan_check tools/range_plan_check.cpp && tools/range_plan_check
// Exit status 0 and "range plan: N cases ok" when every plan is the expected one.
#include <cstdio>
#include <string>
#include "../telr_amd/csrc/range_plan.h"

struct Case {
    const char *name;
    std::vector<std::pair<int32_t, int32_t>> runs;        // the read lengths as (count, length) runs
    double per_base; bool qtarget, vote; int debug; bool pipe_nomem;
    const char *mbp, *kbp, *pipeline;                     // the environment (null: unset)
    int mode; int64_t batch_bases; std::vector<int32_t> ends;
};

static std::vector<int32_t> steps(int32_t step, int32_t n) { std::vector<int32_t> v; for (int32_t e = step; e < n; e += step) v.push_back(e); v.push_back(n); return v; }
static void env(const char *k, const char *v) { if (v) setenv(k, v, 1); else unsetenv(k); }

int main()
{
    const int64_t ONE = 1600LL << 20;
    const int S = RANGE_SERIAL, T = RANGE_IN_TURN, W = RANGE_TWO;
    const std::vector<Case> cases = {
        { "500Mbp", {{5000, 100000}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, S, ONE, {5000} },
        { "700Mbp", {{5000, 140000}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, W, 350140001, {2501, 5000} },
        { "4Gbp", {{20000, 200000}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, W, 1000200001, {5001, 10002, 15003, 20000} },
        { "2.5Gbp", {{12500, 200000}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, W, 1250200001, {6251, 12500} },
        { "2.5Gbp vote", {{12500, 200000}}, 0.25, false, true, 0, false, nullptr, nullptr, nullptr, W, 625200001, {3126, 6252, 9378, 12500} },
        { "640Mi-1", {{4999, 134217}, {1, 137856}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, S, ONE, {5000} },
        { "640Mi", {{4999, 134217}, {1, 137857}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, W, 335682178, {2501, 5000} },
        { "3999 reads", {{3999, 200000}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, S, ONE, {3999} },
        { "4000 reads", {{4000, 200000}}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, W, 400200001, {2001, 4000} },
        { "debug", {{5000, 140000}}, 0.25, false, false, 1, false, nullptr, nullptr, nullptr, S, ONE, {5000} },
        { "pipe_nomem", {{5000, 140000}}, 0.25, false, false, 0, true, nullptr, nullptr, nullptr, S, ONE, {5000} },
        { "debug force", {{5000, 140000}}, 0.25, false, false, 1, false, nullptr, nullptr, "force", W, 350140001, {2501, 5000} },
        { "pipe_nomem force", {{5000, 140000}}, 0.25, false, false, 0, true, nullptr, nullptr, "force", S, ONE, {5000} },
        { "qtarget", {{5000, 140000}}, 0.25, true, false, 0, false, nullptr, nullptr, nullptr, T, 350140001, {2501, 5000} },
        { "qtarget force", {{5000, 140000}}, 0.25, true, false, 0, false, nullptr, nullptr, "force", W, 350140001, {2501, 5000} },
        { "qtarget 500Mbp", {{5000, 100000}}, 0.25, true, false, 0, false, nullptr, nullptr, nullptr, S, ONE, {5000} },
        { "pipeline=1", {{5000, 140000}}, 0.25, false, false, 0, false, nullptr, nullptr, "1", S, ONE, {5000} },
        { "pipeline=2", {{5000, 140000}}, 0.25, false, false, 0, false, nullptr, nullptr, "2", W, 350140001, {2501, 5000} },
        { "pipeline=2 3999", {{3999, 200000}}, 0.25, false, false, 0, false, nullptr, nullptr, "2", S, ONE, {3999} },
        { "force 3999", {{3999, 200000}}, 0.25, false, false, 0, false, nullptr, nullptr, "force", W, 400100001, {2000, 3999} },
        { "force tiny", {{10, 1000}}, 0.25, false, false, 0, false, nullptr, nullptr, "force", W, 6001, {6, 10} },
        { "kbp", {{100, 10000}}, 0.25, false, false, 0, false, nullptr, "60", nullptr, S, 61440, steps(6, 100) },
        { "kbp force", {{100, 10000}}, 0.25, false, false, 0, false, nullptr, "60", "force", W, 61440, steps(6, 100) },
        { "kbp force one range", {{100, 10000}}, 0.25, false, false, 0, false, nullptr, "2000", "force", S, 2048000, {100} },
        { "mbp", {{300, 10000}}, 0.25, false, false, 0, false, "1", nullptr, nullptr, S, 1048576, {104, 208, 300} },
        { "mbp 5000", {{5000, 10000}}, 8.0, false, false, 0, false, "1", nullptr, nullptr, W, 1048576, steps(104, 5000) },
        { "mbp+kbp", {{100, 10000}}, 0.25, false, false, 0, false, "1", "60", nullptr, S, 61440, steps(6, 100) },
        { "density unknown", {{5000, 140000}}, 0.0, false, false, 0, false, nullptr, nullptr, nullptr, W, 350140001, {2501, 5000} },
        { "density cap", {{5000, 200000}}, 2.0, false, false, 0, false, nullptr, nullptr, nullptr, W, 250200001, {1251, 2502, 3753, 5000} },
        { "density floor", {{5000, 240000}}, 8.0, false, false, 0, false, nullptr, nullptr, nullptr, W, 200240001, {834, 1668, 2502, 3336, 4170, 5000} },
        { "density splits", {{5000, 130000}}, 3.0, false, false, 0, false, nullptr, nullptr, nullptr, W, 162630001, {1251, 2502, 3753, 5000} },
        { "long read", {{1, 10000}, {1, 100000}, {2, 10000}}, 0.25, false, false, 0, false, nullptr, "60", nullptr, S, 61440, {1, 2, 4} },
        { "empty reads", {{2, 0}, {1, 30000}, {1, 0}, {1, 30000}, {1, 0}, {1, 1440}, {1, 0}, {1, 1}, {1, 0}}, 0.25, false, false, 0, false, nullptr, "60", nullptr, S, 61440, {8, 10} },
        { "all empty", {{5, 0}}, 0.25, false, false, 0, false, nullptr, "60", nullptr, S, 61440, {5} },
        { "n=0", {}, 0.25, false, false, 0, false, nullptr, nullptr, nullptr, S, ONE, {} },
        { "n=0 force", {}, 0.25, false, false, 0, false, nullptr, nullptr, "force", S, 1, {} },
    };
    int bad = 0;
    for (const Case &c : cases) {
        std::vector<int32_t> len; int32_t max_len = 0;
        for (auto &r : c.runs) { len.insert(len.end(), (size_t)r.first, r.second); max_len = std::max(max_len, r.second); }
        len.shrink_to_fit();                              // no slack behind the last read: a cut that reads past it is seen
        env("TELR_BATCH_MBP", c.mbp); env("TELR_BATCH_KBP", c.kbp); env("TELR_PIPELINE", c.pipeline);
        const RangePlan P = plan_ranges(len.empty() ? nullptr : len.data(), (int32_t)len.size(), max_len, c.per_base, c.qtarget, c.vote, c.debug, c.pipe_nomem);
        std::vector<int32_t> ends; int32_t at = 0; bool joined = true;
        for (auto &r : P.ranges) { joined = joined && r.first == at && r.second > r.first; at = r.second; ends.push_back(r.second); }
        if (P.mode != c.mode || P.batch_bases != c.batch_bases || ends != c.ends || !joined) {
            ++bad;
            fprintf(stderr, "%s: mode %d (want %d), batch_bases %lld (want %lld), %zu ranges (want %zu)\n", c.name, P.mode, c.mode, (long long)P.batch_bases, (long long)c.batch_bases, ends.size(), c.ends.size());
        }
    }
    if (bad) return 1;
    printf("range plan: %zu cases ok\n", cases.size());
    return 0;
}
