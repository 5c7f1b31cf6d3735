// telr_amd/csrc/tile_plan.h alone -- the tile plan and the host checks of telr_annotate_hits -- as a program of its own for a sanitizer
// build (the Python tests load the engine library, which a sanitizer does not see into):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/refte_check tools/refte_check.cpp && tools/refte_check
// The plans against tiles written out by hand and against the covering property by brute force, the error codes, and every refusal of
// the record check.  Exit status 0 and "refte: N checks ok" when every one is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../telr_amd/csrc/tile_plan.h"

static int n_checks = 0, n_bad = 0;
static void expect(const char *what, long long got, long long want)
{
    ++n_checks;
    if (got != want) { ++n_bad; fprintf(stderr, "%s: got %lld, want %lld\n", what, got, want); }
}

static std::vector<telr_tile> plan(const std::vector<int32_t> &len, int32_t tile, int32_t stride, int *code)
{
    int64_t need = -1;
    *code = tile_plan((int32_t)len.size(), len.data(), tile, stride, nullptr, 0, &need);
    std::vector<telr_tile> out;
    if (*code != TELR_E_RANGE || need <= 0) return out;
    out.resize((size_t)need);                                 // exactly `needed`: a store past it is the sanitizer's to find
    *code = tile_plan((int32_t)len.size(), len.data(), tile, stride, out.data(), need, &need);
    return out;
}

static telr_aln rec(int qid, int qs, int qe, int family)
{
    telr_aln a; memset(&a, 0, sizeof(a));
    a.qid = qid; a.qs = qs; a.qe = qe; a.tid = family; a.flags = TELR_F_PRIMARY;
    return a;
}

int main()
{
    int code = 0;
    // 100 bases, tile 48, stride 16: 1 + ceil(52 / 16) = 5 tiles, the last one the 36 bases from 64 on
    {
        const std::vector<telr_tile> t = plan({100}, 48, 16, &code);
        expect("100/48/16 code", code, TELR_OK); expect("100/48/16 count", (long long)t.size(), 5);
        const int want[5][3] = {{0, 0, 48}, {0, 16, 48}, {0, 32, 48}, {0, 48, 48}, {0, 64, 36}};
        for (size_t k = 0; k < t.size() && k < 5; ++k) { expect("tid", t[k].tid, want[k][0]); expect("start", t[k].start, want[k][1]); expect("len", t[k].len, want[k][2]); }
    }
    {
        const std::vector<telr_tile> t = plan({0, 48, 49}, 48, 16, &code);
        expect("0,48,49 count", (long long)t.size(), 3);
        if (t.size() == 3) { expect("tid", t[0].tid, 1); expect("tid", t[2].tid, 2); expect("start", t[2].start, 16); expect("len", t[2].len, 33); }
    }
    // the covering property and "no tile inside another", by brute force
    const int pairs[3][2] = {{48, 16}, {40, 40}, {37, 11}};
    for (const auto &p : pairs) {
        const int tile = p[0], stride = p[1];
        const int lens[] = {0, 1, stride - 1, stride, stride + 1, tile - 1, tile, tile + 1, tile + stride, tile + stride + 1, 3 * tile + 5};
        for (int n : lens) {
            const std::vector<telr_tile> t = plan({n}, tile, stride, &code);
            expect("plan code", code, TELR_OK);
            long long uncovered = 0, nested = 0;
            for (int a = 0; a < n; ++a)
                for (int b = a + 1; b <= n && b - a <= tile - stride + 1; ++b) {
                    bool in = false;
                    for (const telr_tile &x : t) if (x.start <= a && b <= x.start + x.len) in = true;
                    if (!in) ++uncovered;
                }
            for (size_t i = 0; i < t.size(); ++i)
                for (size_t j = 0; j < t.size(); ++j)
                    if (i != j && t[j].start <= t[i].start && t[i].start + t[i].len <= t[j].start + t[j].len) ++nested;
            expect("uncovered intervals", uncovered, 0); expect("nested tiles", nested, 0);
            if (!t.empty()) expect("last tile ends with the target", t.back().start + t.back().len, n);
        }
    }
    // error codes
    {
        const int32_t one[1] = {100}, neg[2] = {100, -1}, big[1] = {0x7fffffff};
        telr_tile out[8]; int64_t need = -1;
        expect("tile 0", tile_plan(1, one, 0, 1, out, 8, &need), TELR_E_ARG);
        expect("stride 0", tile_plan(1, one, 48, 0, out, 8, &need), TELR_E_ARG);
        expect("stride > tile", tile_plan(1, one, 48, 49, out, 8, &need), TELR_E_ARG);
        expect("tile 2^24", tile_plan(1, one, 1 << 24, 16, out, 8, &need), TELR_E_ARG);
        expect("negative length", tile_plan(2, neg, 48, 16, out, 8, &need), TELR_E_ARG);
        expect("null lengths", tile_plan(1, nullptr, 48, 16, out, 8, &need), TELR_E_ARG);
        expect("null needed", tile_plan(1, one, 48, 16, out, 8, nullptr), TELR_E_ARG);
        expect("null out", tile_plan(1, one, 48, 16, nullptr, 8, &need), TELR_E_ARG);
        expect("cap too small", tile_plan(1, one, 48, 16, out, 4, &need), TELR_E_RANGE); expect("needed", need, 5);
        expect("2^31 - 1 tiles", tile_plan(1, big, 1, 1, nullptr, 0, &need), TELR_E_RANGE);
        expect("no targets", tile_plan(0, nullptr, 48, 16, nullptr, 0, &need), TELR_OK); expect("needed", need, 0);
    }
    // the record check of telr_annotate_hits: the tiles of a 10,000-base target (tile 4,096, stride 2,048)
    {
        const std::vector<telr_tile> tiles = plan({10000}, 4096, 2048, &code);
        expect("10000/4096/2048 count", (long long)tiles.size(), 4);
        const int32_t tl[1] = {10000};
        telr_refte_opt O = {100, 0, 0, 0};
        std::vector<telr_aln> ok = {rec(3, 3000, 3856, 0), rec(1, 2100, 2552, 0), rec(2, 52, 504, 0)};
        int32_t mx = 0; std::string why;
        auto run = [&](const std::vector<telr_aln> &a, const std::vector<telr_tile> &t, const int32_t *len, int32_t nfam, const telr_refte_opt &o) {
            return refte_check(a.data(), (int64_t)a.size(), (int64_t)t.size(), t.data(), 1, len, nfam, &o, &mx, &why);
        };
        expect("records ok", run(ok, tiles, tl, 1, O), TELR_OK); expect("max_end", mx, 10000);
        expect("no records", refte_check(nullptr, 0, (int64_t)tiles.size(), tiles.data(), 1, tl, 1, &O, &mx, &why), TELR_OK);
        telr_refte_opt neg = O; neg.join_gap = -1;
        expect("negative option", run(ok, tiles, tl, 1, neg), TELR_E_ARG);
        std::vector<telr_aln> a = ok; a[0].qid = 4;
        expect("qid = n_tiles", run(a, tiles, tl, 1, O), TELR_E_ARG);
        a = ok; a[1].qid = -1;
        expect("qid -1", run(a, tiles, tl, 1, O), TELR_E_ARG);
        a = ok; a[2].tid = 1;
        expect("family = n_families", run(a, tiles, tl, 1, O), TELR_E_ARG);
        a = ok; a[0].qe = 3857;
        expect("qe beyond its tile", run(a, tiles, tl, 1, O), TELR_E_ARG);
        a = ok; a[1].qs = 2553;
        expect("qs > qe", run(a, tiles, tl, 1, O), TELR_E_ARG);
        std::vector<telr_tile> t = tiles; t[3].len = 3857;
        expect("tile beyond its target", run(ok, t, tl, 1, O), TELR_E_ARG);
        t = tiles; t[0].tid = 1;
        expect("tile of no target", run(ok, t, tl, 1, O), TELR_E_ARG);
        const int32_t bad_tl[1] = {-1};
        expect("negative target length", run(ok, tiles, bad_tl, 1, O), TELR_E_ARG);
        expect("null records", refte_check(nullptr, 3, (int64_t)tiles.size(), tiles.data(), 1, tl, 1, &O, &mx, &why), TELR_E_ARG);
        expect("too many records", refte_check(ok.data(), 0x7ffffff0LL, (int64_t)tiles.size(), tiles.data(), 1, tl, 1, &O, &mx, &why), TELR_E_RANGE);
    }
    if (n_bad) { fprintf(stderr, "refte: %d of %d checks FAILED\n", n_bad, n_checks); return 1; }
    printf("refte: %d checks ok\n", n_checks);
    return 0;
}
