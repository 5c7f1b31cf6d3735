// bai_plan_host.cpp -- telr_amd/csrc/bai_plan.h (the .bai reader, reg2bins, the linear-index cut, the merge into intervals and the region
// normaliser) compiled for the CPU, meant to be built with -fsanitize=address,undefined and run over an index BEFORE the region load
// meets a device:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ubench/bai_plan_host.cpp -o bai_plan_host
//   python -c "import sys; sys.path[:0] = ['tests', '.']; import bam_region_ref as G; open('mid.bai', 'wb').write(G.layout('mid')['bai'])"
//   ./bai_plan_host mid.bai
//
// Every run holds the index in a heap block of exactly its size, so a read behind it is an ASan report.  The valid index is planned for
// a handful of region lists; then every truncation of it by one byte more, and copies with a count (n_ref, a bin count, a chunk count, a
// linear count) or a bin number overwritten: any status is right, no report is the point.  The normaliser's refusals are checked too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../telr_amd/csrc/bai_plan.h"

static int plan_copy(const uint8_t *src, size_t n, int32_t n_ref, const std::vector<BaiRegion> &merged, size_t *n_iv)
{
    uint8_t *d = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(d, src, n);
    std::vector<uint64_t> vb, ve; std::string why;
    const int rc = bai_plan(d, n, n_ref, merged, vb, ve, &why);
    if (rc == TELR_OK) {
        for (size_t i = 0; i < vb.size(); ++i) {
            if (vb[i] >= ve[i] || (i && (vb[i] >> 16) <= (ve[i - 1] >> 16))) { printf("FAIL: interval %zu is empty or shares a member with the one before\n", i); free(d); return -100; }
        }
    } else if (why.empty()) { printf("FAIL: a refusal without a reason\n"); free(d); return -100; }
    if (n_iv) *n_iv = vb.size();
    free(d);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: bai_plan_host INDEX.bai\n"); return 2; }
    std::vector<uint8_t> bai; std::string why;
    if (bai_read_file(argv[1], bai, &why) != TELR_OK || bai.size() < 8) { fprintf(stderr, "%s\n", why.c_str()); return 2; }
    const int32_t n_ref = (int32_t)bai_ld32(bai.data() + 4);
    int bad = 0;
    // the normaliser
    {
        const telr_region ok[] = { {0, 100, 200, 0}, {0, 150, 300, 0}, {0, 300, 400, 0}, {n_ref - 1, 0, 1 << 30, 0}, {0, 0, 50, 0} };
        std::vector<BaiRegion> m;
        if (bai_regions(n_ref, nullptr, 5, ok, m, &why) != TELR_OK || m.size() != (n_ref > 1 ? 3u : 2u) || m[0].end != 50 || m[1].beg != 100 || m[1].end != 400) { printf("FAIL: merged regions\n"); ++bad; }
        const telr_region no[] = { {n_ref, 0, 1, 0}, {-1, 0, 1, 0}, {0, -1, 1, 0}, {0, 5, 5, 0}, {0, 0, 1, 1} };
        for (const telr_region &r : no) if (bai_regions(n_ref, nullptr, 1, &r, m, &why) != TELR_E_ARG) { printf("FAIL: a bad region was accepted\n"); ++bad; }
        if (bai_regions(n_ref, nullptr, -1, ok, m, &why) != TELR_E_ARG || bai_regions(n_ref, nullptr, 1, nullptr, m, &why) != TELR_E_ARG) { printf("FAIL: bad counts accepted\n"); ++bad; }
    }
    // region lists: every reference whole, one window each, single bases at seams, nothing
    std::vector<std::vector<BaiRegion>> lists(5);
    for (int32_t t = 0; t < n_ref; ++t) {
        lists[0].push_back(BaiRegion{t, 0, BAI_MAX_COOR});
        lists[1].push_back(BaiRegion{t, 16384, 32768});
        lists[2].push_back(BaiRegion{t, 16383, 16385});
        lists[2].push_back(BaiRegion{t, (1 << 26) - 1, (1 << 26) + 1});
        lists[3].push_back(BaiRegion{t, BAI_MAX_COOR - 1, BAI_MAX_COOR});
    }
    size_t n_iv = 0; long runs = 0, still_ok = 0;
    for (const auto &l : lists) {
        const int rc = plan_copy(bai.data(), bai.size(), n_ref, l, &n_iv);
        if (rc != TELR_OK) { printf("FAIL: the valid index was refused (%d)\n", rc); ++bad; }
        else printf("%zu regions -> %zu intervals\n", l.size(), n_iv);
    }
    // every truncation
    for (size_t n = 0; n < bai.size(); ++n) {
        const int rc = plan_copy(bai.data(), n, n_ref, lists[n & 1 ? 2 : 1], nullptr);
        ++runs; if (rc == TELR_OK) ++still_ok; if (rc == -100) ++bad;
    }
    // corrupted counts and bin numbers: every 4-byte field of the first 4 KiB and 256 more spread over the file, six values each
    const int32_t vals[] = { -1, INT32_MIN, INT32_MAX, 1 << 28, 37450, 0 };
    std::vector<uint8_t> c(bai);
    uint64_t x = 0x9E3779B97F4A7C15ull ^ bai.size();
    for (size_t k = 0; k < 1024 + 256; ++k) {
        size_t at;
        if (k < 1024) { at = 4 + 4 * k; if (at + 4 > bai.size()) break; }
        else { x ^= x << 13; x ^= x >> 7; x ^= x << 17; at = (size_t)(x % (bai.size() - 3)); }
        for (int32_t v : vals) {
            memcpy(c.data() + at, &v, 4);
            for (const auto *l : { k % 8 ? &lists[1] : &lists[0], &lists[2] }) {          // (whole references every eighth time: 37,449 bins each; a changed n_ref is also tried as the caller's)
                const int rc = plan_copy(c.data(), c.size(), at == 4 && v >= 0 ? v : n_ref, *l, nullptr);
                ++runs; if (rc == TELR_OK) ++still_ok; if (rc == -100) ++bad;
            }
        }
        memcpy(c.data() + at, bai.data() + at, 4);
    }
    printf("bai_plan_host: %ld truncated / corrupted copies planned to a status (%ld of them still an index), %d failures\n", runs, still_ok, bad);
    return bad ? 1 : 0;
}
