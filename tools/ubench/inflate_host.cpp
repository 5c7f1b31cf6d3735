// inflate_host.cpp -- the host twin of the device BGZF decoder: telr_amd/csrc/inflate_core.h compiled for the CPU, meant to be built
// with -fsanitize=address,undefined and run on the deflate cases of tests/bam_in_ref.py BEFORE the decoder meets a device:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ubench/inflate_host.cpp -lz -o inflate_host
//   python -c "import sys; sys.path.insert(0, 'tests'); import bam_in_ref as R; R.write_case_file('cases.bin')" && ./inflate_host cases.bin
//
// The window and the tables are heap blocks of exactly the size the kernel has, so an index outside them is an ASan report.
// Per case of the file: the decoder's status is the expected one; a good member gives zlib's bytes and the trailer's CRC through the
// 64-lane CRC split.  Then every good member is run again truncated (64 cuts and the last 16 byte counts) and with single bits
// flipped (every bit of the first 16 bytes, 512 more spread over the stream): any status is right, no report is the point.
// Case file: "BIC1", then per case { u32 name_len, name, u32 expect, u32 isize, u32 crc, u32 in_len, bytes }.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>
#include "../../telr_amd/csrc/inflate_core.h"

struct HostSrc {
    const uint8_t *p;
    uint32_t get8(uint32_t pos) const { return p[pos]; }
    uint32_t get32(uint32_t pos) const { return (uint32_t)p[pos] | (uint32_t)p[pos + 1] << 8 | (uint32_t)p[pos + 2] << 16 | (uint32_t)p[pos + 3] << 24; }
};
struct HostSink {
    uint8_t *win; const uint8_t *in;
    void lit(uint32_t pos, uint8_t b) { win[pos] = b; }
    void match(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i) win[pos + i] = win[pos - dist + i % dist]; }      // the lanes' formula
    void stored(uint32_t pos, uint32_t ipos, uint32_t len) { for (uint32_t i = 0; i < len; ++i) win[pos + i] = in[ipos + i]; }
};

static uint32_t byte_tab[256], xpow64[1024];
static void make_tabs()
{
    for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1; byte_tab[i] = c; }
    uint32_t x64 = 0x80000000u;
    for (int i = 0; i < 8 * 64; ++i) x64 = (x64 & 1u) ? (x64 >> 1) ^ 0xEDB88320u : x64 >> 1;
    xpow64[0] = 0x80000000u;
    for (int k = 1; k < 1024; ++k) xpow64[k] = infl_gf2_mulmod(xpow64[k - 1], x64);
}

// one run: input and window in heap blocks of their exact sizes
static int run(const uint8_t *in, uint32_t in_len, uint32_t isize, uint32_t crc, std::vector<uint8_t> *out)
{
    uint8_t *ibuf = (uint8_t*)malloc(in_len ? in_len : 1);
    uint8_t *win = (uint8_t*)malloc(isize ? isize : 1);
    InflTables *T = (InflTables*)malloc(sizeof(InflTables));
    if (in_len) memcpy(ibuf, in, in_len);
    HostSrc S{ibuf}; HostSink W{win, ibuf};
    int st = infl_member(S, in_len, isize, T, W);
    if (st == INFL_OK) {
        uint32_t c = 0;
        for (int lane = 0; lane < 64; ++lane) c ^= infl_crc_lane(win, isize, lane, byte_tab, xpow64);
        if ((isize ? ~c : 0u) != crc) st = INFL_E_CRC;      // (no byte: the CRC of nothing is 0)
        if (out) out->assign(win, win + isize);
    }
    free(T); free(win); free(ibuf);
    return st;
}

static bool rd32(FILE *f, uint32_t *v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: inflate_host CASEFILE\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    char magic[4];
    if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "BIC1", 4)) { fprintf(stderr, "%s: not a case file\n", argv[1]); return 2; }
    make_tabs();
    int n_case = 0, n_bad = 0; long n_mut = 0, n_mut_ok = 0;
    uint32_t nl;
    while (rd32(f, &nl)) {
        std::string name(nl, ' ');
        uint32_t expect, isize, crc, in_len;
        if (fread(&name[0], 1, nl, f) != nl || !rd32(f, &expect) || !rd32(f, &isize) || !rd32(f, &crc) || !rd32(f, &in_len)) { fprintf(stderr, "truncated case file\n"); return 2; }
        std::vector<uint8_t> in(in_len);
        if (in_len && fread(in.data(), 1, in_len, f) != in_len) { fprintf(stderr, "truncated case file\n"); return 2; }
        ++n_case;
        std::vector<uint8_t> got;
        const int st = run(in.data(), in_len, isize, crc, &got);
        if ((uint32_t)st != expect) { printf("FAIL %s: status %d, expected %u\n", name.c_str(), st, expect); ++n_bad; continue; }
        if (expect != INFL_OK) continue;
        // zlib's bytes
        std::vector<uint8_t> ref(isize + 1);
        z_stream z; memset(&z, 0, sizeof(z));
        inflateInit2(&z, -15);
        z.next_in = in.data(); z.avail_in = in_len; z.next_out = ref.data(); z.avail_out = isize + 1;
        const int zr = inflate(&z, Z_FINISH);
        const bool same = zr == Z_STREAM_END && z.total_out == isize && (isize == 0 || !memcmp(ref.data(), got.data(), isize)) && crc32(0, ref.data(), isize) == crc;
        inflateEnd(&z);
        if (!same) { printf("FAIL %s: output differs from zlib's\n", name.c_str()); ++n_bad; continue; }
        // truncated copies
        for (int k = 0; k < 80; ++k) {
            const uint32_t cut = k < 64 ? (uint32_t)((uint64_t)in_len * k / 64) : in_len - (uint32_t)(k - 63);
            if (cut >= in_len) continue;
            const int s2 = run(in.data(), cut, isize, crc, nullptr);
            ++n_mut; if (s2 == INFL_OK) ++n_mut_ok;
        }
        // single bits flipped
        uint64_t x = 0x9E3779B97F4A7C15ull ^ in_len;
        const long nbits = (long)in_len * 8;
        for (long k = 0; k < 128 + 512 && nbits; ++k) {
            long bit;
            if (k < 128) { bit = k; if (bit >= nbits) break; }
            else { x ^= x << 13; x ^= x >> 7; x ^= x << 17; bit = (long)(x % (uint64_t)nbits); }
            in[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            const int s2 = run(in.data(), in_len, isize, crc, nullptr);
            in[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            ++n_mut; if (s2 == INFL_OK) ++n_mut_ok;
        }
    }
    fclose(f);
    printf("inflate_host: %d cases, %d failed; %ld truncated / bit-flipped copies decoded to a status (%ld of them still valid)\n", n_case, n_bad, n_mut, n_mut_ok);
    return n_bad ? 1 : 0;
}
