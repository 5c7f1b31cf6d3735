// reads_text_host.cpp -- the per-record and per-word functions of telr_amd/csrc/reads_text_core.h, compiled for the CPU and run in the
// loops that the kernels of reads_in.hip.h run with one lane each: every case and every error case of tests/reads_in_ref.py.  Built
// with -fsanitize=address,undefined by tests/test_reads_in_ref.py.  The text sits in a heap block of exactly bias + text + 64 bytes
// (bias 0 and 5: the block is 16-byte aligned, as a chunk's slot is), every output in a block of exactly the layout's size, so a load
// or a store outside what the device code may touch is a report.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/ubench/reads_text_host.cpp -o reads_text_host && ./reads_text_host cases.bin
#include "../../telr_amd/csrc/reads_text_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct Reader {
    std::vector<uint8_t> d; size_t p = 0;
    template <typename T> T get() { T v; memcpy(&v, d.data() + p, sizeof(T)); p += sizeof(T); return v; }
    const uint8_t *bytes(size_t n) { const uint8_t *r = d.data() + p; p += n; return r; }
};
struct Want {
    int keep_qual, status; int64_t record;
    std::vector<uint8_t> text;
    int fastq = 0;
    std::vector<int32_t> lens; std::vector<std::string> names;
    std::vector<uint32_t> w2, wn; std::vector<uint8_t> q; bool has_q = false;
};

static int64_t rec_of(const std::vector<int64_t> &goff, int64_t g)
{
    int64_t lo = 0, hi = (int64_t)goff.size() - 1;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (goff[mid] <= g) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

// -> "" when the case's answer is the wanted one
static std::string run(const Want &W, int bias)
{
    const int64_t len = (int64_t)W.text.size();
    void *blk = nullptr;
    if (posix_memalign(&blk, 16, (size_t)(bias + len + 64))) return "no memory";
    memset(blk, 0, (size_t)(bias + len + 64));
    if (len) memcpy((uint8_t*)blk + bias, W.text.data(), (size_t)len);
    RtText T; T.q = (const uint64_t*)blk; T.bias = bias; T.len = len;
    std::string why;
    int status = RTS_OK; int64_t record = -1;
    std::vector<RtRec> recs;
    std::vector<int64_t> ls(1, 0), S, hl;
    do {
        if (!len) break;
        const uint32_t c0 = rt_byte(T, 0);
        if (c0 != '@' && c0 != '>') { status = 100; break; }
        for (int64_t p = 0; p < len; ++p) if (rt_byte(T, p) == '\n') ls.push_back(p + 1);
        const int64_t nl = (int64_t)ls.size() - 1, nlines = nl + (rt_byte(T, len - 1) != '\n' ? 1 : 0);
        int64_t *lsx = (int64_t*)malloc((size_t)(nl + 1) * 8);          // exactly nl + 1 entries
        memcpy(lsx, ls.data(), (size_t)(nl + 1) * 8);
        if (c0 == '@') {
            for (int64_t r = 0; r < (nlines + 3) / 4; ++r) {
                const RtRec R = rt_fastq_record(T, lsx, nl, nlines, r);
                if (R.status != RTS_OK) { status = R.status; record = r; break; }
                recs.push_back(R);
            }
        } else {
            S.assign((size_t)nlines + 1, 0);
            for (int64_t j = 0; j < nlines; ++j) {
                int64_t s, e;
                rt_line(T, lsx, nl, j, &s, &e);
                const bool h = e > s && rt_byte(T, s) == '>';
                if (h) hl.push_back(j);
                S[(size_t)j + 1] = S[(size_t)j] + (h ? 0 : e - s);
            }
            hl.push_back(nlines);
            int64_t *Sx = (int64_t*)malloc((size_t)(nlines + 1) * 8);
            memcpy(Sx, S.data(), (size_t)(nlines + 1) * 8);
            for (size_t r = 0; r + 1 < hl.size(); ++r) recs.push_back(rt_fasta_record(T, lsx, nl, Sx, hl[r], hl[r + 1]));
            free(Sx);
        }
        // the set's words, as the kernels write them
        const int64_t n = (int64_t)recs.size();
        std::vector<int64_t> goff((size_t)n + 1, 0);
        for (int64_t r = 0; r < n; ++r) goff[(size_t)r + 1] = goff[(size_t)r] + (((int64_t)recs[(size_t)r].len + 63) >> 6);
        const int64_t G = goff[(size_t)n];
        uint32_t *w2 = (uint32_t*)malloc((size_t)G * 16 + 1), *wn = (uint32_t*)malloc((size_t)G * 8 + 1);
        uint8_t *q = (uint8_t*)malloc((size_t)G * 64 + 1);
        int64_t *Sx = S.empty() ? nullptr : (int64_t*)malloc(S.size() * 8);
        if (Sx) memcpy(Sx, S.data(), S.size() * 8);
        std::vector<uint32_t> m16s((size_t)G * 4);
        for (int64_t w = 0; w < G * 4 && n; ++w) {
            const int64_t r = rec_of(goff, w >> 2);
            const RtRec &R = recs[(size_t)r];
            const int64_t j0 = (w - goff[(size_t)r] * 4) * 16, left = (int64_t)R.len - j0;
            const int v = left >= 16 ? 16 : left > 0 ? (int)left : 0;
            uint64_t lo, hi;
            if (R.multi && v > 0) rt_fasta_gather16(T, lsx, Sx, R.first_line, R.first_line + 1 + R.n_lines, Sx[R.first_line] + j0, v, lo, hi);
            else rt_load16(T, v > 0 ? R.seq_pos + j0 : 0, lo, hi);
            uint32_t code, m16;
            rt_pack16(lo, hi, v, code, m16);
            w2[w] = code; m16s[(size_t)w] = m16;
        }
        for (int64_t w = 0; w < G * 4; w += 2) wn[w >> 1] = m16s[(size_t)w] | m16s[(size_t)w + 1] << 16;
        const bool qual = W.keep_qual && c0 == '@';
        if (qual && status == RTS_OK) {
            for (int64_t w = 0; w < G * 16 && n; ++w) {
                const int64_t r = rec_of(goff, w >> 4);
                const RtRec &R = recs[(size_t)r];
                const int64_t j0 = (w - goff[(size_t)r] * 16) * 4, left = (int64_t)R.len - j0;
                const int v = left >= 4 ? 4 : left > 0 ? (int)left : 0;
                bool bad;
                const uint32_t x = rt_qual4((uint32_t)rt_load8(T, v > 0 ? R.qual_pos + j0 : 0), v, &bad);
                memcpy(q + 4 * w, &x, 4);
                if (bad && (status != RTS_QUAL || r < record)) { status = RTS_QUAL; record = r; }
            }
        } else if (qual) {
            // the records below a grammar fault still have their qualities checked: a lower record wins
            for (int64_t r = 0; r < n && status != RTS_QUAL; ++r)
                for (int64_t j0 = 0; j0 < recs[(size_t)r].len; j0 += 4) {
                    const int64_t left = recs[(size_t)r].len - j0; bool bad;
                    (void)rt_qual4((uint32_t)rt_load8(T, recs[(size_t)r].qual_pos + j0), left >= 4 ? 4 : (int)left, &bad);
                    if (bad) { status = RTS_QUAL; record = r; break; }
                }
        }
        if (status == RTS_OK) {
            if ((int)(c0 == '@') != W.fastq) why = "kind";
            if (n != (int64_t)W.lens.size()) why = "record count " + std::to_string(n);
            for (int64_t r = 0; r < n && why.empty(); ++r) {
                const RtRec &R = recs[(size_t)r];
                if (R.len != W.lens[(size_t)r]) why = "length of record " + std::to_string(r);
                std::string nm((size_t)R.name_len, '\0');
                const int64_t src = lsx[R.first_line] + 1;
                for (int32_t k = 0; k < R.name_len; k += 8) {
                    const uint64_t x = rt_load8(T, src + k);
                    for (int b = 0; b < 8 && k + b < R.name_len; ++b) nm[(size_t)(k + b)] = (char)(x >> (8 * b));
                }
                if (nm != W.names[(size_t)r]) why = "name of record " + std::to_string(r);
            }
            if (why.empty() && ((size_t)G * 4 != W.w2.size() || (G && memcmp(w2, W.w2.data(), (size_t)G * 16)))) why = "2-bit words";
            if (why.empty() && ((size_t)G * 2 != W.wn.size() || (G && memcmp(wn, W.wn.data(), (size_t)G * 8)))) why = "mask words";
            if (why.empty() && qual != W.has_q) why = "qualities kept";
            if (why.empty() && qual && ((size_t)G * 64 != W.q.size() || (G && memcmp(q, W.q.data(), (size_t)G * 64)))) why = "Phred bytes";
        }
        free(w2); free(wn); free(q); free(Sx); free(lsx);
    } while (0);
    free(blk);
    if (!why.empty()) return why;
    if (status != W.status) return "status " + std::to_string(status) + " at record " + std::to_string(record) + ", wanted " + std::to_string(W.status);
    if (status != RTS_OK && status != 100 && record != W.record) return "record " + std::to_string(record) + ", wanted " + std::to_string(W.record);
    return "";
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: reads_text_host cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    Reader R;
    fseek(f, 0, SEEK_END); R.d.resize((size_t)ftell(f)); fseek(f, 0, SEEK_SET);
    if (fread(R.d.data(), 1, R.d.size(), f) != R.d.size()) return 2;
    fclose(f);
    const uint32_t ncase = R.get<uint32_t>();
    int failed = 0;
    for (uint32_t c = 0; c < ncase; ++c) {
        Want W;
        const uint32_t nlen = R.get<uint32_t>();
        const std::string name((const char*)R.bytes(nlen), nlen);
        W.keep_qual = (int)R.get<uint32_t>(); W.status = R.get<int32_t>(); W.record = R.get<int64_t>();
        const uint64_t tl = R.get<uint64_t>();
        const uint8_t *t = R.bytes(tl); W.text.assign(t, t + tl);
        if (W.status == 0) {
            const uint32_t n = R.get<uint32_t>(); W.fastq = (int)R.get<uint32_t>();
            for (uint32_t r = 0; r < n; ++r) {
                W.lens.push_back(R.get<int32_t>());
                const uint32_t k = R.get<uint32_t>();
                W.names.emplace_back((const char*)R.bytes(k), k);
            }
            const uint64_t n2 = R.get<uint64_t>(); W.w2.resize(n2); if (n2) memcpy(W.w2.data(), R.bytes(n2 * 4), n2 * 4);
            const uint64_t nn = R.get<uint64_t>(); W.wn.resize(nn); if (nn) memcpy(W.wn.data(), R.bytes(nn * 4), nn * 4);
            W.has_q = R.get<uint32_t>() != 0;
            const uint64_t nq = R.get<uint64_t>(); W.q.resize(nq); if (nq) memcpy(W.q.data(), R.bytes(nq), nq);
        }
        for (int bias : { 0, 5 }) {
            const std::string why = run(W, bias);
            if (!why.empty()) { printf("FAILED %s (bias %d): %s\n", name.c_str(), bias, why.c_str()); ++failed; break; }
        }
    }
    printf("%u cases, %d failed\n", ncase, failed);
    return failed ? 1 : 0;
}
