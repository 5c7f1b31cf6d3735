// sam_records.h — what a SAM / BAM record, the file header and the .bai are made of on the host, each stated once: the SAM
// writer, the host BAM writer (sam_host.hip.h) and the host side of the device BAM writer (bam_dev.hip.h) are built from these.
// Plain C++ on records and characters: no HIP call, no engine type, so it is checked on a CPU by a program of its own
// (tools/sam_records_check.cpp).  The device kernels of bam_dev.hip.h restate the layout and the walk for the GPU; the tests
// hold both to tests/bam_reference.py byte for byte.
#ifndef TELR_SAM_RECORDS_H
#define TELR_SAM_RECORDS_H
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/telr_hip.h"

// ---- bases and bytes ---------------------------------------------------------------------------------------------------
static const char COMP_TAB[256] = {
#define C16 'N','N','N','N','N','N','N','N','N','N','N','N','N','N','N','N'
    C16, C16, C16, C16,
    'N','T','N','G','N','N','N','C','N','N','N','N','N','N','N','N','N','N','N','N','A','A','N','N','N','N','N','N','N','N','N','N',
    'N','t','N','g','N','N','N','c','N','N','N','N','N','N','N','N','N','N','N','N','a','a','N','N','N','N','N','N','N','N','N','N',
    C16, C16, C16, C16, C16, C16, C16, C16
#undef C16
};
// bases as the engine sees them (the 2-bit packing: A C G T/U in either case, anything else ambiguous): what NM / MD / cs
// print, so that the text writers and the device-side BAM writer (bam_dev.hip.h) agree byte for byte
static inline char up(char c)
{
    switch (c) { case 'A': case 'a': return 'A'; case 'C': case 'c': return 'C'; case 'G': case 'g': return 'G'; case 'T': case 't': case 'U': case 'u': return 'T'; default: return 'N'; }
}
static inline uint8_t nt16(char c)          // the 4-bit SEQ code of BAM
{
    switch (c) { case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'G': case 'g': return 4; case 'T': case 't': case 'U': case 'u': return 8; default: return 15; }
}
static inline int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
static inline void put16(std::string &s, uint16_t v) { s.append((const char*)&v, 2); }
static inline void put32(std::string &s, uint32_t v) { s.append((const char*)&v, 4); }
static inline void put64(std::string &s, uint64_t v) { s.append((const char*)&v, 8); }

#define BAM_BLK 65280            /* uncompressed bytes per BGZF block, in every BAM writer */
// every BGZF block begins with these 16 bytes (the gzip header with the BC extra field; BSIZE - 1 follows them); the end-of-file
// block is that head, BSIZE - 1 = 27, an empty deflate block, CRC-32 0 and ISIZE 0
#define BGZF_HEAD_BYTES 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0
static const uint8_t BGZF_HEAD[16] = { BGZF_HEAD_BYTES };
static const uint8_t BGZF_EOF[28] = { BGZF_HEAD_BYTES, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };

// ---- the layout of one record ------------------------------------------------------------------------------------------
// hard clips only on a supplementary record without TELR_SAM_SOFTCLIP; a secondary has SEQ '*' and soft clips, as minimap2
// without --secondary-seq.  SEQ / QUAL hold bases [seq_lo, seq_lo + l_seq) of the read on the alignment strand.
// key: the coordinate order of `samtools sort` (refID, position, forward before reverse); a stable sort keeps the input order
// of equal keys, and SAM_KEY_UNMAPPED puts the reads without a record last.
struct RecLayout { bool rev, sec, sup, hard; int clip5, clip3, flag, seq_lo, l_seq; int64_t key; };
static const int64_t SAM_KEY_UNMAPPED = INT64_MAX;
static inline RecLayout rec_layout(const telr_aln &a, int qlen, int flags)
{
    RecLayout L;
    L.rev = (a.flags & TELR_F_REV) != 0; L.sec = (a.flags & TELR_F_SECONDARY) != 0; L.sup = (a.flags & TELR_F_SUPPL) != 0;
    L.clip5 = L.rev ? qlen - a.qe : a.qs; L.clip3 = L.rev ? a.qs : qlen - a.qe;
    L.hard = L.sup && !(flags & TELR_SAM_SOFTCLIP);
    L.flag = (L.rev ? 0x10 : 0) | (L.sec ? 0x100 : 0) | (L.sup ? 0x800 : 0);
    L.seq_lo = L.hard ? L.clip5 : 0;
    L.l_seq = L.sec ? 0 : (L.hard ? qlen - L.clip5 - L.clip3 : qlen);
    L.key = ((int64_t)(a.tid + 1) << 33) | (int64_t)(uint32_t)a.ts << 1 | (L.rev ? 1 : 0);
    return L;
}

// ---- the alignment walk: NM, MD, cs ------------------------------------------------------------------------------------
// qstr: the read on the alignment strand (whole read; the first aligned base is qstr[clip5]); t: the target (the first aligned
// base is t[ts]).  MD and cs are APPENDED to md / cs when their TELR_SAM_* bit is set (the caller clears and reuses the strings).
// A column with an ambiguous base on either side is a mismatch.  -> NM
static inline int aln_walk(const char *qstr, const char *t, const uint32_t *cg, int n_cigar, int clip5, int ts, int flags, std::string &md, std::string &cs)
{
    const bool want_md = (flags & TELR_SAM_MD) != 0, want_cs = (flags & TELR_SAM_CS) != 0;
    int nm = 0, qi = clip5, ti = ts, run = 0;
    char buf[32];
    for (int z = 0; z < n_cigar; ++z) {
        const int op = cg[z] & 0xf, l = (int)(cg[z] >> 4);
        if (op == 0) {
            int csrun = 0;
            for (int x = 0; x < l; ++x) {
                const char qc = up(qstr[qi + x]), tc = up(t[ti + x]);
                if (qc == tc && tc != 'N') { ++run; ++csrun; }
                else {
                    ++nm;
                    if (want_md) { snprintf(buf, sizeof(buf), "%d%c", run, tc); md += buf; }
                    run = 0;
                    if (want_cs) { if (csrun) { snprintf(buf, sizeof(buf), ":%d", csrun); cs += buf; csrun = 0; } cs += '*'; cs += (char)(tc | 32); cs += (char)(qc | 32); }
                }
            }
            if (want_cs && csrun) { snprintf(buf, sizeof(buf), ":%d", csrun); cs += buf; }
            qi += l; ti += l;
        } else if (op == 1) {
            nm += l;
            if (want_cs) { cs += '+'; for (int x = 0; x < l; ++x) cs += (char)(up(qstr[qi + x]) | 32); }
            qi += l;
        } else {
            nm += l;
            if (want_md) { snprintf(buf, sizeof(buf), "%d^", run); md += buf; for (int x = 0; x < l; ++x) md += up(t[ti + x]); run = 0; }
            if (want_cs) { cs += '-'; for (int x = 0; x < l; ++x) cs += (char)(up(t[ti + x]) | 32); }
            ti += l;
        }
    }
    if (want_md) { snprintf(buf, sizeof(buf), "%d", run); md += buf; }
    return nm;
}

// ---- SA: the other primary / supplementary records of the read ---------------------------------------------------------
// alns[0 .. n): the records of ONE read; self: the record the tag is for; cig: the CIGAR words cigar_off points into.
// One "rname,pos,strand,CIGAR,mapQ,NM;" per record is appended to out, its CIGAR reduced to clip / M / I / D totals.
static inline void sa_text(const telr_aln *alns, size_t n, size_t self, int qlen, const uint32_t *cig, const char *const *tnames, std::string &out)
{
    char sb[64];
    for (size_t k = 0; k < n; ++k) {
        const telr_aln &b = alns[k];
        if (k == self || (b.flags & TELR_F_SECONDARY)) continue;
        const bool brev = (b.flags & TELR_F_REV) != 0;
        const int b5 = brev ? qlen - b.qe : b.qs, b3 = brev ? b.qs : qlen - b.qe;
        int nI = 0, nD = 0;
        for (int z = 0; z < b.n_cigar; ++z) { const uint32_t c = cig[b.cigar_off + z]; if ((c & 0xf) == 1) nI += c >> 4; else if ((c & 0xf) == 2) nD += c >> 4; }
        out += tnames[b.tid];
        snprintf(sb, sizeof(sb), ",%d,%c,", b.ts + 1, brev ? '-' : '+'); out += sb;
        if (b5) { snprintf(sb, sizeof(sb), "%dS", b5); out += sb; }
        snprintf(sb, sizeof(sb), "%dM", (b.qe - b.qs) - nI); out += sb;
        if (nI) { snprintf(sb, sizeof(sb), "%dI", nI); out += sb; }
        if (nD) { snprintf(sb, sizeof(sb), "%dD", nD); out += sb; }
        if (b3) { snprintf(sb, sizeof(sb), "%dS", b3); out += sb; }
        snprintf(sb, sizeof(sb), ",%d,%d;", b.mapq, b.blen - b.mlen); out += sb;
    }
}

// ---- the header ----------------------------------------------------------------------------------------------------------
static inline std::string sam_header_text(bool sorted, int32_t n_targets, const char *const *tnames, const int32_t *t_len,
                                          const char *rg_id, const char *rg_sm, const char *rg_lb, const char *pg_line)
{
    std::string text = sorted ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
    for (int t = 0; t < n_targets; ++t) { text += "@SQ\tSN:"; text += tnames[t]; text += "\tLN:"; text += std::to_string(t_len[t]); text += '\n'; }
    if (rg_id) { text += "@RG\tID:"; text += rg_id; text += "\tSM:"; text += rg_sm ? rg_sm : rg_id; text += "\tLB:"; text += rg_lb ? rg_lb : "lib"; text += '\n'; }
    text += "@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:"; text += pg_line ? pg_line : "telr_map"; text += '\n';
    return text;
}
// the head of a BAM stream: magic, the text of a coordinate-sorted file, the reference table
static inline std::string bam_header(int32_t n_targets, const char *const *tnames, const int32_t *t_len, const char *rg_id, const char *rg_sm, const char *rg_lb, const char *pg_line)
{
    const std::string text = sam_header_text(true, n_targets, tnames, t_len, rg_id, rg_sm, rg_lb, pg_line);
    std::string head = "BAM\1";
    put32(head, (uint32_t)text.size()); head += text; put32(head, (uint32_t)n_targets);
    for (int t = 0; t < n_targets; ++t) { const uint32_t ln = (uint32_t)strlen(tnames[t]) + 1; put32(head, ln); head.append(tnames[t], ln); put32(head, (uint32_t)t_len[t]); }
    return head;
}

// ---- the .bai ------------------------------------------------------------------------------------------------------------
// One builder for every writer.  The mapped records come in FILE order as entries (reference, start, end, offset of the first
// byte, offset behind the last byte); n_no_coor reads without coordinates follow them.  An offset is whatever orders the file and
// tells its BGZF block through blk_of: a virtual file offset (blk_of = v >> 16), or an offset into the uncompressed stream
// (blk_of = u / BAM_BLK) -- then `fix` receives the position of every offset field inside `bai`, and bai_finish rewrites them to
// virtual offsets once the blocks' file offsets are known, so the index is laid out while the blocks are still being coded.
// Per reference: bins in ascending order, the chunks of a bin joined while one ends in the block the next begins in (samtools),
// the metadata pseudo-bin, the 16-kb linear index with untouched windows back-filled (0 before the first record).
// -> false: the entries are not in file order (nothing usable in bai)
struct BaiEntry { int32_t tid, ts, te; uint64_t beg, end; };
template <class At, class BlkOf>
static bool bai_build(size_t n, At at, BlkOf blk_of, uint64_t n_no_coor, int32_t n_targets, const int32_t *t_len, std::string &bai, std::vector<size_t> *fix)
{
    auto put_off = [&](uint64_t v) { if (fix && v) fix->push_back(bai.size()); put64(bai, v); };          // (0 = "from the start of the file" stays 0)
    if (fix) fix->clear();
    bai = "BAI\1"; put32(bai, (uint32_t)n_targets);
    size_t i = 0;
    struct Ch { uint32_t bin; uint64_t beg, end; };
    std::vector<Ch> chs;
    std::vector<uint64_t> lin;
    for (int t = 0; t < n_targets; ++t) {
        chs.clear();
        const int n_lin = (t_len[t] >> 14) + 1;
        lin.assign((size_t)n_lin, 0);
        int max_lin = 0;
        uint64_t ref_beg = 0, ref_end = 0;
        for (; i < n; ++i) {
            const BaiEntry a = at(i);
            if (a.tid != t) { if (a.tid < t) return false; break; }
            const int e = a.te > a.ts ? a.te : a.ts + 1;          // a record without a reference base: the bin and window of [ts, ts + 1)
            if (chs.empty()) ref_beg = a.beg;
            ref_end = a.end;
            chs.push_back(Ch{ (uint32_t)reg2bin(a.ts, e), a.beg, a.end });
            for (int wv = a.ts >> 14; wv <= (e - 1) >> 14 && wv < n_lin; ++wv) { if (lin[wv] == 0 || a.beg < lin[wv]) lin[wv] = a.beg; if (wv + 1 > max_lin) max_lin = wv + 1; }
        }
        const uint64_t n_map = chs.size();
        std::stable_sort(chs.begin(), chs.end(), [](const Ch &x, const Ch &y) { return x.bin < y.bin; });
        const size_t p_nbin = bai.size(); uint32_t nbin = 0;
        put32(bai, 0);
        for (size_t c0 = 0; c0 < chs.size(); ) {
            const size_t p_nc = bai.size() + 4; uint32_t nc = 0;
            put32(bai, chs[c0].bin); put32(bai, 0);
            size_t c1 = c0;
            while (c1 < chs.size() && chs[c1].bin == chs[c0].bin) {
                uint64_t end = chs[c1].end; const uint64_t beg = chs[c1++].beg;
                while (c1 < chs.size() && chs[c1].bin == chs[c0].bin && blk_of(end) == blk_of(chs[c1].beg)) end = chs[c1++].end;
                put_off(beg); put_off(end); ++nc;
            }
            memcpy(&bai[p_nc], &nc, 4);
            ++nbin; c0 = c1;
        }
        if (n_map) {          // samtools' metadata pseudo-bin
            put32(bai, 37450u); put32(bai, 2u);
            put_off(ref_beg); put_off(ref_end); put64(bai, n_map); put64(bai, 0);
            ++nbin;
        }
        memcpy(&bai[p_nbin], &nbin, 4);
        for (int wv = 1; wv < max_lin; ++wv) if (lin[wv] == 0) lin[wv] = lin[wv - 1];
        put32(bai, (uint32_t)max_lin);
        for (int wv = 0; wv < max_lin; ++wv) put_off(lin[wv]);
    }
    put64(bai, n_no_coor);
    return i == n;          // (entries left over: a reference beyond n_targets)
}
// offset u of the uncompressed stream as a virtual file offset; coff[nblk + 1]: the file offset of every block and of the end
static inline uint64_t bgzf_voff(uint64_t u, const uint64_t *coff, size_t nblk)
{
    const size_t b = (size_t)(u / BAM_BLK);
    return b >= nblk ? coff[nblk] << 16 : (coff[b] << 16 | (u - (uint64_t)b * BAM_BLK));
}
static inline void bai_finish(std::string &bai, const std::vector<size_t> &fix, const uint64_t *coff, size_t nblk)
{
    for (size_t p : fix) { uint64_t u; memcpy(&u, &bai[p], 8); const uint64_t v = bgzf_voff(u, coff, nblk); memcpy(&bai[p], &v, 8); }
}
#endif
