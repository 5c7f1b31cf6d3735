// telr_amd/csrc/sam_records.h alone, on the hand-derived cases of tests/test_bam_reference.py, as a program of its own for a
// sanitizer build (the Python tests load the engine library, which a sanitizer does not see into):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/sam_records_check tools/sam_records_check.cpp && tools/sam_records_check
// Layout, walk, SA, both headers and the index builder against strings written out here.  Exit status 0 and
// "sam records: N checks ok" when every one is the expected one.
#include <cstdio>
#include <string>
#include <vector>
#include "../telr_amd/csrc/sam_records.h"

static int n_checks = 0, n_bad = 0;
static void expect(const char *what, const std::string &got, const std::string &want)
{
    ++n_checks;
    if (got != want) { ++n_bad; fprintf(stderr, "%s:\n  got  %s\n  want %s\n", what, got.c_str(), want.c_str()); }
}
static std::string num(long long v) { return std::to_string(v); }
static std::string hex(const std::string &s) { std::string o; char b[4]; for (unsigned char c : s) { snprintf(b, sizeof(b), "%02x", c); o += b; } return o; }
static std::string le32(uint32_t v) { std::string s; put32(s, v); return s; }

static std::vector<uint32_t> ops_of(const char *cigar)
{
    std::vector<uint32_t> v; uint32_t n = 0;
    for (const char *p = cigar; *p; ++p) { if (*p >= '0' && *p <= '9') n = n * 10 + (uint32_t)(*p - '0'); else { v.push_back(n << 4 | (*p == 'M' ? 0u : *p == 'I' ? 1u : 2u)); n = 0; } }
    return v;
}
static telr_aln aln_of(int qid, int tid, int qlen, int qs, int qe, int ts, const std::vector<uint32_t> &ops, int flags, int64_t cigar_off, int mapq)
{
    telr_aln a; memset(&a, 0, sizeof(a));
    a.qid = qid; a.tid = tid; a.qlen = qlen; a.qs = qs; a.qe = qe; a.ts = ts; a.te = ts; a.flags = flags; a.n_cigar = (int)ops.size(); a.cigar_off = cigar_off; a.mapq = mapq;
    for (uint32_t c : ops) if ((c & 15) != 1) a.te += (int)(c >> 4);
    return a;
}
static std::string strand(const std::string &read, bool rev)
{
    if (!rev) return read;
    std::string rc(read.size(), 'N');
    for (size_t x = 0; x < read.size(); ++x) rc[x] = COMP_TAB[(unsigned char)read[read.size() - 1 - x]];
    return rc;
}
// the record's CIGAR column and its SEQ as 4-bit codes, from the layout
static std::string rec_cigar(const RecLayout &L, const std::vector<uint32_t> &ops)
{
    std::string s; const char c = L.hard ? 'H' : 'S';
    if (L.clip5) s += num(L.clip5) + c;
    for (uint32_t o : ops) s += num(o >> 4) + "MID"[o & 15];
    if (L.clip3) s += num(L.clip3) + c;
    return s;
}
static std::string seq_hex(const RecLayout &L, const std::string &qstr)
{
    std::string s;
    for (int x = 0; x < L.l_seq; x += 2) s += (char)(nt16(qstr[L.seq_lo + x]) << 4 | (x + 1 < L.l_seq ? nt16(qstr[L.seq_lo + x + 1]) : 0));
    return hex(s);
}

// ---- one record with TELR_SAM_MD | TELR_SAM_CS | TELR_SAM_SOFTCLIP (the table of test_hand_derived_records) ----
struct Hand { const char *name; std::string target; int ts; std::string read; int qs, qe, rev; const char *cigar, *md, *cs; int nm; std::string seq; const char *rec_cigar; };
static void hand_records()
{
    const std::string T20 = "ACGTACGTACGTACGTACGT", C100 = std::string(100, 'C'), C19 = std::string(19, 'C');
    std::string seq120; for (int i = 0; i < 60; ++i) seq120 += i == 50 ? "42" : "22";
    const std::vector<Hand> hand = {
        { "perfect", T20, 0, "ACGTACGT", 0, 8, 0, "8M", "8", ":8", 0, "12481248", "8M" },
        { "one mismatch", T20, 0, "ACGAACGT", 0, 8, 0, "8M", "3T4", ":3*ta:4", 1, "12411248", "8M" },
        { "first column", T20, 0, "TCGTACGT", 0, 8, 0, "8M", "0A7", "*at:7", 1, "82481248", "8M" },
        { "last column", T20, 0, "ACGTACGA", 0, 8, 0, "8M", "7T0", ":7*ta", 1, "12481241", "8M" },
        { "first and last", T20, 0, "TCGTACGA", 0, 8, 0, "8M", "0A6T0", "*at:6*ta", 2, "82481241", "8M" },
        { "adjacent mismatches", T20, 0, "ACTAACGT", 0, 8, 0, "8M", "2G0T4", ":2*gt*ta:4", 2, "12811248", "8M" },
        { "every column", T20, 0, "TTTA", 0, 4, 0, "4M", "0A0C0G0T0", "*at*ct*gt*ta", 4, "8881", "4M" },
        { "deletion", T20, 0, "ACGTGT", 0, 6, 0, "4M2D2M", "4^AC2", ":4-ac:2", 2, "124848", "4M2D2M" },
        { "deletion then mismatch", T20, 0, "ACGTTT", 0, 6, 0, "4M2D2M", "4^AC0G1", ":4-ac*gt:1", 3, "124888", "4M2D2M" },
        { "mismatch then deletion", T20, 0, "ACGAGT", 0, 6, 0, "4M2D2M", "3T0^AC2", ":3*ta-ac:2", 3, "124148", "4M2D2M" },
        { "insertion", T20, 0, "ACGTTTACGT", 0, 10, 0, "4M2I4M", "8", ":4+tt:4", 2, "1248881248", "4M2I4M" },
        { "M of length 1", T20, 0, "ATTCGT", 0, 6, 0, "1M2I3M", "4", ":1+tt:3", 2, "188248", "1M2I3M" },
        { "D then I", T20, 0, "ACGTGGGT", 0, 8, 0, "4M2D2I2M", "4^AC2", ":4-ac+gg:2", 4, "12484448", "4M2D2I2M" },
        { "I then D", T20, 0, "ACGTGGGT", 0, 8, 0, "4M2I2D2M", "4^AC2", ":4+gg-ac:2", 4, "12484448", "4M2I2D2M" },
        { "D I D", T20, 0, "ACGTGGT", 0, 7, 0, "4M1D1I1D2M", "4^A0^C2", ":4-a+g-c:2", 3, "12484480", "4M1D1I1D2M" },
        { "N in the read", T20, 0, "ACNTACGT", 0, 8, 0, "8M", "2G5", ":2*gn:5", 1, "12f81248", "8M" },
        { "N in the target", "ACNTACGTAC", 0, "ACGTACGT", 0, 8, 0, "8M", "2N5", ":2*ng:5", 1, "12481248", "8M" },
        { "N in both", "ACNTACGTAC", 0, "ACNTACGT", 0, 8, 0, "8M", "2N5", ":2*nn:5", 1, "12f81248", "8M" },
        { "lower case and IUPAC", T20, 0, "acgRacgt", 0, 8, 0, "8M", "3T4", ":3*tn:4", 1, "124f1248", "8M" },
        { "odd length", T20, 0, "ACG", 0, 3, 0, "3M", "3", ":3", 0, "1240", "3M" },
        { "one base", T20, 3, "T", 0, 1, 0, "1M", "1", ":1", 0, "80", "1M" },
        { "start inside the target", T20, 4, "ACGTAC", 0, 6, 0, "6M", "6", ":6", 0, "124812", "6M" },
        { "reverse strand", T20, 0, "ACGTTCGT", 0, 8, 1, "8M", "3T4", ":3*ta:4", 1, "12411248", "8M" },
        { "soft clips", T20, 0, "GGACGTACGTT", 2, 10, 0, "8M", "8", ":8", 0, "441248124880", "2S8M1S" },
        { "soft clips, reverse", T20, 0, "GGACGTACGTT", 2, 10, 1, "8M", "8", ":8", 0, "112481248220", "1S8M2S" },
        { "5' clip only", T20, 0, "GGACGTACGT", 2, 10, 0, "8M", "8", ":8", 0, "4412481248", "2S8M" },
        { "3' clip only", T20, 0, "ACGTACGTT", 0, 8, 0, "8M", "8", ":8", 0, "1248124880", "8M1S" },
        { "MD example of the specification", "CCCCCCCCCCAGGGGGACTTTTTT", 0, "CCCCCCCCCCGGGGGGTTTTTT", 0, 22, 0, "16M2D6M", "10A5^AC6", ":10*ag:5-ac:6", 3, "2222222222444444888888", "16M2D6M" },
        { "numbers of three digits", C100 + "A" + C19, 0, C100 + "G" + C19, 0, 120, 0, "120M", "100A19", ":100*ag:19", 1, seq120, "120M" },
    };
    const int flags = TELR_SAM_MD | TELR_SAM_CS | TELR_SAM_SOFTCLIP;
    for (const Hand &h : hand) {
        std::vector<uint32_t> ops = ops_of(h.cigar);
        ops.shrink_to_fit();                              // no slack behind the last operation or base: a walk that reads past it is seen
        const telr_aln a = aln_of(0, 0, (int)h.read.size(), h.qs, h.qe, h.ts, ops, 1 | (h.rev ? TELR_F_REV : 0), 0, 60);
        const RecLayout L = rec_layout(a, a.qlen, flags);
        std::string qstr = strand(h.read, h.rev != 0), target = h.target.substr(0, (size_t)a.te);
        qstr.shrink_to_fit(); target.shrink_to_fit();
        std::string md = "MD=", cs = "cs=";              // the walk appends
        const int nm = aln_walk(qstr.data(), target.data(), ops.data(), a.n_cigar, L.clip5, a.ts, flags, md, cs);
        const std::string got = "flag " + num(L.flag) + " " + rec_cigar(L, ops) + " " + seq_hex(L, qstr) + " NM " + num(nm) + " " + md + " " + cs + " key " + num(L.key);
        const std::string want = "flag " + num(h.rev ? 16 : 0) + " " + h.rec_cigar + " " + h.seq + " NM " + num(h.nm) + " MD=" + h.md + " cs=" + h.cs + " key " + num((1LL << 33) | (long long)h.ts << 1 | h.rev);
        expect(h.name, got, want);
        // without the bits: NM alone, nothing appended
        std::string m2, c2;
        expect(h.name, num(aln_walk(qstr.data(), target.data(), ops.data(), a.n_cigar, L.clip5, a.ts, 0, m2, c2)) + "|" + m2 + "|" + c2, num(h.nm) + "||");
    }
}

// ---- a read of two pieces with a secondary, and a reverse primary with a forward supplementary: layout, SA, order ----
static void pieces()
{
    const char *tn[2] = { "t0", "t1" };
    // read "two" = ACGTACGT + TACGTAC: 0-8 forward on t0 at 0 (primary), the same at 4 (secondary), 8-15 reverse on t1 at 2 (supplementary)
    std::vector<uint32_t> cig = { 8u << 4, 8u << 4, 7u << 4 };
    std::vector<telr_aln> al = { aln_of(0, 0, 15, 0, 8, 0, { 8u << 4 }, TELR_F_PRIMARY, 0, 60), aln_of(0, 0, 15, 0, 8, 4, { 8u << 4 }, TELR_F_SECONDARY, 1, 0),
                                 aln_of(0, 1, 15, 8, 15, 2, { 7u << 4 }, TELR_F_SUPPL | TELR_F_REV, 2, 30) };
    cig.shrink_to_fit(); al.shrink_to_fit();
    auto lay = [&](const RecLayout &L, const telr_aln &a) { return "flag " + num(L.flag) + " " + rec_cigar(L, std::vector<uint32_t>(cig.begin() + a.cigar_off, cig.begin() + a.cigar_off + a.n_cigar)) +
                                                                   " seq " + num(L.seq_lo) + "+" + num(L.l_seq); };
    expect("primary, soft", lay(rec_layout(al[0], 15, TELR_SAM_SOFTCLIP), al[0]), "flag 0 8M7S seq 0+15");
    expect("primary, hard", lay(rec_layout(al[0], 15, 0), al[0]), "flag 0 8M7S seq 0+15");
    expect("secondary", lay(rec_layout(al[1], 15, 0), al[1]), "flag 256 8M7S seq 0+0");
    expect("supplementary, soft", lay(rec_layout(al[2], 15, TELR_SAM_SOFTCLIP), al[2]), "flag 2064 7M8S seq 0+15");
    expect("supplementary, hard", lay(rec_layout(al[2], 15, 0), al[2]), "flag 2064 7M8H seq 0+7");
    const std::string rc = strand("ACGTACGTTACGTAC", true);
    expect("reverse strand of the read", rc, "GTACGTAACGTACGT");
    expect("supplementary SEQ, hard", seq_hex(rec_layout(al[2], 15, 0), rc), "48124810");
    std::string sa;
    sa_text(al.data(), al.size(), 0, 15, cig.data(), tn, sa); expect("SA of the primary", sa, "t1,3,-,7M8S,30,0;");
    sa.clear(); sa_text(al.data(), al.size(), 2, 15, cig.data(), tn, sa); expect("SA of the supplementary", sa, "t0,1,+,8M7S,60,0;");
    sa.clear(); sa_text(al.data(), 2, 0, 15, cig.data(), tn, sa); expect("SA beside a secondary alone", sa, "");
    // coordinate order: (t0, 0, +) < (t0, 4, +) < (t1, 0, +) < (t1, 2, -) < unmapped; at one position forward before reverse
    const telr_aln z = aln_of(2, 1, 4, 0, 4, 0, { 4u << 4 }, TELR_F_PRIMARY, 0, 60), zr = aln_of(2, 1, 4, 0, 4, 0, { 4u << 4 }, TELR_F_PRIMARY | TELR_F_REV, 0, 60);
    const int64_t k[6] = { rec_layout(al[0], 15, 0).key, rec_layout(al[1], 15, 0).key, rec_layout(z, 4, 0).key, rec_layout(zr, 4, 0).key, rec_layout(al[2], 15, 0).key, SAM_KEY_UNMAPPED };
    std::string ord; for (int i = 0; i + 1 < 6; ++i) ord += k[i] < k[i + 1] ? '<' : '!';
    expect("sort keys", ord, "<<<<<");

    // read "rv" = ACGAACG + ACGTA on ACGTACGTACGTACGTACGT: 0-7 reverse at 1 with one mismatch (primary), 7-12 forward at 12 (supplementary).
    // Its reverse strand is TACGTCGTTCGT: 5 clipped bases, then CGTTCGT against CGTACGT.
    const char *tg[1] = { "tg" };
    std::vector<uint32_t> cg2 = { 7u << 4, 5u << 4 };
    std::vector<telr_aln> rv = { aln_of(0, 0, 12, 0, 7, 1, { 7u << 4 }, TELR_F_PRIMARY | TELR_F_REV, 0, 60), aln_of(0, 0, 12, 7, 12, 12, { 5u << 4 }, TELR_F_SUPPL, 1, 30) };
    rv[0].mlen = 6; rv[0].blen = 7; rv[1].mlen = 5; rv[1].blen = 5;
    const std::string T20 = "ACGTACGTACGTACGTACGT", q = strand("ACGAACGACGTA", true);
    expect("reverse strand of rv", q, "TACGTCGTTCGT");
    const int fl = TELR_SAM_MD | TELR_SAM_CS | TELR_SAM_SOFTCLIP;
    const RecLayout L = rec_layout(rv[0], 12, fl);
    std::string md, cs;
    const int nm = aln_walk(q.data(), T20.data(), cg2.data(), 1, L.clip5, rv[0].ts, fl, md, cs);
    sa.clear(); sa_text(rv.data(), 2, 0, 12, cg2.data(), tg, sa);
    expect("reverse primary", "flag " + num(L.flag) + " " + rec_cigar(L, { 7u << 4 }) + " NM " + num(nm) + " MD " + md + " cs " + cs + " SA " + sa, "flag 16 5S7M NM 1 MD 3A3 cs :3*at:3 SA tg,13,+,7S5M,30,0;");
    sa.clear(); sa_text(rv.data(), 2, 1, 12, cg2.data(), tg, sa);
    expect("SA naming the reverse primary", sa, "tg,2,-,5S7M,60,1;");
}

// ---- the header text and the head of the BAM stream ----
static void headers()
{
    const char *tn[1] = { "chr1" }; const int32_t tl[1] = { 20 };
    const std::string sq_rg_pg = "@SQ\tSN:chr1\tLN:20\n@RG\tID:g1\tSM:sm\tLB:lb\n@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:cmd -x\n";
    expect("header, sorted", sam_header_text(true, 1, tn, tl, "g1", "sm", "lb", "cmd -x"), "@HD\tVN:1.6\tSO:coordinate\n" + sq_rg_pg);
    expect("header, unsorted", sam_header_text(false, 1, tn, tl, "g1", "sm", "lb", "cmd -x"), "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + sq_rg_pg);
    expect("header, defaults", sam_header_text(true, 1, tn, tl, "g1", nullptr, nullptr, nullptr),
           "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:20\n@RG\tID:g1\tSM:g1\tLB:lib\n@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:telr_map\n");
    expect("header, no read group, no target", sam_header_text(true, 0, nullptr, nullptr, nullptr, nullptr, nullptr, "x"), "@HD\tVN:1.6\tSO:coordinate\n@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:x\n");
    const std::string text = "@HD\tVN:1.6\tSO:coordinate\n" + sq_rg_pg;
    expect("BAM head", hex(bam_header(1, tn, tl, "g1", "sm", "lb", "cmd -x")), hex(std::string("BAM\1", 4) + le32(112) + text + le32(1) + le32(5) + std::string("chr1\0", 5) + le32(20)));
    expect("BGZF EOF block", hex(std::string((const char*)BGZF_EOF, sizeof(BGZF_EOF))), "1f8b08040000000000ff0600424302001b0003000000000000000000");
}

// ---- the index ----
// a .bai as text: "refs=2; bins=3: 585[(300,460)] ... 37450[(200,540)(3,0)] lin=3: 200 300 460; ... no_coor=1" ("?" where it does not parse)
static std::string bai_dump(const std::string &b)
{
    size_t p = 0; bool ok = true;
    auto g32 = [&]() { uint32_t v = 0; if (p + 4 <= b.size()) memcpy(&v, &b[p], 4); else ok = false; p += 4; return v; };
    auto g64 = [&]() { uint64_t v = 0; if (p + 8 <= b.size()) memcpy(&v, &b[p], 8); else ok = false; p += 8; return v; };
    if (b.compare(0, 4, "BAI\1") != 0) return "?";
    p = 4;
    const uint32_t n_ref = g32();
    std::string s = "refs=" + num(n_ref) + ";";
    for (uint32_t t = 0; t < n_ref && ok; ++t) {
        const uint32_t nb = g32(); s += " bins=" + num(nb) + ":";
        for (uint32_t i = 0; i < nb && ok; ++i) {
            const uint32_t bin = g32(), nc = g32(); s += " " + num(bin) + "[";
            for (uint32_t c = 0; c < nc && ok; ++c) { const uint64_t x = g64(), y = g64(); s += "(" + num((long long)x) + "," + num((long long)y) + ")"; }
            s += "]";
        }
        const uint32_t nl = g32(); s += " lin=" + num(nl) + ":";
        for (uint32_t i = 0; i < nl && ok; ++i) s += " " + num((long long)g64());
        s += ";";
    }
    s += " no_coor=" + num((long long)g64());
    return ok && p == b.size() ? s : s + " ?";
}
static void index()
{
    std::string bai; std::vector<size_t> fix;
    auto ublk = [](uint64_t u) { return u / BAM_BLK; };
    auto vblk = [](uint64_t v) { return v >> 16; };
    // test_hand_derived_index: three records on a target of 40,000 bases, one on the next, an unmapped read; the records stand at
    // 200, 300, 460 and 540 of the stream, which ends at 610
    {
        std::vector<BaiEntry> e = { { 0, 10, 60, 200, 300 }, { 0, 16300, 16400, 300, 460 }, { 0, 32768, 32778, 460, 540 }, { 1, 0, 8, 540, 610 } };
        e.shrink_to_fit();
        const int32_t tl[2] = { 40000, 20 };
        const bool ok = bai_build(e.size(), [&](size_t i) { return e[i]; }, ublk, 1, 2, tl, bai, &fix);
        expect("index of four records", (ok ? "ok " : "not in order ") + bai_dump(bai),
               "ok refs=2; bins=4: 585[(300,460)] 4681[(200,300)] 4683[(460,540)] 37450[(200,540)(3,0)] lin=3: 200 300 460; bins=2: 4681[(540,610)] 37450[(540,610)(1,0)] lin=1: 540; no_coor=1");
        expect("offset fields of four records", num((long long)fix.size()), "16");
    }
    // six records over two targets; the stream is cut at 65,280: the first two records of bin 4681 end and begin in block 0 and
    // are one chunk, the third begins in block 1 behind a record of bin 585 and is a chunk of its own.  The last record has no
    // reference base (te == ts): the bin and the window of [16384, 16385).  Blocks at 0 and 20,000 of the file, which ends at 25,000.
    {
        std::vector<BaiEntry> e = { { 0, 0, 100, 1000, 2000 }, { 0, 50, 150, 2000, 3000 }, { 0, 100, 20000, 3000, 70000 }, { 0, 150, 250, 70000, 71000 },
                                    { 1, 5, 6, 71000, 71500 }, { 1, 16384, 16384, 71500, 72000 } };
        e.shrink_to_fit();
        const int32_t tl[2] = { 40000, 20000 };
        const bool ok = bai_build(e.size(), [&](size_t i) { return e[i]; }, ublk, 2, 2, tl, bai, &fix);
        expect("index of six records, stream offsets", (ok ? "ok " : "not in order ") + bai_dump(bai),
               "ok refs=2; bins=3: 585[(3000,70000)] 4681[(1000,3000)(70000,71000)] 37450[(1000,71000)(4,0)] lin=2: 1000 3000;"
               " bins=3: 4681[(71000,71500)] 4682[(71500,72000)] 37450[(71000,72000)(2,0)] lin=2: 71000 71500; no_coor=2");
        expect("offset fields of six records", num((long long)fix.size()), "18");
        const uint64_t coff[3] = { 0, 20000, 25000 };
        bai_finish(bai, fix, coff, 2);
        const std::string want = "ok refs=2; bins=3: 585[(3000,1310724720)] 4681[(1000,3000)(1310724720,1310725720)] 37450[(1000,1310725720)(4,0)] lin=2: 1000 3000;"
                                 " bins=3: 4681[(1310725720,1310726220)] 4682[(1310726220,1310726720)] 37450[(1310725720,1310726720)(2,0)] lin=2: 1310725720 1310726220; no_coor=2";
        expect("index of six records, file offsets", "ok " + bai_dump(bai), want);
        // the same entries given as virtual offsets, no fix list: the same bytes
        std::vector<BaiEntry> v = e;
        for (BaiEntry &x : v) { x.beg = bgzf_voff(x.beg, coff, 2); x.end = bgzf_voff(x.end, coff, 2); }
        std::string bai2;
        const bool ok2 = bai_build(v.size(), [&](size_t i) { return v[i]; }, vblk, 2, 2, tl, bai2, nullptr);
        expect("index of six records, virtual offsets", (ok2 ? "ok " : "not in order ") + bai_dump(bai2), want);
        expect("the two ways, byte for byte", hex(bai2), hex(bai));
        expect("the end of the stream on a block boundary", num((long long)bgzf_voff(2 * BAM_BLK, coff, 2)), num(25000LL << 16));
        // not in file order: a reference after a later one; a reference beyond the table
        std::swap(v[3], v[4]);
        expect("references out of order", bai_build(v.size(), [&](size_t i) { return v[i]; }, vblk, 0, 2, tl, bai2, nullptr) ? "ok" : "refused", "refused");
        expect("a reference beyond the table", bai_build(e.size(), [&](size_t i) { return e[i]; }, ublk, 0, 1, tl, bai2, nullptr) ? "ok" : "refused", "refused");
    }
    // no record at all
    {
        const int32_t tl[1] = { 100 };
        const bool ok = bai_build(0, [](size_t) { return BaiEntry{ 0, 0, 0, 0, 0 }; }, ublk, 3, 1, tl, bai, &fix);
        expect("index without records", (ok ? "ok " : "not in order ") + bai_dump(bai) + " fix " + num((long long)fix.size()), "ok refs=1; bins=0: lin=0:; no_coor=3 fix 0");
    }
}

int main()
{
    hand_records();
    pieces();
    headers();
    index();
    if (n_bad) { fprintf(stderr, "sam records: %d of %d checks differ\n", n_bad, n_checks); return 1; }
    printf("sam records: %d checks ok\n", n_checks);
    return 0;
}
