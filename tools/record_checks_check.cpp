// telr_amd/csrc/record_checks.h alone -- the record, call-list and signature refusals of telr_call_insertions, telr_genotype_insertions,
// telr_draft_contigs and telr_bridge_contigs, and the record refusals of telr_depth_medians -- as a program of its own for a sanitizer build (the Python tests load the engine library,
// which a sanitizer does not see into):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/record_checks_check tools/record_checks_check.cpp && tools/record_checks_check
// Every refusal with its full text, the edges of the CIGAR range (the C ABI cannot produce that one on a device: telr_result_from_arrays
// refuses it first), the order of a record's faults, the keys and supports a passing call list leaves, the strand coordinates of a
// forward and a reverse record, and the record of a read set (CutRec) field by field with its two refusals.  Exit status 0 and
// "record_checks: N checks ok" when every one is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../telr_amd/csrc/record_checks.h"

static int n_checks = 0, n_bad = 0;
static void expect(const char *what, const std::string &got, const std::string &want)
{
    ++n_checks;
    if (got != want) { ++n_bad; fprintf(stderr, "%s: got \"%s\", want \"%s\"\n", what, got.c_str(), want.c_str()); }
}
static void expect(const char *what, long long got, long long want)
{
    ++n_checks;
    if (got != want) { ++n_bad; fprintf(stderr, "%s: got %lld, want %lld\n", what, got, want); }
}

// a record that passes against 3 targets and 100 CIGAR words
static telr_aln good()
{
    telr_aln a; memset(&a, 0, sizeof(a));
    a.qid = 4; a.tid = 2; a.qlen = 1000; a.qs = 10; a.qe = 990; a.ts = 500; a.te = 1500; a.cigar_off = 40; a.n_cigar = 60;
    return a;
}
// "" when the record passes, else the reason
static std::string rec_why(const telr_aln &a, size_t i = 7, int32_t nt = 3, uint64_t ncig = 100)
{
    std::string why = "untouched";
    const bool ok = record_check(a, i, nt, ncig, &why);
    if (ok) { expect("a passing record leaves the reason alone", why, "untouched"); return ""; }
    return why;
}

struct Calls {
    std::vector<telr_ins_call> c; std::vector<int64_t> off; std::vector<int32_t> reads;
    std::vector<uint64_t> ckeys; std::vector<int32_t> support;       // exactly n: a store past them is the sanitizer's to find
};
static telr_ins_call call(int tid, int pos, int support) { telr_ins_call c; memset(&c, 0, sizeof(c)); c.tid = tid; c.pos = pos; c.support = support; return c; }
// "" when the list passes, else the reason; n_reads < 0: no bound
static std::string list_why(Calls &L, int64_t n_reads, bool with_support = true, bool null_reads = false)
{
    const int64_t n = (int64_t)L.c.size();
    L.ckeys.assign((size_t)n, 0); L.support.assign((size_t)n, -7);
    std::string why = "untouched";
    const bool ok = call_list_check(n, n ? L.c.data() : nullptr, n ? L.off.data() : nullptr, null_reads ? nullptr : L.reads.data(), 3, n_reads,
                                    L.ckeys.data(), with_support ? L.support.data() : nullptr, &why);
    return ok ? "" : why;
}
static Calls three()
{
    Calls L;
    L.c = {call(0, 100, 2), call(0, 101, 0), call(2, 5, 3)};
    L.off = {0, 2, 2, 5};
    L.reads = {3, 9, 0, 4, 8};
    return L;
}

int main()
{
    // ---- the record check
    telr_aln a = good();
    expect("a passing record", rec_why(a), "");
    a = good(); a.tid = -1;
    expect("tid -1", rec_why(a), "record 7: tid outside n_targets");
    a = good(); a.tid = 3;
    expect("tid = n_targets", rec_why(a), "record 7: tid outside n_targets");
    a = good(); a.tid = 2;
    expect("tid = n_targets - 1", rec_why(a), "");
    a = good(); a.qid = -1;
    expect("qid < 0", rec_why(a), "record 7: coordinates");
    a = good(); a.qlen = -1; a.qs = a.qe = 0;                     // (qs, qe kept inside their own rules: qe > qlen is the fault that remains)
    expect("qlen < 0", rec_why(a), "record 7: coordinates");
    a = good(); a.qs = -1;
    expect("qs < 0", rec_why(a), "record 7: coordinates");
    a = good(); a.qe = a.qs - 1;
    expect("qe < qs", rec_why(a), "record 7: coordinates");
    a = good(); a.qe = a.qlen + 1;
    expect("qe > qlen", rec_why(a), "record 7: coordinates");
    a = good(); a.ts = -1;
    expect("ts < 0", rec_why(a), "record 7: coordinates");
    a = good(); a.te = a.ts - 1;
    expect("te < ts", rec_why(a), "record 7: coordinates");
    a = good(); a.qs = a.qe = a.qlen = 0; a.ts = a.te = 0;
    expect("empty intervals pass", rec_why(a), "");
    a = good();                                                    // 40 + 60 = 100 words
    expect("CIGAR range ends at the word count", rec_why(a), "");
    a = good(); a.n_cigar = 61;
    expect("CIGAR range one past the word count", rec_why(a), "record 7: CIGAR range outside the result's array");
    a = good(); a.cigar_off = 41;
    expect("CIGAR offset one further", rec_why(a), "record 7: CIGAR range outside the result's array");
    a = good(); a.cigar_off = 100; a.n_cigar = 0;
    expect("no words at the array's end", rec_why(a), "");
    a = good(); a.cigar_off = 101; a.n_cigar = 0;
    expect("no words past the array's end", rec_why(a), "record 7: CIGAR range outside the result's array");
    a = good(); a.cigar_off = 0; a.n_cigar = 0;
    expect("an empty array", rec_why(a, 7, 3, 0), "");
    a = good(); a.n_cigar = -1;
    expect("negative n_cigar", rec_why(a), "record 7: CIGAR range outside the result's array");
    a = good(); a.cigar_off = -1;
    expect("negative cigar_off", rec_why(a), "record 7: CIGAR range outside the result's array");
    a = good(); a.cigar_off = INT64_MAX; a.n_cigar = INT32_MAX;   // the sum is below 2^64: it does not wrap to a small one
    expect("an offset near 2^63", rec_why(a), "record 7: CIGAR range outside the result's array");
    expect("an offset near 2^63, the largest word count", rec_why(a, 7, 3, UINT64_MAX), "");
    a = good(); a.cigar_off = INT64_MAX - 5; a.n_cigar = 5;
    expect("an offset near 2^63 ending at 2^63 - 1 words", rec_why(a, 7, 3, (uint64_t)INT64_MAX), "");
    expect("... and one word fewer", rec_why(a, 7, 3, (uint64_t)INT64_MAX - 1), "record 7: CIGAR range outside the result's array");
    a = good(); a.tid = 9; a.qs = -1; a.n_cigar = 1000;
    expect("three faults: tid first", rec_why(a), "record 7: tid outside n_targets");
    a = good(); a.qs = -1; a.n_cigar = 1000;
    expect("two faults: coordinates before the CIGAR range", rec_why(a), "record 7: coordinates");
    a = good(); a.tid = 3;
    expect("the index is the caller's", rec_why(a, 2147483648u), "record 2147483648: tid outside n_targets");
    expect("the index 0", rec_why(a, 0), "record 0: tid outside n_targets");

    // ---- a record as telr_depth_medians takes it: record_check, then te inside its target unless the record is secondary
    {
        const std::vector<int32_t> tlens = {10, 20, 1500};                 // exactly n_targets: a load past them is the sanitizer's to find
        auto depth = [&](const telr_aln &x) {
            std::string why = "untouched";
            const bool ok = depth_rec_check(x, 7, 3, tlens.data(), 100, &why);
            if (ok) { expect("a passing depth record leaves the reason alone", why, "untouched"); return std::string(""); }
            return why; };
        a = good();                                                    // te = 1500 = the target's length
        expect("depth: te = tlen", depth(a), "");
        a = good(); a.te = 1501;
        expect("depth: te = tlen + 1", depth(a), "record 7: te beyond its target's end");
        a = good(); a.te = 1501; a.flags = TELR_F_SECONDARY;
        expect("depth: a secondary record is not counted, its end not held to the target", depth(a), "");
        a = good(); a.te = 1501; a.flags = TELR_F_SECONDARY | TELR_F_REV;
        expect("depth: secondary among other flags", depth(a), "");
        a = good(); a.te = 1501; a.flags = TELR_F_REV;
        expect("depth: other flags do not excuse", depth(a), "record 7: te beyond its target's end");
        a = good(); a.tid = 0; a.ts = 0; a.te = 11;
        expect("depth: the length of the record's own target", depth(a), "record 7: te beyond its target's end");
        a = good(); a.tid = 0; a.ts = 10; a.te = 10;
        expect("depth: an empty record at the target's end", depth(a), "");
        a = good(); a.tid = 3; a.te = 1 << 30;
        expect("depth: tid first (no length is loaded for it)", depth(a), "record 7: tid outside n_targets");
        a = good(); a.tid = -1;
        expect("depth: tid -1", depth(a), "record 7: tid outside n_targets");
        a = good(); a.ts = -1; a.te = 1501;
        expect("depth: coordinates before the target's end", depth(a), "record 7: coordinates");
        a = good(); a.n_cigar = 61; a.te = 1501;
        expect("depth: the CIGAR range before the target's end", depth(a), "record 7: CIGAR range outside the result's array");
        a = good(); a.ts = -1; a.flags = TELR_F_SECONDARY;
        expect("depth: a secondary record is still held to record_check", depth(a), "record 7: coordinates");
    }
    // ---- the strand coordinates: forward as stored, mirrored in the read on TELR_F_REV
    {
        auto strand = [](int qs, int qe, int qlen, int flags) { telr_aln x = good(); x.qs = qs; x.qe = qe; x.qlen = qlen; x.flags = flags; return strand_coords(x); };
        StrandCoords s = strand(10, 990, 1000, 0);
        expect("forward rev", s.rev, 0); expect("forward qs", s.qs, 10); expect("forward qe", s.qe, 990);
        s = strand(10, 970, 1000, TELR_F_REV);
        expect("reverse rev", s.rev, 1); expect("reverse qs = qlen - qe", s.qs, 30); expect("reverse qe = qlen - qs", s.qe, 990);
        s = strand(0, 1000, 1000, 0);
        expect("forward, qs == 0", s.qs, 0); expect("forward, qe == qlen", s.qe, 1000);
        s = strand(0, 400, 1000, TELR_F_REV);
        expect("reverse, qs == 0: qe' == qlen", s.qe, 1000); expect("reverse, qs == 0: qs'", s.qs, 600);
        s = strand(400, 1000, 1000, TELR_F_REV);
        expect("reverse, qe == qlen: qs' == 0", s.qs, 0); expect("reverse, qe == qlen: qe'", s.qe, 600);
        s = strand(10, 970, 1000, TELR_F_REV | TELR_F_SECONDARY);
        expect("other flags do not count", s.rev, 1); expect("... qs", s.qs, 30);
        s = strand(10, 970, 1000, TELR_F_SECONDARY);
        expect("secondary alone is forward", s.rev, 0); expect("... qs", s.qs, 10);
    }
    // ---- a record against a read set (telr_draft_contigs, telr_bridge_contigs): 5 reads, read 4 of 1000 bases
    {
        const std::vector<int32_t> lens = {7, 7, 7, 7, 1000};            // exactly n_reads: a load past them is the sanitizer's to find
        auto cut = [&](const telr_aln &x, CutRec *e, int32_t n_reads = 5) {
            std::string why = "untouched";
            return cut_rec_check(x, 7, 3, 100, n_reads, lens.data(), e, &why) ? std::string("") : why; };
        static_assert(sizeof(CutRec) == 40, "the device layout");
        for (int rev = 0; rev < 2; ++rev) {
            a = good(); a.qs = 10; a.qe = 970; a.flags = rev ? TELR_F_REV : 0;
            CutRec e; memset(&e, 0xff, sizeof(e));
            expect("a passing record of the set", cut(a, &e), "");
            expect("ts", e.ts, 500); expect("te", e.te, 1500); expect("qs", e.qs, rev ? 30 : 10); expect("qe", e.qe, rev ? 990 : 970);
            expect("qlen", e.qlen, 1000); expect("rev", e.rev, rev); expect("n_cigar", e.n_cigar, 60); expect("pad", e.pad, 0);
            expect("cigar_off", (long long)e.cigar_off, 40);
        }
        CutRec e;
        a = good(); a.qid = 5;
        expect("qid = n_reads", cut(a, &e), "record 7: qid outside the read set");
        a = good();
        expect("qid = n_reads - 1", cut(a, &e), "");
        expect("an empty read set", cut(a, &e, 0), "record 7: qid outside the read set");
        a = good(); a.qlen = 1001;
        expect("qlen one more than the read", cut(a, &e), "record 7: qlen is not the length of its read in the read set");
        a = good(); a.qid = 3;
        expect("the length of another read", cut(a, &e), "record 7: qlen is not the length of its read in the read set");
        a = good(); a.qid = 5; a.qlen = 1001;
        expect("two faults: the read id before the length (which is not loaded)", cut(a, &e), "record 7: qid outside the read set");
        a = good(); a.qid = 5; a.n_cigar = 61;
        expect("two faults: the record's own before the read set's", cut(a, &e), "record 7: CIGAR range outside the result's array");
        a = good(); a.qid = -1;
        expect("a negative qid is the record's fault", cut(a, &e), "record 7: coordinates");
    }
    // ---- the call-list check
    {
        Calls L;
        expect("no calls", list_why(L, -1), "");
        expect("no calls, bounded", list_why(L, 10), "");
        expect("no calls, no support", list_why(L, -1, false), "");
    }
    {
        Calls L; L.c = {call(1, 0, 0)}; L.off = {0, 0};
        expect("one call, no reads", list_why(L, -1, true, true), "");
        expect("one call, no reads, bounded by an empty set", list_why(L, 0, false, true), "");
        expect("its key", (long long)L.ckeys[0], 1LL << 32);
    }
    {
        Calls L = three();
        expect("three calls", list_why(L, -1), "");
        expect("key 0", (long long)L.ckeys[0], 100); expect("key 1", (long long)L.ckeys[1], 101); expect("key 2", (long long)L.ckeys[2], (2LL << 32) | 5);
        expect("support 0", L.support[0], 2); expect("support 1", L.support[1], 0); expect("support 2", L.support[2], 3);
        expect("three calls, bound 10", list_why(L, 10, false), "");
        expect("keys without support", (long long)L.ckeys[2], (2LL << 32) | 5);
        expect("the largest read id + 1 as the bound", list_why(L, 10), ""); expect("support filled in bounded mode too", L.support[2], 3);
        expect("read id = the bound", list_why(L, 9), "call 0: read id outside the read set");
        L = three(); L.c[2].pos = 0x7fffffff;
        expect("the largest pos", list_why(L, -1), ""); expect("its key", (long long)L.ckeys[2], (2LL << 32) | 0x7fffffffLL);
    }
    {
        Calls L = three(); L.c[0].tid = -1;
        expect("call tid -1", list_why(L, -1), "call 0: tid outside n_targets");
        L = three(); L.c[2].tid = 3;
        expect("call tid = n_targets", list_why(L, -1), "call 2: tid outside n_targets");
        L = three(); L.c[1].pos = -1;
        expect("negative pos", list_why(L, -1), "call 1: negative pos");
        L = three(); L.c[1].pos = 100;
        expect("equal keys", list_why(L, -1), "call 1: calls not strictly ascending by (tid, pos)");
        L = three(); L.c[1].pos = 99;
        expect("pos descends", list_why(L, -1), "call 1: calls not strictly ascending by (tid, pos)");
        L = three(); L.c[1].tid = 1; L.c[2].tid = 0; L.c[2].pos = 5000;
        expect("tid descends", list_why(L, -1), "call 2: calls not strictly ascending by (tid, pos)");
        L = three(); L.off[0] = 1;
        expect("read_off[0] is not 0", list_why(L, -1), "read_off[0] is not 0");
        L = three(); L.off = {0, 2, 1, 5};
        expect("an offset descends", list_why(L, -1), "call 1: read offsets descend");
        L = three();
        expect("null reads, a list that is not empty", list_why(L, -1, true, true), "null reads");
        L = three(); L.off = {0, 0, 0, 0};
        expect("null reads, every list empty", list_why(L, 10, true, true), "");
        L = three(); L.reads = {3, 3, 0, 4, 8};
        expect("an equal read id", list_why(L, -1), "call 0: read list not ascending");
        L = three(); L.reads = {3, 9, 0, 8, 4};
        expect("a descending read id", list_why(L, 10), "call 2: read list not ascending");
        L = three(); L.reads = {9, 3, 0, 4, 8};
        expect("a descending read id in the first list", list_why(L, -1), "call 0: read list not ascending");
        L = three(); L.reads = {3, 9, -1, 4, 8};
        expect("read id -1, no bound", list_why(L, -1), "call 2: negative read id");
        expect("read id -1, bounded", list_why(L, 10), "call 2: read id outside the read set");
        L = three(); L.reads = {3, 9, 0, 4, 10};
        expect("read id = the bound, last", list_why(L, 10), "call 2: read id outside the read set");
        expect("the same without a bound", list_why(L, -1), "");
        L = three(); L.c[2].tid = 3; L.off[0] = 1;
        expect("the calls before the offsets", list_why(L, -1), "call 2: tid outside n_targets");
        L = three(); L.reads = {3, 9, 0, -1, -2};
        expect("the id before the order", list_why(L, -1), "call 2: negative read id");
    }
    // ---- the signature array (telr_draft_contigs, telr_bridge_contigs): two records of read 4, one of read 5; 3 targets, 6 reads
    {
        std::vector<telr_aln> recs(3, good());
        recs[2].qid = 5;
        auto sig = [](int tid, int pos, int qid, int kind, int rec, int mate) {
            telr_ins_sig s; memset(&s, 0, sizeof(s)); s.tid = tid; s.pos = pos; s.qid = qid; s.kind = kind; s.rec = rec; s.mate = mate; return s; };
        auto sig_why = [&](const std::vector<telr_ins_sig> &S, int32_t n_reads = 6) {
            std::string why = "untouched";
            return sig_list_check((int64_t)S.size(), S.empty() ? nullptr : S.data(), recs.data(), recs.size(), 3, n_reads, &why) ? std::string("") : why; };
        const std::vector<telr_ins_sig> ok = {sig(0, 10, 4, 0, 0, -1), sig(0, 10, 4, 1, 0, 1), sig(2, 5, 5, 2, 2, -1)};
        expect("a passing signature array", sig_why(ok), "");
        expect("no signatures", sig_why({}), "");
        std::vector<telr_ins_sig> S = ok; S[1].tid = 3;
        expect("sig tid = n_targets", sig_why(S), "signature 1: tid outside n_targets");
        S = ok; S[0].tid = -1;
        expect("sig tid -1", sig_why(S), "signature 0: tid outside n_targets");
        S = ok; S[2].pos = -1;
        expect("sig negative pos", sig_why(S), "signature 2: negative pos");
        S = ok; S[0].rec = 3;
        expect("sig rec = n", sig_why(S), "signature 0: rec outside the records");
        S = ok; S[0].rec = -1;
        expect("sig rec -1", sig_why(S), "signature 0: rec outside the records");
        S = ok; S[1].mate = 3;
        expect("sig mate = n", sig_why(S), "signature 1: mate outside the records");
        S = ok; S[1].mate = -1;
        expect("sig mate -1 on a split", sig_why(S), "signature 1: mate outside the records");
        S = ok; S[0].mate = 99;
        expect("the mate of a kind 0 is not read", sig_why(S), "");
        expect("sig qid = n_reads", sig_why(ok, 5), "signature 2: qid outside the read set");
        S = ok; S[0].qid = 5;
        expect("sig qid of another read", sig_why(S), "signature 0: qid is not its records' read");
        S = ok; S[1].mate = 2;
        expect("sig mate of another read", sig_why(S), "signature 1: qid is not its records' read");
        S = {ok[2], ok[0]};
        expect("sigs descend", sig_why(S), "signature 1: signatures not ascending by (tid, pos)");
        S = {ok[1], ok[0]};
        expect("equal keys pass", sig_why(S), "");
    }
    if (n_bad) { fprintf(stderr, "record_checks: %d of %d checks FAILED\n", n_bad, n_checks); return 1; }
    printf("record_checks: %d checks ok\n", n_checks);
    return 0;
}
