// record_checks.h — what the call stages (telr_call_insertions, telr_genotype_insertions, telr_draft_contigs, telr_bridge_contigs;
// DESIGN.md 5.10 - 5.12, 5.18) and telr_depth_medians refuse in a result's records, in a call list and in a signature array, stated once, with a record's strand
// coordinates (strand_coords) and the record that the two stages which cut reads at reference coordinates upload (CutRec).  These checks are
// all that stands between a caller's arrays and the kernels that index with them.  Plain C++: no HIP call and no type of the engine's own, so they are pinned on a CPU and run under the
// sanitizers from a stand-alone program (tools/record_checks_check.cpp).  The reason comes back in a std::string; the entry's name in
// front of it ("telr_call_insertions: " ...) and the TELR_E_RANGE limits on the counts stay with the callers.
//
// Two neighbours are separate contracts on purpose.  cons_first_bad_record (pileup.hip.h) answers yes or no without a reason, walks
// every op of every CIGAR against the query and target lengths and runs on the host's threads.  part_merge_check (part_plan.h) holds a
// part's records to that part's own word count, its tid map and the query order, in its own words.
#ifndef TELR_RECORD_CHECKS_H
#define TELR_RECORD_CHECKS_H
#include <cstdint>
#include <string>
#include "../../include/telr_hip.h"

// Record i of a result of ncig CIGAR words against n_targets targets: true, or false with "record i: <what>" in *why.  The first
// fault in the order tid, coordinates, CIGAR range is the one reported.  One call per record, from the caller's own loop.
static inline bool record_check(const telr_aln &a, size_t i, int32_t n_targets, uint64_t ncig, std::string *why)
{
    const char *what = nullptr;
    if (a.tid < 0 || a.tid >= n_targets) what = "tid outside n_targets";
    else if (a.qid < 0 || a.qlen < 0 || a.qs < 0 || a.qe < a.qs || a.qe > a.qlen || a.ts < 0 || a.te < a.ts) what = "coordinates";
    else if (a.n_cigar < 0 || a.cigar_off < 0 || (uint64_t)a.cigar_off + (uint64_t)a.n_cigar > ncig) what = "CIGAR range outside the result's array";
    if (what) *why = "record " + std::to_string(i) + ": " + what;
    return !what;
}

// Record i as telr_depth_medians takes it, against targets of lengths target_len (none negative): record_check, then -- unless the
// record is secondary, which the depth does not count -- its end inside its target.  True, or false with "record i: <what>" in *why.
static inline bool depth_rec_check(const telr_aln &a, size_t i, int32_t n_targets, const int32_t *target_len, uint64_t ncig, std::string *why)
{
    if (!record_check(a, i, n_targets, ncig, why)) return false;
    if (!(a.flags & TELR_F_SECONDARY) && a.te > target_len[a.tid]) { *why = "record " + std::to_string(i) + ": te beyond its target's end"; return false; }
    return true;
}

// A record on its own strand: the query interval as stored on a forward record, mirrored in the read on TELR_F_REV.
struct StrandCoords { int32_t rev, qs, qe; };
static inline StrandCoords strand_coords(const telr_aln &a)
{
    const int32_t rev = (a.flags & TELR_F_REV) ? 1 : 0;
    return {rev, rev ? a.qlen - a.qe : a.qs, rev ? a.qlen - a.qs : a.qe};
}

// A record as the stages that cut reads at reference coordinates (telr_draft_contigs, telr_bridge_contigs) hold it on the device, one
// per record of the result: 40 bytes, qs / qe on the record's own strand.
struct CutRec { int32_t ts, te, qs, qe, qlen, rev, n_cigar, pad; int64_t cigar_off; };

// Record i against a read set of n_reads sequences of lengths read_len: record_check, then the record's read is a sequence of the set,
// then with its length; the first fault is the one reported.  True with *e filled, or false with "record i: <what>" in *why.
static inline bool cut_rec_check(const telr_aln &a, size_t i, int32_t n_targets, uint64_t ncig, int32_t n_reads, const int32_t *read_len, CutRec *e, std::string *why)
{
    if (!record_check(a, i, n_targets, ncig, why)) return false;
    const char *what = a.qid >= n_reads ? "qid outside the read set" : a.qlen != read_len[a.qid] ? "qlen is not the length of its read in the read set" : nullptr;
    if (what) { *why = "record " + std::to_string(i) + ": " + what; return false; }
    const StrandCoords s = strand_coords(a);
    *e = {a.ts, a.te, s.qs, s.qe, a.qlen, s.rev, a.n_cigar, 0, a.cigar_off};
    return true;
}

// A call list as telr_call_insertions returns it: (tid, pos) strictly ascending, read_off from 0 and ascending, every supporter list
// ascending and distinct with ids in [0, n_reads) -- n_reads < 0: no upper bound.  Fills ckeys[k] = tid << 32 | pos and, when support
// is not null, support[k]; both hold n_calls elements.  True, or false with the reason in *why (ckeys / support then hold a prefix).
static inline bool call_list_check(int64_t n_calls, const telr_ins_call *calls, const int64_t *read_off, const int32_t *reads, int32_t n_targets, int64_t n_reads,
                                   uint64_t *ckeys, int32_t *support, std::string *why)
{
    auto bad = [&](int64_t k, const char *what) { *why = "call " + std::to_string(k) + ": " + what; return false; };
    for (int64_t k = 0; k < n_calls; ++k) {
        const telr_ins_call &c = calls[k];
        if (c.tid < 0 || c.tid >= n_targets) return bad(k, "tid outside n_targets");
        if (c.pos < 0) return bad(k, "negative pos");
        ckeys[k] = ((uint64_t)(uint32_t)c.tid << 32) | (uint32_t)c.pos;
        if (k > 0 && ckeys[k] <= ckeys[k - 1]) return bad(k, "calls not strictly ascending by (tid, pos)");
        if (support) support[k] = c.support;
    }
    if (n_calls <= 0) return true;
    if (read_off[0] != 0) { *why = "read_off[0] is not 0"; return false; }
    for (int64_t k = 0; k < n_calls; ++k) {
        if (read_off[k + 1] < read_off[k]) return bad(k, "read offsets descend");
        if (read_off[k + 1] > read_off[k] && !reads) { *why = "null reads"; return false; }
        for (int64_t j = read_off[k]; j < read_off[k + 1]; ++j) {
            if (n_reads < 0 ? reads[j] < 0 : (reads[j] < 0 || reads[j] >= n_reads)) return bad(k, n_reads < 0 ? "negative read id" : "read id outside the read set");
            if (j > read_off[k] && reads[j] <= reads[j - 1]) return bad(k, "read list not ascending");
        }
    }
    return true;
}

// A signature array as telr_call_insertions returns it, against the n records it was made from (every one passed record_check) and a
// read set of n_reads sequences: ascending by (tid, pos), every rec (and the mate of a kind 1) a record of the signature's own read.
// True, or false with "signature j: <what>" in *why.  What telr_draft_contigs and telr_bridge_contigs refuse in their signatures.
static inline bool sig_list_check(int64_t n_sig, const telr_ins_sig *sigs, const telr_aln *alns, size_t n, int32_t n_targets, int32_t n_reads, std::string *why)
{
    auto bad = [&](int64_t j, const char *what) { *why = "signature " + std::to_string(j) + ": " + what; return false; };
    uint64_t prev = 0;
    for (int64_t j = 0; j < n_sig; ++j) {
        const telr_ins_sig &s = sigs[j];
        if (s.tid < 0 || s.tid >= n_targets) return bad(j, "tid outside n_targets");
        if (s.pos < 0) return bad(j, "negative pos");
        if (s.rec < 0 || (size_t)s.rec >= n) return bad(j, "rec outside the records");
        if (s.kind == 1 && (s.mate < 0 || (size_t)s.mate >= n)) return bad(j, "mate outside the records");
        if (s.qid < 0 || s.qid >= n_reads) return bad(j, "qid outside the read set");
        if (alns[s.rec].qid != s.qid || (s.kind == 1 && alns[s.mate].qid != s.qid)) return bad(j, "qid is not its records' read");
        const uint64_t key = ((uint64_t)(uint32_t)s.tid << 32) | (uint32_t)s.pos;
        if (j > 0 && key < prev) return bad(j, "signatures not ascending by (tid, pos)");
        prev = key;
    }
    return true;
}
#endif /* TELR_RECORD_CHECKS_H */
