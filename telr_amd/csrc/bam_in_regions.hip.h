// bam_in_regions.hip.h -- telr_bam_load_regions: only the BGZF members that a .bai names for a list of regions are uploaded and inflated;
// their records are chained, filtered by true overlap and parsed on the device (the definition is in include/telr_hip.h
// and, as plain Python, in tests/bam_region_ref.py).  The result is what telr_bam_load gives for a file of the selected records.
//
//   host      bai_plan.h: regions -> merged regions; the index -> intervals [vbeg, vend) of virtual offsets, no member in two of them
//   device    the header, in a step of its own: the members from file offset 0 until bam_in_header is satisfied (k_bgzf_inflate)
//   host      the member list: hopped from every interval's coffset (never from the file's start); telr_bam_chunk_plan cuts it into chunks
//   per chunk (bamc_setup / bamc_issue / bamc_wait of bam_in_chunked.hip.h with their slots, carry and overlap: this load tells them which
//             members are file neighbours (BamChunked::run_of = the member's interval), so a chunk's file bytes go up run after run and lie
//             packed in the slot, and gives them the members' file offsets (BamChunked::coff) to name a block that fails to inflate):
//     k_bgzf_inflate
//     k_bam_chain_seg     one lane per segment: count pass, dev_qscan, emit pass -> the offsets of every record walked
//     k_bam_rec           every walked record is parsed and checked, selected or not (the bins over-select)
//     k_bam_region_keep   one lane per walked record: lower bound in the merged regions' keys, the overlap test -> keep flag
//     dev_qscan + k_bam_gather   dense BamRec, offsets and name lengths of the selected records
//     bam_load_fetch (bam_in_chunked.hip.h): k_bam_names, the copy to the host, the lowest record that broke a rule
//   host      bam_load_pass2 (bam_in_chunked.hip.h): bam_in_decide on the selected records; pass 2 (k_bam_cig, k_bam_seq, k_bam_qual) finds
//             them again by the same offsets
//
// Segments.  A chunk's buffer is carry + inflated members, and a chunk may hold many intervals, so it carries a list of segments (start,
// end, open) in buffer offsets, one per interval that has a member in the chunk.  The first may continue an interval of the chunk before:
// it starts at the carry (offset 0).  The last may stay open into the next chunk: it ends at the buffer's end and its tail behind the last
// complete record is the next carry.  A closed segment must chain to exactly its end; anything else is "the index does not match the file".
// The walk of one segment is serial, as the whole-file chain is; the segments of a chunk walk side by side.
#include "bai_plan.h"

struct BamSeg { int64_t start, end; int32_t open, pad; };

// pass 1 (EMIT false): cnt[s] = the segment's records, status[s] = 0 | 1 (a record runs past the end) | 2 (block_size below 32) | 3 (too
// many records), endp[s] = where the walk ended.  Pass 2: the same walk writes the offsets at base[s], the scan of cnt
template <bool EMIT>
__global__ void __launch_bounds__(64) k_bam_chain_seg(const uint8_t *__restrict__ stream, const BamSeg *__restrict__ seg, int32_t nseg, int32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ status, int64_t *__restrict__ endp, const int64_t *__restrict__ base, int64_t *__restrict__ offs)
{
    const int32_t s = (int32_t)blockIdx.x * 64 + (int32_t)threadIdx.x;
    if (s >= nseg) return;
    const int64_t end = seg[s].end, o = EMIT ? base[s] : 0;
    int64_t p = seg[s].start;
    int32_t n = 0, st = 0;
    while (p < end) {
        if (p + 4 > end) { st = 1; break; }
        const int32_t bs = (int32_t)bi_ld32(stream, p);
        if (bs < 32) { st = 2; break; }
        if (p + 4 + (int64_t)bs > end) { st = 1; break; }
        if (n >= 0x7ffffff0) { st = 3; break; }
        if (EMIT) offs[o + n] = p;
        ++n;
        p += 4 + (int64_t)bs;
    }
    if (!EMIT) { cnt[s] = n; status[s] = st; endp[s] = p; }
}

// keep[r] = 1 for a selected record: mapped, and [pos, pos + max(1, M + D)) overlaps a region of its target.  rkey[i] = tid << 32 | end of
// merged region i (ascending, disjoint), rbeg[i] its beg: the first region whose key is above the record's (refid, pos) is the only one
// that can overlap it.  A record that broke a rule is kept as well: the host names the lowest one
__global__ void __launch_bounds__(256) k_bam_region_keep(const BamRec *__restrict__ recs, int64_t nrec, const uint64_t *__restrict__ rkey, const int32_t *__restrict__ rbeg,
                                                         int32_t nreg, int32_t *__restrict__ keep)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    const BamRec *B = recs + r;
    const int32_t refid = B->refid, pos = B->pos;
    int32_t k = 0;
    if (B->status != BREC_OK) k = 1;
    else if (!(B->flag & 4) && refid >= 0) {
        const uint64_t key = (uint64_t)(uint32_t)refid << 32 | (uint32_t)pos;
        int32_t lo = 0, hi = nreg;
        while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (rkey[mid] <= key) lo = mid + 1; else hi = mid; }
        if (lo < nreg && (int32_t)(rkey[lo] >> 32) == refid) {
            const int64_t span = max((int64_t)1, (int64_t)B->sm + B->sd);
            if ((int64_t)pos + span > (int64_t)rbeg[lo]) k = 1;
        }
    }
    keep[r] = k;
}

// the kept records, dense, in file order: at[r] = the scan of keep
__global__ void __launch_bounds__(256) k_bam_gather(const BamRec *__restrict__ recs, const int64_t *__restrict__ offs, const int32_t *__restrict__ nlen, int64_t nrec,
                                                    const int32_t *__restrict__ keep, const int32_t *__restrict__ at, BamRec *__restrict__ recs_out,
                                                    int64_t *__restrict__ offs_out, int32_t *__restrict__ nlen_out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec || !keep[r]) return;
    const int32_t j = at[r];
    recs_out[j] = recs[r]; offs_out[j] = offs[r]; nlen_out[j] = nlen[r];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the header: the members from file offset 0 are inflated, as few as hold it (a header that needs more than the step before thought is
// inflated again from the start: there is one such step per 64 KiB of header at the most).  *n_members = how many the last step took
static int bamr_header(telr_ctx *ctx, BamInHop &H, telr_bam_in *B, int64_t *n_members)
{
    const uint8_t *d = H.F.p; const size_t size = H.F.n;
    size_t p = 0;
    int64_t need = 12, total = 0;
    H.mem.clear(); H.isz.clear();
    for (;;) {
        while (total < need && p < size) {
            BgzfMember M; size_t bsize = 0;
            if (const char *why = bgzf_member_at(d, size, p, M, bsize)) { ctx->err = "telr_bam_load: block " + std::to_string(H.mem.size()) + ": " + why; return TELR_E_ARG; }
            H.mem.push_back(M); H.isz.push_back((int32_t)M.isize); total += M.isize; p += bsize;
        }
        const bool all = p >= size;
        std::vector<uint8_t> h((size_t)total + 1);
        {
            BamChunked C(ctx, H);
            const uint8_t *d_h = nullptr;
            TRY(bamc_inflate_whole(C, &d_h));
            if (total) HIPCHK(hipMemcpy(h.data(), d_h, (size_t)total, hipMemcpyDeviceToHost));
        }
        int64_t from = 0, want = 0;
        const int rc = bam_in_header(ctx, h.data(), total, all ? total : INT64_MAX / 2, B, &from, &want);
        if (rc == TELR_OK) break;
        if (rc != 1) return rc;
        need = want;          // (rc 1 comes only while members are left: with all of them `total` is the stream's end and the header's error is final)
    }
    *n_members = (int64_t)H.mem.size();
    return TELR_OK;
}

// the member list of a region load: the intervals' members in file order
struct BamRegPlan {
    std::vector<BaiRegion> merged;
    std::vector<uint64_t> vbeg, vend;
    std::vector<int64_t> coff;         // [members] file offset of the member (of its header: the coffset of a virtual offset)
    std::vector<int64_t> ucum;         // [members + 1] inflated bytes before the member, over this list
    std::vector<int32_t> iv_of;        // [members] its interval
    std::vector<int64_t> iv_first;     // [intervals + 1] the interval's first member
    int64_t packed = 0;                // file bytes of all of them
};
static std::string bamr_mismatch(uint64_t v) { return "telr_bam_load: the index does not match the file at virtual offset " + std::to_string(v); }

// hops every interval from its coffset; H.mem / H.isz become the load's member list
static int bamr_members(telr_ctx *ctx, BamInHop &H, BamRegPlan &P)
{
    const uint8_t *d = H.F.p; const size_t size = H.F.n;
    H.mem.clear(); H.isz.clear(); H.total = 0;
    P.ucum.assign(1, 0);
    const size_t ni = P.vbeg.size();
    for (size_t i = 0; i < ni; ++i) {
        const uint64_t c0 = P.vbeg[i] >> 16, c1 = P.vend[i] >> 16; const uint32_t u0 = (uint32_t)(P.vbeg[i] & 0xffff), u1 = (uint32_t)(P.vend[i] & 0xffff);
        for (uint64_t c : { c0, c1 }) {
            if (c >= size) { ctx->err = "telr_bam_load: the index names file offset " + std::to_string(c) + ", at or beyond the BAM's size"; return TELR_E_ARG; }
            if (c + 4 > size || d[c] != 0x1f || d[c + 1] != 0x8b || d[c + 2] != 8 || d[c + 3] != 4) {
                ctx->err = "telr_bam_load: the index names file offset " + std::to_string(c) + ", which does not start with the BGZF magic"; return TELR_E_ARG;
            }
        }
        P.iv_first.push_back((int64_t)H.mem.size());
        size_t p = (size_t)c0;
        for (;;) {
            if (p == c1 && u1 == 0) break;
            if (p > c1) { ctx->err = bamr_mismatch(P.vend[i]); return TELR_E_ARG; }          // the members from c0 do not meet c1
            BgzfMember M; size_t bsize = 0;
            if (const char *why = bgzf_member_at(d, size, p, M, bsize)) { ctx->err = "telr_bam_load: block at file offset " + std::to_string(p) + ": " + why; return TELR_E_ARG; }
            if (H.mem.size() >= 0x7ffffff0u) { ctx->err = "telr_bam_load: too many BGZF members"; return TELR_E_RANGE; }
            H.mem.push_back(M); H.isz.push_back((int32_t)M.isize); P.coff.push_back((int64_t)p); P.iv_of.push_back((int32_t)i);
            H.total += M.isize; P.ucum.push_back(H.total); P.packed += (int64_t)M.clen;
            if (p == c1) break;
            p += bsize;
        }
        // the offsets inside the first and the last member must exist
        const size_t a = (size_t)P.iv_first.back(), b = H.mem.size();
        if (b == a || u0 > H.mem[a].isize) { ctx->err = bamr_mismatch(P.vbeg[i]); return TELR_E_ARG; }
        if (u1 > H.mem[b - 1].isize || (b - a == 1 && u1 && u1 <= u0)) { ctx->err = bamr_mismatch(P.vend[i]); return TELR_E_ARG; }
    }
    P.iv_first.push_back((int64_t)H.mem.size());
    return TELR_OK;
}

// the virtual offset of inflated byte g of the member list; the answer stays inside members [m0, m1)
static uint64_t bamr_voff(const BamRegPlan &P, int64_t g, int64_t m0, int64_t m1)
{
    int64_t m = (int64_t)(std::upper_bound(P.ucum.begin(), P.ucum.end(), g) - P.ucum.begin()) - 1;
    m = std::min(std::max(m, m0), m1 - 1);
    return (uint64_t)P.coff[(size_t)m] << 16 | (uint64_t)std::min<int64_t>(std::max<int64_t>(g - P.ucum[(size_t)m], 0), 0xffff);
}

// chunk k's segments in the offsets of its buffer (carry + members)
static void bamr_segments(const BamChunked &C, const BamRegPlan &P, int64_t k, int64_t carry, std::vector<BamSeg> &seg, std::vector<int32_t> &seg_iv)
{
    seg.clear(); seg_iv.clear();
    const int64_t m0 = C.first[(size_t)k], m1 = C.first[(size_t)k + 1];
    const int64_t u0 = P.ucum[(size_t)m0], buflen = carry + (P.ucum[(size_t)m1] - u0);
    for (int64_t m = m0; m < m1; ) {
        const int32_t i = P.iv_of[(size_t)m];
        const int64_t a = P.iv_first[(size_t)i], b = P.iv_first[(size_t)i + 1], last = std::min(b, m1) - 1;
        BamSeg S; S.pad = 0;
        S.start = m == a ? carry + (P.ucum[(size_t)m] - u0) + (int64_t)(P.vbeg[(size_t)i] & 0xffff) : 0;          // (m > a only for the chunk's first member: the carry is its interval's)
        S.open = b > m1 ? 1 : 0;
        const int64_t ue = (int64_t)(P.vend[(size_t)i] & 0xffff);
        S.end = S.open ? buflen : carry + (ue ? P.ucum[(size_t)last] - u0 + ue : P.ucum[(size_t)last + 1] - u0);
        seg.push_back(S); seg_iv.push_back(i);
        m = last + 1;
    }
}

static int bam_load_regions(telr_ctx *ctx, const char *path, const char *bai_path, int32_t keep_qual, int64_t chunk_bytes, int64_t n_regions, const telr_region *regions,
                            telr_bam_in **out)
{
    BamInClock wall, clk;
    std::unique_ptr<telr_bam_in, void (*)(telr_bam_in*)> B(new telr_bam_in(), telr_bam_in_free);
    B->ctx = ctx;
    // refusals that need no file
    if (n_regions < 0) { ctx->err = "telr_bam_load_regions: a negative number of regions"; return TELR_E_ARG; }
    if (n_regions > 0 && !regions) { ctx->err = "telr_bam_load_regions: null regions"; return TELR_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    BamInHop H;
    TRY(bam_in_open(ctx, "telr_bam_load", path, H));
    B->counters[8] = H.no_eof;
    int64_t n_hdr = 0;
    TRY(bamr_header(ctx, H, B.get(), &n_hdr));
    const int32_t n_ref = (int32_t)B->tnames.size();
    // ---- the plan: regions, intervals, members
    clk.lap();
    BamRegPlan P;
    std::string why;
    int rc = bai_regions(n_ref, B->tlens.data(), n_regions, regions, P.merged, &why);
    if (rc != TELR_OK) { ctx->err = "telr_bam_load_regions: " + why; return rc; }
    if (!P.merged.empty()) {
        std::vector<uint8_t> bai;
        const std::string bp = bai_path ? std::string(bai_path) : std::string(path) + ".bai";
        if ((rc = bai_read_file(bp.c_str(), bai, &why)) != TELR_OK || (rc = bai_plan(bai.data(), bai.size(), n_ref, P.merged, P.vbeg, P.vend, &why)) != TELR_OK) {
            ctx->err = "telr_bam_load_regions: " + why; return rc;
        }
    }
    TRY(bamr_members(ctx, H, P));
    H.ms = clk.lap();
    B->phase_ms[BIN_HOP] = H.ms;
    const int64_t nm = (int64_t)H.mem.size();
    B->counters[0] = nm;
    TRY(bamc_auto_chunk(ctx, P.packed + H.total, &chunk_bytes));
    BamChunked C(ctx, H);
    C.run_of = P.iv_of.data(); C.coff = P.coff.data();          // a run ends where the interval does; a failed block is named by its file offset
    TRY(bamc_setup(C, chunk_bytes, 1));
    hipStream_t st = C.s_main;
    const int64_t nch = C.nch;
    // the merged regions' keys
    const int32_t nreg = (int32_t)P.merged.size();
    uint64_t *d_rkey = nullptr; int32_t *d_rbeg = nullptr;
    if (nreg) {
        std::vector<uint64_t> rkey((size_t)nreg); std::vector<int32_t> rbeg((size_t)nreg);
        for (int32_t i = 0; i < nreg; ++i) { rkey[(size_t)i] = (uint64_t)(uint32_t)P.merged[(size_t)i].tid << 32 | (uint32_t)P.merged[(size_t)i].end; rbeg[(size_t)i] = P.merged[(size_t)i].beg; }
        TRY(ctx_buf_t(ctx, "bamr_rkey", (size_t)nreg, &d_rkey));
        TRY(ctx_buf_t(ctx, "bamr_rbeg", (size_t)nreg, &d_rbeg));
        HIPCHK(hipMemcpyAsync(d_rkey, rkey.data(), (size_t)nreg * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_rbeg, rbeg.data(), (size_t)nreg * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // ---- pass 1: every chunk's segments, its walked records, the selected ones' fields and names
    BamPass1 P1;
    std::vector<int64_t> &rec0 = P1.rec0, &carry_in = P1.carry_in, &cut = P1.cut, offs_k;
    std::vector<uint64_t> voff;          // [selected] file-order numbers are unknown here: a record is named by its virtual offset
    const auto who = [&](int64_t r) { return "at virtual offset " + std::to_string(voff[(size_t)r]); };
    rec0.assign((size_t)nch + 1, 0); carry_in.assign((size_t)nch + 1, 0); cut.assign((size_t)nch, 0);
    std::vector<BamSeg> seg; std::vector<int32_t> seg_iv, h_stat; std::vector<int64_t> h_endp;
    int64_t carry = 0, &max_carry = P1.max_carry, n_walked = 0;
    float ms_parse = 0;
    if (nch) TRY(bamc_issue(C, 0));
    for (int64_t k = 0; k < nch; ++k) {
        const bool last = k + 1 >= nch;
        TRY(bamc_wait(C, k));
        BamChunkSlot &s = C.at(k);
        const int64_t m0 = C.first[(size_t)k], buflen = carry + C.payload(k), g0 = P.ucum[(size_t)m0] - carry;      // g0: the buffer's first byte in the member list's stream
        uint8_t *buf = s.d_buf + s.room - carry;
        carry_in[(size_t)k] = carry; max_carry = std::max(max_carry, carry);
        bamr_segments(C, P, k, carry, seg, seg_iv);
        const int32_t nseg = (int32_t)seg.size();          // at least one: the chunk holds a member, and every member has its interval
        BamSeg *d_seg; int32_t *d_cnt, *d_stat; int64_t *d_endp, *d_base, *d_tot;
        TRY(ctx_buf_t(ctx, "bamr_seg", (size_t)nseg, &d_seg));
        TRY(ctx_buf_t(ctx, "bamr_cnt", (size_t)nseg + 1, &d_cnt));
        TRY(ctx_buf_t(ctx, "bamr_stat", (size_t)nseg, &d_stat));
        TRY(ctx_buf_t(ctx, "bamr_endp", (size_t)nseg, &d_endp));
        TRY(ctx_buf_t(ctx, "bamr_base", (size_t)nseg + 2, &d_base));
        TRY(ctx_buf_t(ctx, "bamr_tot", 2, &d_tot));
        HIPCHK(hipMemcpyAsync(d_seg, seg.data(), (size_t)nseg * sizeof(BamSeg), hipMemcpyHostToDevice, st));
        const dim3 sgrid((unsigned)((nseg + 63) / 64));
        HIPCHK(hipEventRecord(C.ec0, st));
        hipLaunchKernelGGL(k_bam_chain_seg<false>, sgrid, dim3(64), 0, st, buf, d_seg, nseg, d_cnt, d_stat, d_endp, nullptr, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(C.ec1, st));
        TRY((dev_qscan<int32_t, int64_t>(ctx, d_cnt, nseg, d_base, d_tot, 0, nullptr, nullptr)));
        if (!last) TRY(bamc_issue(C, k + 1));         // (the host is busy with the upload while the segments walk)
        h_stat.resize((size_t)nseg); h_endp.resize((size_t)nseg);
        int64_t nwalk = 0;
        HIPCHK(hipMemcpyAsync(h_stat.data(), d_stat, (size_t)nseg * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_endp.data(), d_endp, (size_t)nseg * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&nwalk, d_tot, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, C.ec0, C.ec1)); C.ms_chain += ms;
        clk.lap();
        for (int32_t j = 0; j < nseg; ++j) {          // in file order: the lowest offending segment is the error
            const BamSeg &S = seg[(size_t)j];
            if (h_stat[(size_t)j] == 3) { ctx->err = "telr_bam_load: too many records"; return TELR_E_RANGE; }
            if (h_stat[(size_t)j] == 2 || (!S.open && (h_stat[(size_t)j] != 0 || h_endp[(size_t)j] != S.end))) {
                const int32_t iv = seg_iv[(size_t)j];          // (the offset is named inside the members of the segment's interval)
                ctx->err = bamr_mismatch(bamr_voff(P, g0 + h_endp[(size_t)j], P.iv_first[(size_t)iv], P.iv_first[(size_t)iv + 1]));
                if (h_stat[(size_t)j] == 2) ctx->err += " (block_size below 32)";
                return TELR_E_ARG;
            }
        }
        if (nwalk >= 0x7ffffff0LL || rec0[(size_t)k] + nwalk >= 0x7ffffff0LL) { ctx->err = "telr_bam_load: too many records"; return TELR_E_RANGE; }
        n_walked += nwalk;
        const int64_t p_end = seg.back().open ? h_endp[(size_t)nseg - 1] : buflen;
        int64_t nsel = 0;
        if (nwalk) {
            int64_t *d_woffs; BamRec *d_wrecs; int32_t *d_wnlen, *d_keep, *d_kat;
            TRY(ctx_buf_t(ctx, "bamr_woffs", (size_t)nwalk + 1, &d_woffs));
            TRY(ctx_buf_t(ctx, "bamr_wrecs", (size_t)nwalk, &d_wrecs));
            TRY(ctx_buf_t(ctx, "bamr_wnlen", (size_t)nwalk + 1, &d_wnlen));
            TRY(ctx_buf_t(ctx, "bamr_keep", (size_t)nwalk + 1, &d_keep));
            TRY(ctx_buf_t(ctx, "bamr_kat", (size_t)nwalk + 2, &d_kat));
            hipLaunchKernelGGL(k_bam_chain_seg<true>, sgrid, dim3(64), 0, st, buf, d_seg, nseg, nullptr, nullptr, nullptr, d_base, d_woffs);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_bam_rec, dim3((unsigned)((nwalk + 3) / 4)), dim3(256), 0, st, buf, d_woffs, nwalk, n_ref, d_wrecs, d_wnlen);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_bam_region_keep, grid256(nwalk), dim3(256), 0, st, d_wrecs, nwalk, d_rkey, d_rbeg, nreg, d_keep);
            HIPCHK(hipGetLastError());
            TRY((dev_qscan<int32_t, int32_t>(ctx, d_keep, (int32_t)nwalk, d_kat, d_tot + 1, 0, nullptr, nullptr)));
            HIPCHK(hipMemcpyAsync(&nsel, d_tot + 1, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (nsel) {
                BamRec *d_recs; int32_t *d_nlen; int64_t *d_offs;
                TRY(ctx_buf_t(ctx, "bamin_recs", (size_t)nsel, &d_recs));
                TRY(ctx_buf_t(ctx, "bamin_offs", (size_t)nsel + 1, &d_offs));
                TRY(ctx_buf_t(ctx, "bamin_nlen", (size_t)nsel + 1, &d_nlen));
                hipLaunchKernelGGL(k_bam_gather, grid256(nwalk), dim3(256), 0, st, d_wrecs, d_woffs, d_wnlen, nwalk, d_keep, d_kat, d_recs, d_offs, d_nlen);
                HIPCHK(hipGetLastError());
                // the selected records' virtual offsets first: a record that broke a rule -- it is selected too -- is named by its
                offs_k.resize((size_t)nsel);
                HIPCHK(hipMemcpyAsync(offs_k.data(), d_offs, (size_t)nsel * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int64_t i = 0; i < nsel; ++i) voff.push_back(bamr_voff(P, g0 + offs_k[(size_t)i], 0, nm));
                TRY(bam_load_fetch(ctx, buf, d_recs, d_offs, d_nlen, nsel, P1, who));
            }
        }
        ms_parse += clk.lap();
        rec0[(size_t)k + 1] = rec0[(size_t)k] + nsel;
        cut[(size_t)k] = p_end;
        carry = buflen - p_end;
        if (!last) TRY(bamc_carry(C, k, buf + p_end, carry, (size_t)C.payload(k + 1)));
    }
    B->phase_ms[BIN_CHAIN] = C.ms_chain; B->phase_ms[BIN_PARSE] = ms_parse;
    // ---- the host decides on the selected records -- they are the file now -- and pass 2 finds them again by the same offsets: same carry,
    // same members.  One chunk: slot 0 holds it where pass 1 left it and "bamin_recs" holds its selected records' fields
    int64_t passes = 1;
    TRY(bam_load_pass2(ctx, B.get(), C, P1, keep_qual, clk, who, &passes));
    B->phase_ms[BIN_TOTAL] = wall.lap();
    B->chunk_info[0] = nch; B->chunk_info[1] = passes; B->chunk_info[2] = (int64_t)C.max_alloc; B->chunk_info[3] = max_carry;
    B->region_info[0] = nreg; B->region_info[1] = (int64_t)P.vbeg.size(); B->region_info[2] = nm; B->region_info[3] = n_hdr;
    B->region_info[4] = n_walked; B->region_info[5] = (int64_t)P1.recs.size();
    B->region_bytes = C.uploaded;          // both passes; the header step had slots of its own
    *out = B.release();
    return TELR_OK;
}

static thread_local std::string g_bai_plan_err;
extern "C" int telr_bai_plan(const char *bai_path, int32_t n_ref, int64_t n_regions, const telr_region *regions, uint64_t *vbeg, uint64_t *vend, int64_t cap, int64_t *n_intervals)
{
    g_bai_plan_err.clear();
    const int rc = bai_plan_file(bai_path, n_ref, n_regions, regions, vbeg, vend, cap, n_intervals, &g_bai_plan_err);
    if (rc != TELR_OK) g_bai_plan_err = "telr_bai_plan: " + g_bai_plan_err;
    return rc;
}
extern "C" const char *telr_bai_plan_error(void) { return g_bai_plan_err.c_str(); }

extern "C" int telr_bam_load_regions(telr_ctx *ctx, const char *bam_path, const char *bai_path, int32_t keep_qual, int64_t chunk_bytes, int64_t n_regions,
                                     const telr_region *regions, telr_bam_in **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    if (!bam_path || !out) { ctx->err = "telr_bam_load_regions: null path or output"; return TELR_E_ARG; }
    if (chunk_bytes < TELR_BAM_CHUNK_FIT) { ctx->err = "telr_bam_load_regions: chunk_bytes below TELR_BAM_CHUNK_FIT"; return TELR_E_ARG; }
    return bam_load_regions(ctx, bam_path, bai_path, keep_qual, chunk_bytes, n_regions, regions, out);
}
extern "C" int telr_bam_in_region_info(const telr_bam_in *in, int64_t *out)
{
    if (!in || !out) return TELR_E_ARG;
    memcpy(out, in->region_info, sizeof(in->region_info));
    return TELR_OK;
}
extern "C" int64_t telr_bam_in_region_bytes(const telr_bam_in *in) { return in ? in->region_bytes : 0; }
