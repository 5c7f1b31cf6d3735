// bam_in_chunked.hip.h -- bam_load: the one load behind telr_bam_load and telr_bam_load_chunked, its chunk slots, and
// the entry points.  The file is cut into chunks of whole BGZF members (bam_chunk_plan.h); every chunk is uploaded, inflated and parsed
// in turn, so that the transient device memory depends on the chunk and not on the file.  telr_bam_load is the plan of one chunk: one
// slot, the file next to its inflated stream.  The kernels are those of bam_in.hip.h.  The region load (bam_in_regions.hip.h) and the
// reads load (reads_in.hip.h) run the same slots, setup, issue and wait; the region load also the same tail of pass 1 (bam_load_fetch)
// and the same back half (bam_load_pass2).
//
// Two passes.  Which records are kept and where their words and bases go depends on the whole file (a supplementary record may come
// any number of chunks before its primary, the first name wins across chunks, orphans and len_mismatch need the primary's length):
//   pass 1    per chunk: upload, k_bgzf_inflate, k_bam_chain, k_bam_rec, k_bam_names; fields and names go to the host
//   host      bam_in_decide, on the whole file's records
//   pass 2    per chunk: upload and inflate again, then k_bam_cig, k_bam_seq, k_bam_qual straight into the final arrays at their
//             final offsets.  The reads first met in one chunk have consecutive numbers: one contiguous stretch of the set's layout.
//             One chunk: it is still in its slot, inflated, and so are its records' fields; nothing is uploaded or inflated again.
// So every store position stays a scan's result or the lane's own index, there is no atomic and no provisional array to gather from;
// the price, with more than one chunk, is a second inflate.
//
// A chunk's buffer.  slot = [ room | the chunk's inflated members | 64 ].  The members are inflated to a fixed place behind `room`, so the
// inflate of chunk k + 1 can run before chunk k's record chain has said how long the carry is; the carry -- the bytes of chunk k behind
// its last complete record, or all of it while the header is incomplete -- is then copied to the END of the next slot's room and the
// chunk's kernels see  buf = slot + room - carry,  carry + members bytes long.  A carry longer than the room (a record or a header
// longer than a chunk grows it over several chunks) makes the slot grow; that is no error.  Offsets into `buf` are the same in both
// passes: same carry, same members.
//
// A chunk's file bytes.  The members of a list need not be neighbours in the file: a region load (bam_in_regions.hip.h) runs these slots
// over the members of its intervals and says which are neighbours (BamChunked::run_of).  A chunk is uploaded run after run, packed one
// behind the other in the slot's file buffer, and its member table points into the packed bytes; a whole file is the case of one run per
// chunk.  bamc_setup sizes the file buffer by the same sum over runs that bamc_issue uploads, plus the padding that the inflate kernel's
// staged reads need behind the last byte.  A block that fails to inflate is named by bamc_wait: by its number in the file or, for a list
// that is not the file's, by its file offset (BamChunked::coff).
//
// Overlap.  Two slots (one chunk: one).  Chunk k + 1 is uploaded and inflated on a second stream while chunk k is chained and parsed on
// the context's stream; the host waits for chunk k's results at the end of every chunk (it needs them), which also orders the slots' reuse.
#include "bam_chunk_plan.h"

#define BAMC_AUTO_DIV  16               /* chunk_bytes 0: free device memory / 16 ... */
#define BAMC_AUTO_MAX  (1LL << 30)      /* ... at most 1 GiB ... */
#define BAMC_AUTO_MIN  (1LL << 20)      /* ... at least 1 MiB */
#define BAMC_ROOM      (65536 - 64)     /* a slot's carry room is a multiple of this: with the 64 bytes behind the members a slot is never
                                           more than 64 KiB above carry + members */
#define BAMC_WHOLE     INT64_MAX        /* a chunk_bytes that no sum of ISIZE reaches (below 2^31 members of at most 64 KiB): one chunk */

struct BamChunkSlot {
    char nm_file[32], nm_buf[32], nm_mem[32], nm_ooff[32], nm_status[32];
    uint8_t *d_file = nullptr, *d_buf = nullptr;
    size_t room = 0;
    BgzfMember *d_mem = nullptr; int64_t *d_ooff = nullptr; int32_t *d_status = nullptr;
    std::vector<BgzfMember> h_mem; std::vector<int64_t> h_ooff; std::vector<int32_t> h_status;      // alive while their copies may run
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;      // before the upload, behind it, behind the inflate
};
struct BamChunked {
    telr_ctx *ctx; const BamInHop &H;
    hipStream_t s_main, s_io;
    std::vector<int64_t> first;          // [nch + 1] the chunks' first members
    int64_t nch = 0;
    size_t max_payload = 0, max_cbytes = 0, max_members = 0, max_alloc = 0;      // max_alloc: the largest slot buffer of the load
    BamChunkSlot slot[2];
    int nslot = 2;                       // 1 or 2 of them are set up; chunk k runs in at(k)
    BamChunkSlot &at(int64_t k) { return slot[k & (nslot - 1)]; }
    CrcTabs *d_tabs = nullptr;
    hipEvent_t ec0 = nullptr, ec1 = nullptr;      // around a chunk's record chain
    float ms_upload = 0, ms_inflate = 0, ms_chain = 0;
    const char *what = "telr_bam_load";      // opens a failed block's error text (telr_reads_load runs the same slots: reads_in.hip.h)
    // a member list that is not one stretch of the file (a region load's; null: all of H.mem are file neighbours):
    const int32_t *run_of = nullptr;     // [members] two neighbours of the list are neighbours in the file iff their entries are equal
    const int64_t *coff = nullptr;       // [members] file offsets: a failed block is named by its, not by its number in the list
    int64_t uploaded = 0;                // file bytes that bamc_issue has sent up so far
    BamChunked(telr_ctx *c, const BamInHop &h) : ctx(c), H(h), s_main(c->stream), s_io(c->side[0]) {}
    ~BamChunked()
    {
        (void)hipStreamSynchronize(s_io); (void)hipStreamSynchronize(s_main);      // nothing of a failed load is left running
        for (BamChunkSlot &s : slot) for (hipEvent_t e : { s.e0, s.e1, s.e2 }) if (e) (void)hipEventDestroy(e);
        if (ec0) (void)hipEventDestroy(ec0);
        if (ec1) (void)hipEventDestroy(ec1);
    }
    int64_t payload(int64_t k) const { int64_t s = 0; for (int64_t m = first[(size_t)k]; m < first[(size_t)k + 1]; ++m) s += H.mem[(size_t)m].isize; return s; }
};

// a slot's carry room of at least `need` bytes; the `keep` bytes of members behind the room move with it
static int bamc_room(BamChunked &C, BamChunkSlot &s, size_t need, size_t keep)
{
    telr_ctx *ctx = C.ctx;
    if (s.room >= need && s.d_buf) return TELR_OK;
    const size_t room = std::max<size_t>((need + BAMC_ROOM - 1) / BAMC_ROOM, 1) * BAMC_ROOM, bytes = room + C.max_payload + 64;
    C.max_alloc = std::max(C.max_alloc, bytes);
    HIPCHK(hipStreamSynchronize(C.s_io)); HIPCHK(hipStreamSynchronize(C.s_main));
    DBuf &b = ctx->bufs[s.nm_buf];
    const bool move = keep && s.d_buf;
    // nothing moves: the old buffer (an earlier load's, too) goes first, so that a load never holds a slot twice
    if (!move && b.p) { s.d_buf = nullptr; HIPCHK(hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    if (move) {
        const hipError_t e = hipMemcpy((uint8_t*)p + room, s.d_buf + s.room, keep, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { (void)hipFree(p); HIPCHK(e); }
    }
    if (b.p) HIPCHK(hipFree(b.p));
    b.p = p; b.bytes = bytes;
    s.d_buf = (uint8_t*)p; s.room = room;
    return TELR_OK;
}

// the load's `nslot` slots: names, carry room (C.max_payload says how much follows it) and events; `members`: and what a chunk of BGZF
// members needs on its way -- its slice of the file, its member table, output offsets and statuses (C.max_cbytes, C.max_members)
static int bamc_slots(BamChunked &C, int nslot, bool members)
{
    telr_ctx *ctx = C.ctx;
    C.nslot = nslot;
    for (int i = 0; i < nslot; ++i) {
        BamChunkSlot &s = C.slot[i];
        snprintf(s.nm_file, sizeof(s.nm_file), "bamin_c%d_file", i); snprintf(s.nm_buf, sizeof(s.nm_buf), "bamin_c%d_buf", i);
        snprintf(s.nm_mem, sizeof(s.nm_mem), "bamin_c%d_mem", i); snprintf(s.nm_ooff, sizeof(s.nm_ooff), "bamin_c%d_ooff", i);
        snprintf(s.nm_status, sizeof(s.nm_status), "bamin_c%d_status", i);
        if (members) {
            TRY(ctx_buf_t(ctx, s.nm_file, ((C.max_cbytes + 3) & ~(size_t)3) + BGZF_INCH + 16, &s.d_file));
            TRY(ctx_buf_t(ctx, s.nm_mem, C.max_members + 1, &s.d_mem));
            TRY(ctx_buf_t(ctx, s.nm_ooff, C.max_members + 1, &s.d_ooff));
            TRY(ctx_buf_t(ctx, s.nm_status, C.max_members + 1, &s.d_status));
        }
        // (the buffer of an earlier load is not taken over: its room and its members' place are this load's)
        s.d_buf = nullptr; s.room = 0;
        TRY(bamc_room(C, s, 0, 0));
        HIPCHK(hipEventCreate(&s.e0)); HIPCHK(hipEventCreate(&s.e1)); HIPCHK(hipEventCreate(&s.e2));
    }
    return TELR_OK;
}

// members [m, m1) of a chunk: one behind the last member of the run of file neighbours that starts at m
static int64_t bamc_run_end(const BamChunked &C, int64_t m, int64_t m1)
{
    if (!C.run_of) return m1;
    int64_t e = m + 1;
    while (e < m1 && C.run_of[(size_t)e] == C.run_of[(size_t)m]) ++e;
    return e;
}
// the file bytes of the run [m, e)
static size_t bamc_run_bytes(const BamChunked &C, int64_t m, int64_t e)
{
    const BgzfMember &a = C.H.mem[(size_t)m], &b = C.H.mem[(size_t)e - 1];
    return (size_t)(b.off + b.clen - a.off);
}

// the chunk plan and its slots: two, or one where the plan has at most one chunk and the caller asks for no more (min_slots 1).  A chunk's
// file bytes are those of its runs, which lie packed in the slot; one run: from its first member to the end of its last
static int bamc_setup(BamChunked &C, int64_t chunk_bytes, int min_slots)
{
    telr_ctx *ctx = C.ctx;
    const int64_t nm = (int64_t)C.H.mem.size();
    int64_t nch = 0;
    int rc = bam_chunk_plan(nm, C.H.isz.data(), chunk_bytes, nullptr, 0, &nch);
    if (rc != TELR_OK && rc != TELR_E_RANGE) { ctx->err = std::string(C.what) + ": chunk plan"; return rc; }
    C.first.assign((size_t)nch + 1, nm);
    if (nch) TRY(bam_chunk_plan(nm, C.H.isz.data(), chunk_bytes, C.first.data(), nch, &nch));
    C.nch = nch;
    for (int64_t k = 0; k < nch; ++k) {
        const int64_t m0 = C.first[(size_t)k], m1 = C.first[(size_t)k + 1];
        size_t cb = 0;
        for (int64_t m = m0, e; m < m1; m = e) { e = bamc_run_end(C, m, m1); cb += bamc_run_bytes(C, m, e); }
        C.max_payload = std::max(C.max_payload, (size_t)C.payload(k));
        C.max_cbytes = std::max(C.max_cbytes, cb);
        C.max_members = std::max(C.max_members, (size_t)(m1 - m0));
    }
    TRY(bamc_slots(C, (int)std::max<int64_t>(std::min<int64_t>(nch, 2), min_slots), true));
    HIPCHK(hipEventCreate(&C.ec0)); HIPCHK(hipEventCreate(&C.ec1));
    TRY(ctx_buf_t(ctx, "bamin_crctabs", 1, &C.d_tabs));
    { static CrcTabs T; static bool made = false; if (!made) { crc_tabs_make(T); made = true; } HIPCHK(hipMemcpyAsync(C.d_tabs, &T, sizeof(T), hipMemcpyHostToDevice, C.s_main)); }
    HIPCHK(hipStreamSynchronize(C.s_main));
    return TELR_OK;
}

// chunk k: its file bytes go up run after run, packed one behind the other, with its member table (offsets relative to the packed bytes);
// its members are inflated behind the slot's room
static int bamc_issue(BamChunked &C, int64_t k)
{
    telr_ctx *ctx = C.ctx;
    BamChunkSlot &s = C.at(k);
    const std::vector<BgzfMember> &mem = C.H.mem;
    const int64_t m0 = C.first[(size_t)k], m1 = C.first[(size_t)k + 1], n = m1 - m0;
    s.h_mem.assign(mem.begin() + m0, mem.begin() + m1); s.h_ooff.resize((size_t)n); s.h_status.resize((size_t)n);
    size_t cb = 0;
    int64_t o = 0;
    for (int64_t m = m0, e; m < m1; m = e) {
        e = bamc_run_end(C, m, m1);
        const int64_t f0 = mem[(size_t)m].off;
        for (int64_t j = m - m0; j < e - m0; ++j) { s.h_mem[(size_t)j].off += (int64_t)cb - f0; s.h_ooff[(size_t)j] = o; o += s.h_mem[(size_t)j].isize; }
        cb += bamc_run_bytes(C, m, e);
    }
    C.uploaded += (int64_t)cb;
    HIPCHK(hipEventRecord(s.e0, C.s_io));
    for (int64_t m = m0, e; m < m1; m = e) {          // (a run's place among the packed bytes is its first member's)
        e = bamc_run_end(C, m, m1);
        const size_t len = bamc_run_bytes(C, m, e);
        if (len) HIPCHK(hipMemcpyAsync(s.d_file + s.h_mem[(size_t)(m - m0)].off, C.H.F.p + mem[(size_t)m].off, len, hipMemcpyHostToDevice, C.s_io));
    }
    HIPCHK(hipMemsetAsync(s.d_file + cb, 0, ((cb + 3) & ~(size_t)3) - cb + BGZF_INCH + 16, C.s_io));
    HIPCHK(hipMemcpyAsync(s.d_mem, s.h_mem.data(), (size_t)n * sizeof(BgzfMember), hipMemcpyHostToDevice, C.s_io));
    HIPCHK(hipMemcpyAsync(s.d_ooff, s.h_ooff.data(), (size_t)n * 8, hipMemcpyHostToDevice, C.s_io));
    HIPCHK(hipMemsetAsync(s.d_buf + s.room + o, 0, 64, C.s_io));
    HIPCHK(hipEventRecord(s.e1, C.s_io));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n), dim3(64), 0, C.s_io, s.d_file, s.d_mem, s.d_ooff, C.d_tabs, s.d_buf + s.room, s.d_status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.h_status.data(), s.d_status, (size_t)n * 4, hipMemcpyDeviceToHost, C.s_io));
    HIPCHK(hipEventRecord(s.e2, C.s_io));
    return TELR_OK;
}
// chunk k is inflated; the lowest block that failed is the error.  It is named by its number in the member list, which for a whole file is
// its number in the file; a load whose list is not the file's (C.coff) names it by its file offset
static int bamc_wait(BamChunked &C, int64_t k)
{
    telr_ctx *ctx = C.ctx;
    BamChunkSlot &s = C.at(k);
    HIPCHK(hipEventSynchronize(s.e2));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, s.e0, s.e1)); HIPCHK(hipEventElapsedTime(&b, s.e1, s.e2));
    C.ms_upload += a; C.ms_inflate += b;
    for (size_t j = 0; j < s.h_status.size(); ++j)
        if (s.h_status[j] != INFL_OK) {
            const int64_t m = C.first[(size_t)k] + (int64_t)j;
            ctx->err = std::string(C.what) + ": block " + (C.coff ? "at file offset " + std::to_string(C.coff[(size_t)m]) : std::to_string(m)) + ": " + infl_text(s.h_status[j]);
            return TELR_E_ARG;
        }
    return TELR_OK;
}
// the `len` bytes at src (chunk k's buffer) become chunk k + 1's carry: the end of its slot's room.  keep: the bytes of chunk k + 1 that
// are behind that room already, or on their way there; they move with a room that grows
static int bamc_carry(BamChunked &C, int64_t k, const uint8_t *src, int64_t len, size_t keep)
{
    telr_ctx *ctx = C.ctx;
    BamChunkSlot &d = C.at(k + 1);
    TRY(bamc_room(C, d, (size_t)len, keep));
    if (len) HIPCHK(hipMemcpyAsync(d.d_buf + d.room - len, src, (size_t)len, hipMemcpyDeviceToDevice, C.s_main));
    HIPCHK(hipStreamSynchronize(C.s_main));
    return TELR_OK;
}

// all of H.mem as one chunk, inflated in slot 0: *d_out = its inflated stream (the header step of a region load, the test tap)
static int bamc_inflate_whole(BamChunked &C, const uint8_t **d_out)
{
    TRY(bamc_setup(C, BAMC_WHOLE, 1));
    if (C.nch) { TRY(bamc_issue(C, 0)); TRY(bamc_wait(C, 0)); }
    *d_out = C.slot[0].d_buf + C.slot[0].room;
    return TELR_OK;
}

// chunk_bytes <= 0 becomes a size: free device memory / BAMC_AUTO_DIV, clamped; or, for TELR_BAM_CHUNK_FIT and a load whose file bytes and
// inflated stream (fit_bytes together) stay below half the free memory, one chunk
static int bamc_auto_chunk(telr_ctx *ctx, int64_t fit_bytes, int64_t *chunk_bytes)
{
    if (*chunk_bytes > 0) return TELR_OK;
    int64_t fr = 0;
    TRY(telr_device_mem(ctx, &fr, nullptr));
    if (*chunk_bytes == TELR_BAM_CHUNK_FIT && fit_bytes < fr / 2) *chunk_bytes = BAMC_WHOLE;
    else *chunk_bytes = std::min<int64_t>(std::max<int64_t>(fr / BAMC_AUTO_DIV, BAMC_AUTO_MIN), BAMC_AUTO_MAX);
    return TELR_OK;
}

// what pass 1 leaves for the host: the records of the file, or the selected ones of a region load.  who(r), in the functions below: how an
// error text names record r of them
struct BamPass1 {
    std::vector<BamRec> recs; std::vector<int64_t> noff = std::vector<int64_t>(1, 0); std::vector<char> names;
    std::vector<int64_t> rec0, carry_in, cut;      // per chunk: its first record, the carry it started with, where its walk ended
    int64_t max_carry = 0;
    std::vector<int64_t> noff_k;      // (bam_load_fetch's landing place for one chunk's name offsets)
};
// The tail of pass 1 for one chunk, whichever way its n records came about: their fields, offsets in `buf` and name lengths are on the
// device (k_bam_rec's own, or the gathered ones of a region load).  The name lengths are scanned and k_bam_names writes the names; fields,
// name offsets and names come to the host behind what P1 holds; the lowest record that broke a rule is the error, named by who(its number)
template <class Who>
static int bam_load_fetch(telr_ctx *ctx, const uint8_t *buf, const BamRec *d_recs, const int64_t *d_offs, const int32_t *d_nlen, int64_t n, BamPass1 &P1, Who who)
{
    hipStream_t st = ctx->stream;
    int64_t *d_noff, *d_ntot, ntot = 0; uint8_t *d_names;
    TRY(ctx_buf_t(ctx, "bamin_noff", (size_t)n + 2, &d_noff));
    TRY(ctx_buf_t(ctx, "bamin_ntot", 2, &d_ntot));
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_nlen, (int32_t)n, d_noff, d_ntot, 0, nullptr, nullptr)));
    HIPCHK(hipMemcpyAsync(&ntot, d_ntot, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    TRY(ctx_buf_t(ctx, "bamin_names", (size_t)ntot + 1, &d_names));
    hipLaunchKernelGGL(k_bam_names, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, buf, d_offs, n, d_nlen, d_noff, d_names);
    HIPCHK(hipGetLastError());
    const size_t nb = P1.names.size();
    const int64_t base = (int64_t)P1.recs.size();
    P1.recs.resize((size_t)(base + n)); P1.noff_k.resize((size_t)n + 1); P1.names.resize(nb + (size_t)ntot);
    HIPCHK(hipMemcpyAsync(P1.recs.data() + base, d_recs, (size_t)n * sizeof(BamRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(P1.noff_k.data(), d_noff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (ntot) HIPCHK(hipMemcpyAsync(P1.names.data() + nb, d_names, (size_t)ntot, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t i = 1; i <= n; ++i) P1.noff.push_back((int64_t)nb + P1.noff_k[(size_t)i]);
    return bam_in_rec_fault(ctx, P1.recs.data() + base, n, base, who);
}
// What a load does behind pass 1, whichever way its chunks came about: the host decides on all records (P1.recs), the result's arrays and
// the set are made, and pass 2 writes the kept records' words and the reads' bases where they stay; with more than one chunk, each is
// uploaded and inflated again into its slot.  The handle takes the set and the result
template <class Who>
static int bam_load_pass2(telr_ctx *ctx, telr_bam_in *B, BamChunked &C, BamPass1 &P1, int32_t keep_qual, BamInClock &clk, Who who, int64_t *passes)
{
    std::vector<BamRec> &recs = P1.recs; std::vector<int64_t> &noff = P1.noff, &rec0 = P1.rec0, &carry_in = P1.carry_in, &cut = P1.cut; std::vector<char> &names = P1.names;
    const int64_t nch = C.nch, max_carry = P1.max_carry;
    hipStream_t st = C.s_main;
    // ---- host: names -> read numbers; which records are kept, and where
    clk.lap();
    names.push_back(0);
    BamInDecided D;
    TRY(bam_in_decide(ctx, B, recs, names, noff, D));
    const int32_t nq = (int32_t)D.reads.size();
    const size_t nk = D.kept_rec.size();
    std::unique_ptr<telr_result> R(std::move(D.R));
    std::vector<int32_t> kept_at(recs.size(), -1);             // record -> its place among the kept ones: pass 2 meets them in file order
    for (size_t i = 0; i < nk; ++i) kept_at[(size_t)D.kept_rec[i]] = (int32_t)i;
    B->phase_ms[BIN_NAMES_HOST] = clk.lap();
    // ---- the result's arrays and the set, final from the start
    TRY(bam_in_result_arrays(ctx, R.get(), D.ncig));
    telr_seqset *S = new telr_seqset();
    S->ctx = ctx; S->n = nq; S->len = D.rlen;
    TRY(seqset_alloc(ctx, S, "telr_bam_load", true, st));          // (frees S on failure)
    std::unique_ptr<telr_seqset, void (*)(telr_seqset*)> Sg(S, telr_seqset_free);
    const bool with_qual = nq && keep_qual && !D.any_ff;
    if (with_qual) {
        HIPCHK(hipMalloc(&S->d_qual, (size_t)S->padded_bases + 64));
        HIPCHK(hipMemsetAsync(S->d_qual + S->padded_bases, 0, 64, st));
    }
    // ---- pass 2: the kept records' words and the reads' bases go where they stay.  More than one chunk: each is uploaded and inflated
    // again.  One chunk: slot 0 holds it where pass 1 left it (carry_in[0] == 0) and "bamin_recs" holds its records' fields
    *passes = 1;
    if (nq || nk) {
        *passes = 2;
        const bool again = nch > 1;
        // (keep 0: a room that grew would drop the members behind it.  One chunk has no carry, max_carry is 0 and its room stays)
        for (int i = 0; i < C.nslot; ++i) TRY(bamc_room(C, C.slot[i], (size_t)max_carry, 0));
        std::vector<int32_t> h_idx, h_over; std::vector<int64_t> h_off;
        int32_t q = 0;
        if (again) TRY(bamc_issue(C, 0));
        for (int64_t k = 0; k < nch; ++k) {
            if (again) TRY(bamc_wait(C, k));
            BamChunkSlot &s = C.at(k);
            const uint8_t *buf = s.d_buf + s.room - carry_in[(size_t)k];
            const int64_t r0 = rec0[(size_t)k], r1 = rec0[(size_t)k + 1];
            h_idx.clear(); h_off.clear();
            for (int64_t r = r0; r < r1; ++r) if (kept_at[(size_t)r] >= 0) { h_idx.push_back((int32_t)(r - r0)); h_off.push_back(D.kept_off[(size_t)kept_at[(size_t)r]]); }
            if (!h_idx.empty()) {
                const size_t n = h_idx.size();
                BamRec *d_recs; int32_t *d_krec; int64_t *d_koff;
                TRY(ctx_buf_t(ctx, "bamin_recs", (size_t)(r1 - r0), &d_recs));
                TRY(ctx_buf_t(ctx, "bamin_krec", n, &d_krec));
                TRY(ctx_buf_t(ctx, "bamin_koff", n, &d_koff));
                if (again) HIPCHK(hipMemcpyAsync(d_recs, recs.data() + r0, (size_t)(r1 - r0) * sizeof(BamRec), hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(d_krec, h_idx.data(), n * 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(d_koff, h_off.data(), n * 8, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_bam_cig, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, buf, d_recs, d_krec, d_koff, (int64_t)n, R->d_cig);
                HIPCHK(hipGetLastError());
            }
            const int32_t q0 = q;
            while (q < nq && D.first_rec[(size_t)q] < r1) ++q;
            const int32_t nqk = q - q0;
            int32_t *d_over = nullptr;
            if (nqk) {
                BamRead *d_reads;
                TRY(ctx_buf_t(ctx, "bamin_reads", (size_t)nqk, &d_reads));
                HIPCHK(hipMemcpyAsync(d_reads, D.reads.data() + q0, (size_t)nqk * sizeof(BamRead), hipMemcpyHostToDevice, st));
                const int64_t b0 = S->boff[(size_t)q0], b1 = S->boff[(size_t)q];
                hipLaunchKernelGGL(k_bam_seq, grid256((b1 - b0) / 16), dim3(256), 0, st, buf, d_reads, S->d_boff + q0, nqk, b0 / 16, b1 / 16, S->d_seq2, S->d_nmask);
                HIPCHK(hipGetLastError());
                if (with_qual) {
                    TRY(ctx_buf_t(ctx, "bamin_over", (size_t)nqk, &d_over));
                    HIPCHK(hipMemsetAsync(d_over, 0, (size_t)nqk * 4, st));
                    hipLaunchKernelGGL(k_bam_qual, grid256((b1 - b0) / 4), dim3(256), 0, st, buf, d_reads, S->d_boff + q0, nqk, b0 / 4, b1 / 4, (uint32_t*)S->d_qual, d_over);
                    HIPCHK(hipGetLastError());
                    h_over.resize((size_t)nqk);
                    HIPCHK(hipMemcpyAsync(h_over.data(), d_over, (size_t)nqk * 4, hipMemcpyDeviceToHost, st));
                }
            }
            if (k + 1 < nch) TRY(bamc_issue(C, k + 1));
            HIPCHK(hipStreamSynchronize(st));
            if (d_over)          // (reads are numbered in file order of their records: the first one found is the lowest record)
                for (int32_t j = 0; j < nqk; ++j) if (h_over[(size_t)j]) {
                    ctx->err = "telr_bam_load: record " + who(D.first_rec[(size_t)(q0 + j)]) + ": a base quality above 93"; return TELR_E_ARG;
                }
            if (k + 1 < nch) TRY(bamc_carry(C, k, buf + cut[(size_t)k], carry_in[(size_t)k + 1], (size_t)C.payload(k + 1)));
        }
        if (D.ncig) HIPCHK(hipMemcpyAsync(R->cig, R->d_cig, (size_t)D.ncig * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    R->twin_n = R->ncig; R->twin_off = false;
    B->phase_ms[BIN_SEQ] = clk.lap();
    B->phase_ms[BIN_UPLOAD] = C.ms_upload; B->phase_ms[BIN_INFLATE] = C.ms_inflate;
    bam_in_finish(B, Sg.release(), R.release());
    return TELR_OK;
}

// the load.  chunk_bytes BAMC_WHOLE: the whole file as one chunk in one slot.  report: the handle's chunk_info is filled
static int bam_load(telr_ctx *ctx, const BamInHop &H, int32_t keep_qual, int64_t chunk_bytes, bool report, telr_bam_in **out)
{
    BamInClock wall, clk;
    std::unique_ptr<telr_bam_in, void (*)(telr_bam_in*)> B(new telr_bam_in(), telr_bam_in_free);
    B->ctx = ctx;
    B->counters[0] = (int64_t)H.mem.size(); B->counters[8] = H.no_eof;
    B->phase_ms[BIN_HOP] = H.ms;
    HIPCHK(hipSetDevice(ctx->device));
    BamChunked C(ctx, H);
    TRY(bamc_setup(C, chunk_bytes, 1));
    hipStream_t st = C.s_main;
    const int64_t nch = C.nch, nrun = std::max<int64_t>(nch, 1);      // (a file without members: one empty chunk, for the header's error)
    // ---- pass 1: every chunk's records and names
    BamPass1 P1;
    std::vector<int64_t> &rec0 = P1.rec0, &carry_in = P1.carry_in, &cut = P1.cut;
    rec0.assign((size_t)nrun + 1, 0); carry_in.assign((size_t)nrun + 1, 0); cut.assign((size_t)nrun, 0);
    const auto who = [](int64_t r) { return std::to_string(r); };      // a record is named by its number in the file
    bool hdr = false;
    int64_t carry = 0, &max_carry = P1.max_carry;
    int32_t n_ref = 0;
    float ms_parse = 0;
    if (nch) TRY(bamc_issue(C, 0));
    for (int64_t k = 0; k < nrun; ++k) {
        const bool last = k + 1 >= nrun;
        if (nch) TRY(bamc_wait(C, k));
        BamChunkSlot &s = C.at(k);
        const int64_t buflen = carry + (nch ? C.payload(k) : 0);
        uint8_t *buf = s.d_buf + s.room - carry;
        carry_in[(size_t)k] = carry; max_carry = std::max(max_carry, carry);
        int64_t from = 0;
        if (!hdr) {
            // the header: small, parsed on the host; incomplete in a chunk that is not the last: the whole buffer is carried on
            std::vector<uint8_t> h;
            int64_t have = std::min<int64_t>(buflen, 1 << 16), need = 0;
            for (;;) {
                h.resize((size_t)have + 1);
                if (have) HIPCHK(hipMemcpy(h.data(), buf, (size_t)have, hipMemcpyDeviceToHost));
                const int rc = bam_in_header(ctx, h.data(), have, last ? buflen : INT64_MAX / 2, B.get(), &from, &need);
                if (rc == TELR_OK) { hdr = true; break; }
                if (rc != 1) return rc;
                if (have == buflen) break;
                have = std::min<int64_t>(buflen, std::max<int64_t>(need, have * 4));
            }
            n_ref = (int32_t)B->tnames.size();
        }
        int64_t nrec_k = 0, p_end = 0, *d_offs = nullptr, *d_res = nullptr;
        if (hdr) {
            const int64_t cap = (buflen - from) / 36 + 1;
            TRY(ctx_buf_t(ctx, "bamin_offs", (size_t)cap + 1, &d_offs));
            TRY(ctx_buf_t(ctx, "bamin_res", 3, &d_res));
            HIPCHK(hipEventRecord(C.ec0, st));
            hipLaunchKernelGGL(k_bam_chain, dim3(1), dim3(64), 0, st, buf, buflen, from, d_offs, cap, d_res);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(C.ec1, st));
        }
        if (k + 1 < nch) TRY(bamc_issue(C, k + 1));          // (the host is busy with the upload while the chain walks)
        if (hdr) {
            int64_t res[3] = {0, 0, 0};
            HIPCHK(hipMemcpyAsync(res, d_res, 24, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            float ms = 0; HIPCHK(hipEventElapsedTime(&ms, C.ec0, C.ec1)); C.ms_chain += ms;
            clk.lap();
            const int64_t base = rec0[(size_t)k];
            if (res[1] == 1 && last) { ctx->err = "telr_bam_load: record " + std::to_string(base + res[0]) + ": runs past the stream"; return TELR_E_ARG; }
            if (res[1] == 2) { ctx->err = "telr_bam_load: record " + std::to_string(base + res[0]) + ": block_size below 32"; return TELR_E_ARG; }
            if (res[1] == 3 || base + res[0] >= 0x7ffffff0LL) { ctx->err = "telr_bam_load: too many records"; return TELR_E_RANGE; }
            nrec_k = res[0]; p_end = res[2];
            if (nrec_k) {
                BamRec *d_recs; int32_t *d_nlen;
                TRY(ctx_buf_t(ctx, "bamin_recs", (size_t)nrec_k, &d_recs));
                TRY(ctx_buf_t(ctx, "bamin_nlen", (size_t)nrec_k + 1, &d_nlen));
                hipLaunchKernelGGL(k_bam_rec, dim3((unsigned)((nrec_k + 3) / 4)), dim3(256), 0, st, buf, d_offs, nrec_k, n_ref, d_recs, d_nlen);
                HIPCHK(hipGetLastError());
                TRY(bam_load_fetch(ctx, buf, d_recs, d_offs, d_nlen, nrec_k, P1, who));
            }
            ms_parse += clk.lap();
        }
        rec0[(size_t)k + 1] = rec0[(size_t)k] + nrec_k;
        cut[(size_t)k] = p_end;
        carry = buflen - p_end;
        if (!last) TRY(bamc_carry(C, k, buf + p_end, carry, (size_t)C.payload(k + 1)));
    }
    B->phase_ms[BIN_CHAIN] = C.ms_chain; B->phase_ms[BIN_PARSE] = ms_parse;
    int64_t passes = 1;
    TRY(bam_load_pass2(ctx, B.get(), C, P1, keep_qual, clk, who, &passes));
    B->phase_ms[BIN_TOTAL] = wall.lap() + H.ms;
    if (report) { B->chunk_info[0] = nch; B->chunk_info[1] = passes; B->chunk_info[2] = (int64_t)C.max_alloc; B->chunk_info[3] = max_carry; }
    *out = B.release();
    return TELR_OK;
}

extern "C" int telr_bam_chunk_plan(int64_t n_members, const int32_t *isize, int64_t chunk_bytes, int64_t *first_member_of_chunk, int64_t cap, int64_t *n_chunks)
{
    return bam_chunk_plan(n_members, isize, chunk_bytes, first_member_of_chunk, cap, n_chunks);
}

extern "C" int telr_bam_load(telr_ctx *ctx, const char *path, int32_t keep_qual, telr_bam_in **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    if (!path || !out) { ctx->err = "telr_bam_load: null path or output"; return TELR_E_ARG; }
    BamInHop H;
    TRY(bam_in_hop(ctx, "telr_bam_load", path, H));
    return bam_load(ctx, H, keep_qual, BAMC_WHOLE, false, out);
}

extern "C" int telr_bam_load_chunked(telr_ctx *ctx, const char *path, int32_t keep_qual, int64_t chunk_bytes, telr_bam_in **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    if (!path || !out) { ctx->err = "telr_bam_load_chunked: null path or output"; return TELR_E_ARG; }
    if (chunk_bytes < TELR_BAM_CHUNK_FIT) { ctx->err = "telr_bam_load_chunked: chunk_bytes below TELR_BAM_CHUNK_FIT"; return TELR_E_ARG; }
    BamInHop H;
    TRY(bam_in_hop(ctx, "telr_bam_load", path, H));
    const bool fit = chunk_bytes == TELR_BAM_CHUNK_FIT;
    TRY(bamc_auto_chunk(ctx, (int64_t)H.F.n + H.total, &chunk_bytes));
    return bam_load(ctx, H, keep_qual, chunk_bytes, !(fit && chunk_bytes == BAMC_WHOLE), out);          // (a file that fits: telr_bam_load, which reports no chunks)
}

// test tap: the inflated stream of a BGZF file (any payload) -> out[0 .. cap); *n = its length (nothing is copied when it exceeds cap)
extern "C" int telr_debug_bgzf_inflate(telr_ctx *ctx, const char *path, uint8_t *out, int64_t cap, int64_t *n)
{
    (void)hipGetLastError();
    if (!ctx || !path || !n) return TELR_E_ARG;
    BamInHop H;
    TRY(bam_in_hop(ctx, "telr_debug_bgzf_inflate", path, H));
    HIPCHK(hipSetDevice(ctx->device));
    BamChunked C(ctx, H);
    C.what = "telr_debug_bgzf_inflate";
    const uint8_t *d = nullptr;
    TRY(bamc_inflate_whole(C, &d));
    *n = H.total;
    if (H.total && H.total <= cap && out) HIPCHK(hipMemcpy(out, d, (size_t)H.total, hipMemcpyDeviceToHost));
    return TELR_OK;
}
