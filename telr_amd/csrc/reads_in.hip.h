// reads_in.hip.h -- telr_reads_load: a FASTA / FASTQ file -- plain, gzip or BGZF -- becomes a read set on the device without its text
// ever being held as host text (the definition is in include/telr_hip.h and, as plain Python, in tests/reads_in_ref.py).
//
//   host      map the file; the BGZF hop of bam_in.hip.h over the whole file decides the container: BGZF where it accepts the file, gzip
//             for any other file that opens 1f 8b, plain for one that opens '@' or '>'
//   chunks    BGZF: telr_bam_chunk_plan over the members' ISIZE; upload + k_bgzf_inflate (bam_in_chunked.hip.h: its slots, its carry)
//             gzip: ONE host thread runs zlib's inflate into two pinned buffers, chunk_bytes of text at a time; plain: the mapped bytes
//             text chunks below 4 KiB that close no record (fewer than four line feeds / no '>') are gathered on the host, up to 4 KiB
//   device    k_rt_line_count, scan, k_rt_line_write     one lane per 16 text bytes: where the lines start
//             k_rt_fastq_rec                             one lane per record: its four lines checked (rt_fastq_record)
//             k_rt_fa_lines, two scans, k_rt_fa_heads, k_rt_fa_rec    FASTA: header flag and bases per line -> records and the running sum
//             scans of name lengths and 64-base groups, k_rt_summary  the lowest record that is not OK, the totals, the carry's start
//             k_rt_names                                 the names into one compact buffer -> one copy to the host
//             k_rt_pack<MULTI>, k_rt_qual                one lane per 2-bit word / per 4 Phred bytes of the chunk's piece of the set
//   join      the pieces are copied end to end into the set's arrays (two sets end to end are the set of the concatenated lengths)
// One pass: a chunk's words do not depend on a later chunk.  Every store position is a scan's result or the lane's own index; no atomic;
// the same bytes on every run.  Every text load is a whole aligned qword or wider (reads_text_core.h).
#include "reads_text_core.h"
#include <condition_variable>
#include <mutex>
#include <zlib.h>

#define RT_GATHER 4096          /* text chunks are gathered on the host up to this many bytes while they close no record */

// ---- lines ------------------------------------------------------------------------------------------------------------------------
// the 16 bytes of aligned block i as a mask of its line feeds, inside text bytes [bias, bias + len) only
static __device__ __forceinline__ uint32_t rt_lf_mask(const uint4 *__restrict__ blk, int64_t i, int64_t bias, int64_t len)
{
    const uint4 v = blk[i];
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    uint32_t m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t x = w[d] ^ 0x0a0a0a0au;
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);          // 0x80 in the bytes that are '\n'
        m |= ((z >> 7 & 1u) | (z >> 14 & 2u) | (z >> 21 & 4u) | (z >> 28 & 8u)) << (4 * d);
    }
    const int64_t g0 = 16 * i, lo = bias - g0, hi = bias + len - g0;          // valid bytes of the block: [lo, hi)
    if (lo > 0) m &= ~((1u << lo) - 1u);
    if (hi < 16) m &= (1u << hi) - 1u;
    return m;
}
// cnt[i] = line feeds in block i; res[1] = the text's last byte
__global__ void __launch_bounds__(256) k_rt_line_count(const uint4 *__restrict__ blk, int64_t bias, int64_t len, int32_t nblk, int32_t *__restrict__ cnt,
                                                       int64_t *__restrict__ res)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nblk) return;
    cnt[i] = __popc(rt_lf_mask(blk, i, bias, len));
    if (i == nblk - 1) {
        const int64_t k = bias + len - 1;
        res[1] = (int64_t)((((const uint32_t*)blk)[k >> 2] >> ((k & 3) * 8)) & 0xffu);
    }
}
// ls[0] = 0, ls[r] = the offset behind the r-th line feed
__global__ void __launch_bounds__(256) k_rt_line_write(const uint4 *__restrict__ blk, int64_t bias, int64_t len, int32_t nblk, const int64_t *__restrict__ rank,
                                                       int64_t *__restrict__ ls)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nblk) return;
    if (i == 0) ls[0] = 0;
    uint32_t m = rt_lf_mask(blk, i, bias, len);
    int64_t r = rank[i];
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1u;
        ls[++r] = 16 * i + b - bias + 1;
    }
}

// ---- records ----------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ void rt_store_rec(const RtRec &R, int64_t r, RtRec *__restrict__ recs, int32_t *__restrict__ nlen, int32_t *__restrict__ grp,
                                                    int32_t *__restrict__ lens)
{
    const bool ok = R.status == RTS_OK;
    recs[r] = R; lens[r] = R.len;
    nlen[r] = ok ? R.name_len : 0;
    grp[r] = ok ? (int32_t)(((int64_t)R.len + 63) >> 6) : 0;
}
__global__ void __launch_bounds__(256) k_rt_fastq_rec(RtText T, const int64_t *__restrict__ ls, int64_t nl, int64_t nlines, int64_t n, RtRec *__restrict__ recs,
                                                      int32_t *__restrict__ nlen, int32_t *__restrict__ grp, int32_t *__restrict__ lens)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    rt_store_rec(rt_fastq_record(T, ls, nl, nlines, r), r, recs, nlen, grp, lens);
}
// FASTA, one lane per line: is it a header, and how many bases does it add
__global__ void __launch_bounds__(256) k_rt_fa_lines(RtText T, const int64_t *__restrict__ ls, int64_t nl, int64_t nlines, int32_t *__restrict__ hflag, int64_t *__restrict__ nb)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nlines) return;
    int64_t s, e;
    rt_line(T, ls, nl, j, &s, &e);
    const bool h = e > s && rt_byte(T, s) == '>';
    hflag[j] = h ? 1 : 0;
    nb[j] = h ? 0 : e - s;
}
// hl[k] = the line of the k-th header (its rank in the scan of the flags), hl[nh] = the number of lines
__global__ void __launch_bounds__(256) k_rt_fa_heads(const int32_t *__restrict__ hflag, const int32_t *__restrict__ hrank, int64_t nlines, int64_t nh, int64_t *__restrict__ hl)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j == 0) hl[nh] = nlines;
    if (j >= nlines) return;
    if (hflag[j]) hl[hrank[j]] = j;
}
__global__ void __launch_bounds__(256) k_rt_fa_rec(RtText T, const int64_t *__restrict__ ls, int64_t nl, const int64_t *__restrict__ S, const int64_t *__restrict__ hl, int64_t n,
                                                   RtRec *__restrict__ recs, int32_t *__restrict__ nlen, int32_t *__restrict__ grp, int32_t *__restrict__ lens)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    rt_store_rec(rt_fasta_record(T, ls, nl, S, hl[r], hl[r + 1]), r, recs, nlen, grp, lens);
}
// One workgroup.  res[0] = the lowest record whose status is not RTS_OK (n: none), res[1] = its status, res[2] = 1 when a record before it
// has bases on several lines, res[3] / res[4] = the name bytes / 64-base groups of the records before it, res[5] = where the carry
// starts (ls[cut_line], FASTA: ls[hl[cut_line]]; cut_line < 0: 0), res[6] = that line
__global__ void __launch_bounds__(256) k_rt_summary(const RtRec *__restrict__ recs, int64_t n, const int64_t *__restrict__ noff, const int64_t *__restrict__ goff,
                                                    const int64_t *__restrict__ ls, const int64_t *__restrict__ hl, int64_t cut_line, int64_t *__restrict__ res)
{
    __shared__ int64_t s[256];
    const int tid = threadIdx.x;
    int64_t first = n;
    for (int64_t r = tid; r < n; r += 256) if (recs[r].status != RTS_OK) { first = r; break; }
    s[tid] = first;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) { if (tid < o) s[tid] = s[tid + o] < s[tid] ? s[tid + o] : s[tid]; __syncthreads(); }
    first = s[0];
    __syncthreads();
    int64_t multi = 0;
    for (int64_t r = tid; r < first; r += 256) multi |= recs[r].multi;
    s[tid] = multi;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) { if (tid < o) s[tid] |= s[tid + o]; __syncthreads(); }
    if (tid != 0) return;
    res[0] = first; res[1] = first < n ? recs[first].status : RTS_OK; res[2] = s[0];
    res[3] = n ? noff[first] : 0; res[4] = n ? goff[first] : 0;
    const int64_t line = cut_line < 0 ? 0 : hl ? hl[cut_line] : cut_line;
    res[5] = cut_line < 0 ? 0 : ls[line]; res[6] = line;
}
// the names behind one another: record r's at noff[r].  One lane per record, 8 text bytes per load
__global__ void __launch_bounds__(256) k_rt_names(RtText T, const RtRec *__restrict__ recs, const int64_t *__restrict__ ls, int64_t n, const int64_t *__restrict__ noff,
                                                  uint8_t *__restrict__ names)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const RtRec R = recs[r];
    const int64_t src = ls[R.first_line] + 1;
    uint8_t *d = names + noff[r];
    for (int32_t k = 0; k < R.name_len; k += 8) {
        const uint64_t x = rt_load8(T, src + k);
        const int m = R.name_len - k < 8 ? R.name_len - k : 8;
        for (int b = 0; b < m; ++b) d[k + b] = (uint8_t)(x >> (8 * b));
    }
}

// ---- the set's words ----------------------------------------------------------------------------------------------------------------
// the last record whose first 64-base group is at or before group g
static __device__ __forceinline__ int64_t rt_rec_of(const int64_t *__restrict__ goff, int64_t n, int64_t g)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (goff[mid] <= g) lo = mid + 1; else hi = mid; }
    return lo - 1;
}
// one lane per 2-bit word of the chunk's piece (16 bases), the mask words from lane pairs (nw is a multiple of 4).  MULTI: a record may
// have its bases on several lines (FASTA); a launch without it never looks at S
template <bool MULTI>
__global__ void __launch_bounds__(256) k_rt_pack(RtText T, const RtRec *__restrict__ recs, const int64_t *__restrict__ goff, int64_t n, const int64_t *__restrict__ ls,
                                                 const int64_t *__restrict__ S, int64_t nw, uint32_t *__restrict__ out2, uint32_t *__restrict__ outn)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;
    const int64_t q = rt_rec_of(goff, n, w >> 2);
    const RtRec R = recs[q];
    const int64_t j0 = (w - goff[q] * 4) * 16, left = (int64_t)R.len - j0;
    const int v = left >= 16 ? 16 : left > 0 ? (int)left : 0;
    uint64_t lo, hi;
    if (MULTI && R.multi && v > 0) rt_fasta_gather16(T, ls, S, R.first_line, R.first_line + 1 + R.n_lines, S[R.first_line] + j0, v, lo, hi);
    else rt_load16(T, v > 0 ? R.seq_pos + j0 : 0, lo, hi);
    uint32_t code, m16;
    rt_pack16(lo, hi, v, code, m16);
    out2[w] = code;
    const uint32_t other = __shfl_xor(m16, 1);
    if (!(w & 1)) outn[w >> 1] = m16 | (other << 16);
}
// one lane per 4 Phred bytes of the piece (nw4 is a multiple of 16); wbad[wave] = the lowest record of the wave with a character outside
// 33..126, INT32_MAX without one
__global__ void __launch_bounds__(256) k_rt_qual(RtText T, const RtRec *__restrict__ recs, const int64_t *__restrict__ goff, int64_t n, int64_t nw4,
                                                 uint32_t *__restrict__ out4, int32_t *__restrict__ wbad)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t mine = 0x7fffffff;
    if (w < nw4) {
        const int64_t q = rt_rec_of(goff, n, w >> 4);
        const RtRec R = recs[q];
        const int64_t j0 = (w - goff[q] * 16) * 4, left = (int64_t)R.len - j0;
        const int v = left >= 4 ? 4 : left > 0 ? (int)left : 0;
        bool bad;
        out4[w] = rt_qual4((uint32_t)rt_load8(T, v > 0 ? R.qual_pos + j0 : 0), v, &bad);
        if (bad) mine = (int32_t)q;
    }
    for (int o = 32; o >= 1; o >>= 1) { const int32_t x = __shfl_xor(mine, o); mine = x < mine ? x : mine; }
    if ((threadIdx.x & 63) == 0) wbad[((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6] = mine;
}
// one workgroup: res[0] = the least of v[0 .. n)
__global__ void __launch_bounds__(256) k_rt_min32(const int32_t *__restrict__ v, int64_t n, int64_t *__restrict__ res)
{
    __shared__ int32_t s[256];
    const int tid = threadIdx.x;
    int32_t m = 0x7fffffff;
    for (int64_t i = tid; i < n; i += 256) m = v[i] < m ? v[i] : m;
    s[tid] = m;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) { if (tid < o) s[tid] = s[tid + o] < s[tid] ? s[tid + o] : s[tid]; __syncthreads(); }
    if (tid == 0) res[0] = s[0];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
enum { RIN_HOP, RIN_UPLOAD, RIN_INFLATE, RIN_LINES, RIN_RECORDS, RIN_NAMES, RIN_PACK, RIN_JOIN, RIN_TOTAL, RIN_NPHASE };
enum { RIN_PLAIN = 0, RIN_GZIP = 1, RIN_BGZF = 2 };
struct telr_reads_in {
    telr_ctx *ctx = nullptr;
    std::vector<std::string> qnames; std::vector<const char*> qname_ptr;
    telr_seqset *set = nullptr; bool set_owned = true;
    int64_t counters[8] = {0};         // container, fastq, members, text_bytes, lines, records, bases, no_eof
    int64_t chunk_info[4] = {0};       // chunks, largest buffer, largest carry, peak transient bytes
    float phase_ms[RIN_NPHASE] = {0};
};
extern "C" void telr_reads_in_free(telr_reads_in *in)
{
    if (!in) return;
    if (in->set && in->set_owned) telr_seqset_free(in->set);
    delete in;
}

// the pieces' memory: slabs of at least 1 MiB, freed with the load
struct RtSlabs {
    std::vector<void*> slabs; uint8_t *cur = nullptr; size_t left = 0, total = 0;
    ~RtSlabs() { for (void *p : slabs) (void)hipFree(p); }
    int get(telr_ctx *ctx, size_t bytes, void **out)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes > left) {
            const size_t sz = std::max<size_t>(bytes, (size_t)1 << 20);
            void *p = nullptr;
            HIPCHK(hipMalloc(&p, sz));
            slabs.push_back(p); cur = (uint8_t*)p; left = sz; total += sz;
        }
        *out = cur; cur += bytes; left -= bytes;
        return TELR_OK;
    }
};
struct RtPiece { uint32_t *w2, *wn; uint8_t *q; int64_t groups; };

static size_t rt_marks(const uint8_t *p, size_t n, bool fastq)
{
    const uint8_t c = fastq ? '\n' : '>';
    size_t k = 0;
    for (const uint8_t *e = p + n; p < e && (p = (const uint8_t*)memchr(p, c, (size_t)(e - p))); ++p) ++k;
    return k;
}

// gzip: one thread inflates the file's members (window bits 47, reset at each member's end) into two pinned buffers in turn
struct RtGzip {
    const uint8_t *src = nullptr; size_t n = 0, ipos = 0, chunk = 0;
    uint8_t *pin[2] = { nullptr, nullptr };
    size_t len[2] = { 0, 0 }; bool full[2] = { false, false }, last[2] = { false, false }, failed[2] = { false, false };
    std::string err; int64_t members = 0; float ms = 0;
    z_stream z; bool z_on = false, stop = false, fastq = false;
    std::mutex m; std::condition_variable cv; std::thread th;
    ~RtGzip()
    {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
        if (z_on) inflateEnd(&z);
    }
    void run()
    {
        bool boundary = true, end = false;
        for (int64_t k = 0; !end && err.empty(); ++k) {
            const int i = (int)(k & 1);
            { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return stop || !full[i]; }); if (stop) return; }
            BamInClock clk;
            size_t take = 0, marks = 0;
            do {
                const size_t c0 = take;
                size_t want = chunk;
                while (want && !end && err.empty()) {
                    if (z.avail_in == 0) { const size_t c = std::min<size_t>(n - ipos, (size_t)1 << 30); z.next_in = (Bytef*)(src + ipos); z.avail_in = (uInt)c; ipos += c; }
                    if (z.avail_in == 0) { if (boundary) end = true; else err = "gzip: the file ends inside a member"; break; }
                    const uInt out0 = (uInt)std::min<size_t>(want, (size_t)1 << 30), in0 = z.avail_in;
                    z.next_out = pin[i] + take; z.avail_out = out0;
                    const int rc = inflate(&z, Z_NO_FLUSH);
                    const size_t got = out0 - z.avail_out;
                    take += got; want -= got;
                    if (rc == Z_STREAM_END) { ++members; boundary = true; if (z.avail_in == 0 && ipos == n) end = true; else inflateReset(&z); }
                    else if (rc == Z_OK || rc == Z_BUF_ERROR) { if (z.avail_in != in0 || got) boundary = false; }
                    else err = std::string("gzip: ") + (z.msg ? z.msg : "zlib error") ;
                }
                if (k == 0 && c0 == 0 && take) fastq = pin[i][0] == '@';
                if (chunk < RT_GATHER) marks += rt_marks(pin[i] + c0, take - c0, fastq);
            } while (!end && err.empty() && marks < (fastq ? 4u : 1u) && take < RT_GATHER);
            ms += clk.lap();
            { std::lock_guard<std::mutex> lk(m); len[i] = take; last[i] = end; failed[i] = !err.empty(); full[i] = true; }
            cv.notify_all();
        }
    }
    // chunk k, once it is there
    void get(int64_t k) { const int i = (int)(k & 1); std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return full[i]; }); }
    void give_back(int64_t k) { { std::lock_guard<std::mutex> lk(m); full[(int)(k & 1)] = false; } cv.notify_all(); }
};

struct RtLoad {
    telr_ctx *ctx; hipStream_t st; bool keep_qual;
    int kind = -1;                                   // 0 FASTA, 1 FASTQ
    std::vector<int32_t> lens, h_len; std::vector<std::string> names; std::vector<int64_t> h_noff; std::vector<char> h_names;
    RtSlabs slabs; std::vector<RtPiece> pieces;
    int64_t lines = 0, carry_lf = 0, bases = 0, groups = 0;
    hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    float ms[4] = { 0, 0, 0, 0 };                      // lines, records, names, pack
    RtLoad(telr_ctx *c, bool kq) : ctx(c), st(c->stream), keep_qual(kq) {}
    ~RtLoad() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

static int rt_fault(telr_ctx *ctx, int status, int64_t record)
{
    static const char *const why[] = RT_TEXTS;
    ctx->err = "telr_reads_load: record " + std::to_string(record) + ": " + why[status >= 0 && status <= 7 ? status : 0];
    return status == RTS_LONG ? TELR_E_RANGE : TELR_E_ARG;
}

// one chunk's buffer (the carry and the new text; 64 zero bytes behind it): its complete records -- all that is left when `last` -- join
// the load; *cut = where the carry for the next chunk starts
static int rt_parse(RtLoad &L, const uint8_t *buf, int64_t buflen, bool last, int64_t *cut)
{
    telr_ctx *ctx = L.ctx; hipStream_t st = L.st;
    *cut = last ? buflen : 0;
    if (buflen == 0) return TELR_OK;
    const bool fastq = L.kind == 1;
    const uintptr_t a0 = (uintptr_t)buf & ~(uintptr_t)15;
    RtText T; T.q = (const uint64_t*)a0; T.bias = (int64_t)((uintptr_t)buf - a0); T.len = buflen;
    const int64_t nblk = (T.bias + buflen + 15) / 16;
    if (nblk >= 0x7ffffff0LL) { ctx->err = "telr_reads_load: a chunk and its carry of 32 GiB or more"; return TELR_E_RANGE; }
    // ---- lines
    int32_t *d_cnt; int64_t *d_rank, *d_res, *d_ls, res[8] = {0};
    TRY(ctx_buf_t(ctx, "rin_cnt", (size_t)nblk + 1, &d_cnt));
    TRY(ctx_buf_t(ctx, "rin_rank", (size_t)nblk + 2, &d_rank));
    TRY(ctx_buf_t(ctx, "rin_res", 16, &d_res));
    HIPCHK(hipEventRecord(L.ev[0], st));
    hipLaunchKernelGGL(k_rt_line_count, grid256(nblk), dim3(256), 0, st, (const uint4*)a0, T.bias, buflen, (int32_t)nblk, d_cnt, d_res);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_cnt, (int32_t)nblk, d_rank, d_res, 0, nullptr, nullptr)));
    HIPCHK(hipMemcpyAsync(res, d_res, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t nl = res[0], nlines = last ? nl + (res[1] != '\n' ? 1 : 0) : nl;
    L.lines += nl - L.carry_lf + (nlines - nl);
    L.carry_lf = nl;
    if (!last && nl < (fastq ? 4 : 2)) return TELR_OK;          // no record can be complete: everything is carried on
    if (nlines >= 0x7ffffff0LL) { ctx->err = "telr_reads_load: too many lines in one chunk"; return TELR_E_RANGE; }
    TRY(ctx_buf_t(ctx, "rin_ls", (size_t)nl + 2, &d_ls));
    hipLaunchKernelGGL(k_rt_line_write, grid256(nblk), dim3(256), 0, st, (const uint4*)a0, T.bias, buflen, (int32_t)nblk, d_rank, d_ls);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(L.ev[1], st));
    // ---- records
    int64_t nrec = 0, cut_line = -1, *d_S = nullptr, *d_hl = nullptr;
    if (fastq) { nrec = last ? (nlines + 3) / 4 : nl / 4; cut_line = last ? -1 : 4 * nrec; }
    else {
        int32_t *d_hflag, *d_hrank; int64_t *d_nb, nh = 0;
        TRY(ctx_buf_t(ctx, "rin_hflag", (size_t)nlines + 1, &d_hflag));
        TRY(ctx_buf_t(ctx, "rin_hrank", (size_t)nlines + 2, &d_hrank));
        TRY(ctx_buf_t(ctx, "rin_nb", (size_t)nlines + 1, &d_nb));
        TRY(ctx_buf_t(ctx, "rin_S", (size_t)nlines + 2, &d_S));
        hipLaunchKernelGGL(k_rt_fa_lines, grid256(nlines), dim3(256), 0, st, T, d_ls, nl, nlines, d_hflag, d_nb);
        HIPCHK(hipGetLastError());
        TRY((dev_qscan<int32_t, int32_t>(ctx, d_hflag, (int32_t)nlines, d_hrank, d_res + 2, 0, nullptr, nullptr)));
        TRY((dev_qscan<int64_t, int64_t>(ctx, d_nb, (int32_t)nlines, d_S, nullptr, 0, nullptr, nullptr)));
        HIPCHK(hipMemcpyAsync(&nh, d_res + 2, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        TRY(ctx_buf_t(ctx, "rin_hl", (size_t)nh + 2, &d_hl));
        hipLaunchKernelGGL(k_rt_fa_heads, grid256(std::max<int64_t>(nlines, 1)), dim3(256), 0, st, d_hflag, d_hrank, nlines, nh, d_hl);
        HIPCHK(hipGetLastError());
        nrec = last ? nh : std::max<int64_t>(nh - 1, 0); cut_line = last ? -1 : nh - 1;
    }
    if (nrec >= 0x7ffffff0LL) { ctx->err = "telr_reads_load: too many records"; return TELR_E_RANGE; }
    RtRec *d_recs; int32_t *d_nlen, *d_grp, *d_len; int64_t *d_noff, *d_goff;
    TRY(ctx_buf_t(ctx, "rin_recs", (size_t)nrec, &d_recs));
    TRY(ctx_buf_t(ctx, "rin_nlen", (size_t)nrec + 1, &d_nlen));
    TRY(ctx_buf_t(ctx, "rin_grp", (size_t)nrec + 1, &d_grp));
    TRY(ctx_buf_t(ctx, "rin_len", (size_t)nrec + 1, &d_len));
    TRY(ctx_buf_t(ctx, "rin_noff", (size_t)nrec + 2, &d_noff));
    TRY(ctx_buf_t(ctx, "rin_goff", (size_t)nrec + 2, &d_goff));
    if (nrec) {
        if (fastq) hipLaunchKernelGGL(k_rt_fastq_rec, grid256(nrec), dim3(256), 0, st, T, d_ls, nl, nlines, nrec, d_recs, d_nlen, d_grp, d_len);
        else hipLaunchKernelGGL(k_rt_fa_rec, grid256(nrec), dim3(256), 0, st, T, d_ls, nl, d_S, d_hl, nrec, d_recs, d_nlen, d_grp, d_len);
        HIPCHK(hipGetLastError());
        TRY((dev_qscan<int32_t, int64_t>(ctx, d_nlen, (int32_t)nrec, d_noff, nullptr, 0, nullptr, nullptr)));
        TRY((dev_qscan<int32_t, int64_t>(ctx, d_grp, (int32_t)nrec, d_goff, nullptr, 0, nullptr, nullptr)));
    }
    hipLaunchKernelGGL(k_rt_summary, dim3(1), dim3(256), 0, st, d_recs, nrec, d_noff, d_goff, d_ls, d_hl, cut_line, d_res + 4);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(L.ev[2], st));
    HIPCHK(hipMemcpyAsync(res, d_res + 4, 56, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t base = (int64_t)L.lens.size(), nk = res[0], ntot = res[3], gtot = res[4];
    const int fault = nk < nrec && res[1] != RTS_NONE ? (int)res[1] : RTS_OK;          // (the records below it still go first: a quality of theirs is the lower fault)
    if (!last) { *cut = res[5]; L.carry_lf = nl - res[6]; }
    if (base + nk >= 0x7ffffff0LL) { ctx->err = "telr_reads_load: too many records"; return TELR_E_RANGE; }
    // ---- names, words, qualities
    if (nk) {
        uint8_t *d_names; int64_t bad = 0x7fffffff;
        TRY(ctx_buf_t(ctx, "rin_names", (size_t)ntot + 1, &d_names));
        hipLaunchKernelGGL(k_rt_names, grid256(nk), dim3(256), 0, st, T, d_recs, d_ls, nk, d_noff, d_names);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(L.ev[3], st));
        RtPiece P; P.w2 = P.wn = nullptr; P.q = nullptr; P.groups = gtot;
        const bool qual = L.keep_qual && fastq;
        if (gtot) {
            void *p;
            TRY(L.slabs.get(ctx, (size_t)gtot * 16, &p)); P.w2 = (uint32_t*)p;
            TRY(L.slabs.get(ctx, (size_t)gtot * 8, &p)); P.wn = (uint32_t*)p;
            const int64_t nw = gtot * 4;
            if (res[2]) hipLaunchKernelGGL(k_rt_pack<true>, grid256(nw), dim3(256), 0, st, T, d_recs, d_goff, nk, d_ls, d_S, nw, P.w2, P.wn);
            else hipLaunchKernelGGL(k_rt_pack<false>, grid256(nw), dim3(256), 0, st, T, d_recs, d_goff, nk, d_ls, d_S, nw, P.w2, P.wn);
            HIPCHK(hipGetLastError());
            if (qual) {
                TRY(L.slabs.get(ctx, (size_t)gtot * 64, &p)); P.q = (uint8_t*)p;
                const int64_t nw4 = gtot * 16, nwave = (int64_t)grid256(nw4).x * 4;
                int32_t *d_wbad;
                TRY(ctx_buf_t(ctx, "rin_wbad", (size_t)nwave, &d_wbad));
                hipLaunchKernelGGL(k_rt_qual, grid256(nw4), dim3(256), 0, st, T, d_recs, d_goff, nk, nw4, (uint32_t*)P.q, d_wbad);
                hipLaunchKernelGGL(k_rt_min32, dim3(1), dim3(256), 0, st, d_wbad, nwave, d_res + 12);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(&bad, d_res + 12, 8, hipMemcpyDeviceToHost, st));
            }
        }
        HIPCHK(hipEventRecord(L.ev[4], st));
        L.h_len.resize((size_t)nk); L.h_noff.resize((size_t)nk + 1); L.h_names.resize((size_t)ntot + 1);
        HIPCHK(hipMemcpyAsync(L.h_len.data(), d_len, (size_t)nk * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(L.h_noff.data(), d_noff, ((size_t)nk + 1) * 8, hipMemcpyDeviceToHost, st));
        if (ntot) HIPCHK(hipMemcpyAsync(L.h_names.data(), d_names, (size_t)ntot, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, L.ev[2], L.ev[3])); L.ms[2] += ms;
        HIPCHK(hipEventElapsedTime(&ms, L.ev[3], L.ev[4])); L.ms[3] += ms;
        if (bad != 0x7fffffff) return rt_fault(ctx, RTS_QUAL, base + bad);
        for (int64_t r = 0; r < nk; ++r) {
            L.lens.push_back(L.h_len[(size_t)r]); L.bases += L.h_len[(size_t)r];
            L.names.emplace_back(L.h_names.data() + L.h_noff[(size_t)r], (size_t)(L.h_noff[(size_t)r + 1] - L.h_noff[(size_t)r]));
        }
        L.groups += gtot;
        L.pieces.push_back(P);
    }
    { float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, L.ev[0], L.ev[1])); L.ms[0] += ms;
      HIPCHK(hipEventElapsedTime(&ms, L.ev[1], L.ev[2])); L.ms[1] += ms; }
    if (fault != RTS_OK) return rt_fault(ctx, fault, base + nk);
    return TELR_OK;
}

// text that comes from the host (gzip, plain) goes straight behind a slot's room (bamc_slots without the members' buffers: the layout
// of bam_in_chunked.hip.h, the payload C.max_payload bytes at the most)
static int rt_issue_host(BamChunked &C, int64_t k, const uint8_t *p, size_t n)
{
    telr_ctx *ctx = C.ctx;
    BamChunkSlot &s = C.at(k);
    HIPCHK(hipEventRecord(s.e0, C.s_io));
    if (n) HIPCHK(hipMemcpyAsync(s.d_buf + s.room, p, n, hipMemcpyHostToDevice, C.s_io));
    HIPCHK(hipMemsetAsync(s.d_buf + s.room + n, 0, 64, C.s_io));
    HIPCHK(hipEventRecord(s.e1, C.s_io));
    return TELR_OK;
}
static int reads_load(telr_ctx *ctx, const BamInHop &H, int container, int32_t keep_qual, int64_t chunk_bytes, telr_reads_in **out)
{
    BamInClock wall, clk;
    std::unique_ptr<telr_reads_in, void (*)(telr_reads_in*)> B(new telr_reads_in(), telr_reads_in_free);
    B->ctx = ctx;
    B->counters[0] = container; B->phase_ms[RIN_HOP] = H.ms;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RtLoad L(ctx, keep_qual != 0);
    for (hipEvent_t &e : L.ev) HIPCHK(hipEventCreate(&e));
    BamChunked C(ctx, H);
    C.what = "telr_reads_load";
    RtGzip Z;
    const uint8_t *fp = H.F.p; const size_t fn = H.F.n;
    size_t ppos = 0;                                   // plain: the next byte of the file
    size_t pay[2] = { 0, 0 }; bool lastf[2] = { false, false };
    const size_t chunk = (size_t)chunk_bytes;
    if (container == RIN_BGZF) TRY(bamc_setup(C, chunk_bytes, 2));
    else if (container == RIN_GZIP) {
        // (deflate does not expand beyond 1,032 times: a small file needs no buffer of a whole chunk)
        const size_t cap = (size_t)std::min<double>((double)chunk + RT_GATHER, (double)fn * 1032.0 + RT_GATHER);
        C.max_payload = cap;
        TRY(bamc_slots(C, 2, false));
        void *p;
        TRY(ctx_hbuf(ctx, "rin_pin0", cap + 64, &p)); Z.pin[0] = (uint8_t*)p;
        TRY(ctx_hbuf(ctx, "rin_pin1", cap + 64, &p)); Z.pin[1] = (uint8_t*)p;
        Z.src = fp; Z.n = fn; Z.chunk = std::min(chunk, cap);
        memset(&Z.z, 0, sizeof(Z.z));
        if (inflateInit2(&Z.z, 47) != Z_OK) { ctx->err = "telr_reads_load: gzip: zlib does not start"; return TELR_E_NOMEM; }
        Z.z_on = true;
        Z.th = std::thread([&Z] { Z.run(); });
    } else {
        C.max_payload = std::min<size_t>(chunk + RT_GATHER, std::max<size_t>(fn, 1));
        TRY(bamc_slots(C, 2, false));
    }
    // chunk k on its way to its slot; BGZF: inflated there
    auto issue = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        if (container == RIN_BGZF) { TRY(bamc_issue(C, k)); pay[i] = (size_t)C.payload(k); lastf[i] = k + 1 >= C.nch; return TELR_OK; }
        if (container == RIN_GZIP) {
            Z.get(k);
            if (Z.failed[i]) { ctx->err = "telr_reads_load: " + Z.err; return TELR_E_ARG; }
            pay[i] = Z.len[i]; lastf[i] = Z.last[i];
            return rt_issue_host(C, k, Z.pin[i], pay[i]);
        }
        const bool fq = fn && fp[0] == '@';
        size_t take = 0, marks = 0;
        do {
            const size_t c = std::min(chunk, fn - ppos - take);
            if (chunk < RT_GATHER) marks += rt_marks(fp + ppos + take, c, fq);
            take += c;
        } while (ppos + take < fn && marks < (fq ? 4u : 1u) && take < RT_GATHER);
        pay[i] = take; lastf[i] = ppos + take >= fn;
        TRY(rt_issue_host(C, k, fp + ppos, take));
        ppos += take;
        return TELR_OK;
    };
    auto wait = [&](int64_t k) -> int {
        if (container == RIN_BGZF) return bamc_wait(C, k);
        BamChunkSlot &s = C.at(k);
        HIPCHK(hipEventSynchronize(s.e1));
        float a = 0;
        HIPCHK(hipEventElapsedTime(&a, s.e0, s.e1)); C.ms_upload += a;
        if (container == RIN_GZIP) Z.give_back(k);
        return TELR_OK;
    };
    int64_t carry = 0, max_carry = 0, text = 0, nchunks = 0;
    if (container != RIN_BGZF || C.nch) {
        TRY(issue(0));
        for (int64_t k = 0; ; ++k) {
            TRY(wait(k));
            const int i = (int)(k & 1);
            const bool last = lastf[i];
            const int64_t payload = (int64_t)pay[i];
            bool ahead = false;
            if (!last && container != RIN_GZIP) { TRY(issue(k + 1)); ahead = true; }          // (gzip: its thread is ahead already; the upload follows the parse)
            BamChunkSlot &s = C.at(k);
            const int64_t buflen = carry + payload;
            const uint8_t *buf = s.d_buf + s.room - carry;
            max_carry = std::max(max_carry, carry); text += payload; ++nchunks;
            if (L.kind < 0 && buflen) {
                uint8_t c = 0;
                HIPCHK(hipMemcpy(&c, buf, 1, hipMemcpyDeviceToHost));
                if (c != '@' && c != '>') { ctx->err = "telr_reads_load: the text opens with neither '@' nor '>'"; return TELR_E_ARG; }
                L.kind = c == '@' ? 1 : 0;
            }
            int64_t cut = 0;
            TRY(rt_parse(L, buf, buflen, last, &cut));
            if (last) break;
            carry = buflen - cut;
            TRY(bamc_carry(C, k, buf + cut, carry, ahead ? pay[(k + 1) & 1] : 0));
            if (!ahead) TRY(issue(k + 1));
        }
    }
    B->phase_ms[RIN_UPLOAD] = C.ms_upload; B->phase_ms[RIN_INFLATE] = container == RIN_GZIP ? Z.ms : C.ms_inflate;
    B->phase_ms[RIN_LINES] = L.ms[0]; B->phase_ms[RIN_RECORDS] = L.ms[1]; B->phase_ms[RIN_NAMES] = L.ms[2]; B->phase_ms[RIN_PACK] = L.ms[3];
    // ---- the set: its arrays, the pieces end to end
    clk.lap();
    telr_seqset *S = new telr_seqset();
    S->ctx = ctx; S->n = (int32_t)L.lens.size(); S->len = L.lens;
    TRY(seqset_alloc(ctx, S, "telr_reads_load", true, st));          // (frees S on failure)
    std::unique_ptr<telr_seqset, void (*)(telr_seqset*)> Sg(S, telr_seqset_free);
    const bool with_qual = keep_qual && L.kind == 1;
    if (with_qual) {
        HIPCHK(hipMalloc(&S->d_qual, (size_t)S->padded_bases + 64));
        HIPCHK(hipMemsetAsync(S->d_qual + S->padded_bases, 0, 64, st));
    }
    int64_t g = 0;
    for (const RtPiece &P : L.pieces) {
        if (P.groups) {
            HIPCHK(hipMemcpyAsync(S->d_seq2 + g * 4, P.w2, (size_t)P.groups * 16, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(S->d_nmask + g * 2, P.wn, (size_t)P.groups * 8, hipMemcpyDeviceToDevice, st));
            if (with_qual) HIPCHK(hipMemcpyAsync(S->d_qual + g * 64, P.q, (size_t)P.groups * 64, hipMemcpyDeviceToDevice, st));
        }
        g += P.groups;
    }
    HIPCHK(hipStreamSynchronize(st));
    B->phase_ms[RIN_JOIN] = clk.lap();
    B->counters[1] = L.kind == 1 ? 1 : 0;
    B->counters[2] = container == RIN_BGZF ? (int64_t)H.mem.size() : container == RIN_GZIP ? Z.members : 0;
    B->counters[3] = text; B->counters[4] = L.lines; B->counters[5] = (int64_t)L.lens.size(); B->counters[6] = L.bases;
    B->counters[7] = container == RIN_BGZF ? H.no_eof : 0;
    B->chunk_info[0] = nchunks; B->chunk_info[1] = (int64_t)C.max_alloc; B->chunk_info[2] = max_carry;
    B->chunk_info[3] = (int64_t)L.slabs.total + 2 * (int64_t)C.max_alloc;
    B->qnames.swap(L.names);
    for (auto &n : B->qnames) B->qname_ptr.push_back(n.c_str());
    B->qname_ptr.push_back(nullptr);
    B->set = Sg.release();
    B->phase_ms[RIN_TOTAL] = wall.lap() + H.ms;
    *out = B.release();
    return TELR_OK;
}

extern "C" int telr_reads_load(telr_ctx *ctx, const char *path, int32_t keep_qual, int64_t chunk_bytes, telr_reads_in **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    if (!path || !out) { ctx->err = "telr_reads_load: null path or output"; return TELR_E_ARG; }
    if (chunk_bytes < 0) { ctx->err = "telr_reads_load: negative chunk_bytes"; return TELR_E_ARG; }
    BamInHop H;
    const int rc = bam_in_hop(ctx, "telr_reads_load", path, H);          // (it maps the file; what it says about the members counts for a BGZF file only)
    if (rc == TELR_E_IO) return rc;
    const uint8_t *p = H.F.p; const size_t n = H.F.n;
    int container = RIN_PLAIN;
    if (n >= 2 && p[0] == 0x1f && p[1] == 0x8b) container = rc == TELR_OK && n >= 3 && p[2] == 8 ? RIN_BGZF : RIN_GZIP;
    else if (n && p[0] != '@' && p[0] != '>') { ctx->err = "telr_reads_load: neither gzip nor BGZF, and the file opens with neither '@' nor '>'"; return TELR_E_ARG; }
    ctx->err.clear();
    TRY(bamc_auto_chunk(ctx, 0, &chunk_bytes));          // (0 is the only value it acts on here: there is no "fits" for a reads file)
    return reads_load(ctx, H, container, keep_qual, chunk_bytes, out);
}
extern "C" int32_t telr_reads_in_count(const telr_reads_in *in) { return in ? (int32_t)in->qnames.size() : 0; }
extern "C" const char *const *telr_reads_in_names(const telr_reads_in *in) { return in ? in->qname_ptr.data() : nullptr; }
extern "C" const int32_t *telr_reads_in_lens(const telr_reads_in *in) { return in && in->set ? in->set->len.data() : nullptr; }
extern "C" telr_seqset *telr_reads_in_seqset(const telr_reads_in *in) { return in ? in->set : nullptr; }
extern "C" telr_seqset *telr_reads_in_detach_seqset(telr_reads_in *in) { if (!in || !in->set_owned) return nullptr; in->set_owned = false; return in->set; }
extern "C" int telr_reads_in_counters(const telr_reads_in *in, int64_t *out) { if (!in || !out) return TELR_E_ARG; memcpy(out, in->counters, sizeof(in->counters)); return TELR_OK; }
extern "C" int telr_reads_in_chunk_info(const telr_reads_in *in, int64_t *out) { if (!in || !out) return TELR_E_ARG; memcpy(out, in->chunk_info, sizeof(in->chunk_info)); return TELR_OK; }
extern "C" int telr_reads_in_phase_ms(const telr_reads_in *in, float *out) { if (!in || !out) return TELR_E_ARG; memcpy(out, in->phase_ms, sizeof(in->phase_ms)); return TELR_OK; }
