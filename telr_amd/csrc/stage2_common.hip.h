// What the stages on top of a mapped telr_result share: the CIGAR array on the device, the launch and bit-count
// helpers, the wave and search inlines of the span / pair kernels, the funnel shifts of the piece cutters, what the drafter and the bridge
// share (the one-coordinate CIGAR walk, the reach clamp, the signature window, the span kernel, their input: CutInput), and the stable permutation sort over radix.hip.h.  Included by telr_engine.hip once telr_result is
// defined (telr_depth_medians is a caller), so before every feature header (inscall, genotype, draft, bridge, refte, bam_in, seq_extract,
// part_merge, pileup, bam_dev): none of them takes a name from a sibling, but for sitecall, the second entry on inscall's signatures.  The host-side record and call-list checks of the call stages are record_checks.h.
#pragma once
#include "record_checks.h"

// ---- the result's CIGAR words on the device ---------------------------------------------------------------------------------------
// The device copy a result kept (TELR_MF_KEEP_CIGARS, telr_result_from_device_cigars, telr_merge_parts) is complete iff this holds.
static inline bool result_cigars_resident(const telr_result *r) { return r->d_cig && !r->twin_off && r->twin_n == r->ncig; }

// *d_cig = the result's own device copy when it is complete and the caller allows it, else the host array uploaded on the context's
// stream into the context buffer `tag` of ncig + slack words.  Call it after result_wait(r).  *resident (nullable) says which.
static int result_dev_cigars(telr_ctx *ctx, const telr_result *r, const char *tag, bool allow_resident, uint32_t **d_cig, bool *resident, size_t slack = 0)
{
    const bool res = allow_resident && result_cigars_resident(r);
    if (resident) *resident = res;
    // the last pieces of a mapped result's device copy were made on other streams than the caller's: a device-wide wait, not a stream's
    if (res) { *d_cig = r->d_cig; HIPCHK(hipDeviceSynchronize()); return TELR_OK; }
    TRY(ctx_buf_t(ctx, tag, r->ncig + slack, d_cig));
    if (r->ncig) HIPCHK(hipMemcpyAsync(*d_cig, r->cig, r->ncig * 4, hipMemcpyHostToDevice, ctx->stream));
    return TELR_OK;
}

// ---- small helpers ----------------------------------------------------------------------------------------------------------------
static inline dim3 grid256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }      // one lane per element, 256 per workgroup
static inline int bits_of(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// inclusive prefix sum over the wave
template <typename T>
static __device__ __forceinline__ T d_wave_incl(T v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T x = __shfl_up(v, o); if (lane >= o) v += x; }
    return v;
}

// first i in [0, n) with k[i] >= v (UPPER: > v)
template <bool UPPER>
static __device__ __forceinline__ int64_t d_bound(const uint64_t *__restrict__ k, int64_t n, uint64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t x = k[mid];
        if (UPPER ? x <= v : x < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the calls with (tid, pos) keys in [(tid, lo), (tid, hi)], 0 <= lo and hi < 2^32: a contiguous run of the ascending keys
static __device__ __forceinline__ void d_span(const uint64_t *__restrict__ ckeys, int32_t ncall, int32_t tid, int64_t lo, int64_t hi, int32_t *first, int32_t *cnt)
{
    const uint64_t t = (uint64_t)(uint32_t)tid << 32;
    const int64_t b0 = d_bound<false>(ckeys, ncall, t | (uint64_t)lo), b1 = d_bound<true>(ckeys, ncall, t | (uint64_t)hi);
    *first = (int32_t)b0; *cnt = b1 > b0 ? (int32_t)(b1 - b0) : 0;
}
// off = exclusive scan of n counts (off[n] = the pairs): pair p belongs to the last element with off <= p
static __device__ __forceinline__ int32_t d_pair_owner(const int64_t *__restrict__ off, int32_t n, int64_t p)
{
    int32_t lo = 0, hi = n;                               // first element with off > p
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= p) lo = mid + 1; else hi = mid; }
    return lo - 1;
}
// is q among the ascending reads[lo .. hi)
static __device__ __forceinline__ bool d_in_list(const int32_t *__restrict__ reads, int64_t lo, int64_t hi, int32_t q)
{
    const int64_t end = hi;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (reads[mid] < q) lo = mid + 1; else hi = mid; }
    return lo < end && reads[lo] == q;
}

// ---- 2-bit packed bases: the funnel shifts of the piece cutters (k_draft_extract, k_seq_extract, k_seq_join, k_bridge_vote) ---------
// 16 bases from base offset S of a packed array (S >= -15: what lies before the array reads as zero)
static __device__ __forceinline__ uint32_t d_window2(const uint32_t *__restrict__ p, int64_t S)
{
    const int64_t sw = S >> 4;
    const int sh = (int)(S & 15) * 2;
    const uint32_t a = sw >= 0 ? p[sw] : 0u;
    if (sh == 0) return a;
    return (uint32_t)((((uint64_t)p[sw + 1] << 32) | a) >> sh);
}
static __device__ __forceinline__ uint32_t d_window1(const uint32_t *__restrict__ p, int64_t S)
{
    const int64_t sw = S >> 5;
    const int sh = (int)(S & 31);
    const uint32_t a = sw >= 0 ? p[sw] : 0u;
    if (sh <= 16) return (a >> sh) & 0xffffu;
    return (uint32_t)((((uint64_t)p[sw + 1] << 32) | a) >> sh) & 0xffffu;
}
static __device__ __forceinline__ uint32_t d_rev16x2(uint32_t x)      // the sixteen 2-bit codes of a word in reverse order
{
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(x);
}

static __device__ __forceinline__ uint32_t d_spread16(uint32_t v)     // bit i -> bit 2i
{
    v = (v | v << 8) & 0x00FF00FFu; v = (v | v << 4) & 0x0F0F0F0Fu; v = (v | v << 2) & 0x33333333u; v = (v | v << 1) & 0x55555555u;
    return v;
}
// 16 bases and their 16 mask bits from strand coordinate t (0 <= t < qlen) of the read of qlen bases at base offset src of a set: the read
// itself, or with rc its reverse complement (read from the other end, base-reversed and complemented), so both strands cost the same.
// What lies behind the read's last base is undefined: the caller masks it.
static __device__ __forceinline__ void d_strand16(const uint32_t *__restrict__ p2, const uint32_t *__restrict__ pn, int64_t src, int32_t qlen, int rc, int64_t t,
                                                  uint32_t &code, uint32_t &m16)
{
    const int64_t S = rc ? src + qlen - 16 - t : src + t;      // >= -15
    code = d_window2(p2, S); m16 = d_window1(pn, S);
    if (rc) { code = ~d_rev16x2(code); m16 = __brev(m16) >> 16; }
}

// ---- what the stages that cut reads at reference coordinates share (draft.hip.h, bridge.hip.h) ----------------------------------------
struct DraftPiece { int64_t src; int32_t len, rc; };                                  // src: first base of the piece in the parent set's base layout

// the positions within `reach` of pos: [max(pos - reach, 0), min(pos + reach, 2^31 - 1)]
static __device__ __forceinline__ void d_reach(int32_t pos, int32_t reach, int64_t *lo, int64_t *hi)
{
    *lo = pos > reach ? (int64_t)pos - reach : 0;
    *hi = (int64_t)pos + reach < 0x7fffffffLL ? (int64_t)pos + reach : 0x7fffffffLL;
}

// One wave walks the n CIGAR words at c from the state (ts, qs): lo = the smallest strand coordinate among the states at reference
// coordinate xlo (the first op that holds xlo within [p, p + its reference length]), hi = the largest among those at xhi (the last
// such op; an I at xhi is inside).  Every lane returns the same values.
template <bool WANT_LO, bool WANT_HI>
static __device__ __forceinline__ void draft_walk(const uint32_t *__restrict__ c, int32_t n, int64_t ts, int64_t qs, int64_t xlo, int64_t xhi, int lane,
                                                  int64_t &lo, bool &flo, int64_t &hi, bool &fhi)
{
    const int64_t xend = WANT_HI ? xhi : xlo;
    int64_t rbase = ts, qbase = qs;                       // the state before the step's first op (the same in every lane)
    uint32_t next = lane < n ? c[lane] : 0u;
    for (int32_t i0 = 0; i0 < n && rbase <= xend; i0 += 64) {
        const int32_t i = i0 + lane;
        const uint32_t word = next;
        next = i < n - 64 ? c[i + 64] : 0u;               // the next step's words are on their way while this step's are summed
        const int32_t op = (int32_t)(word & 15u);
        const int64_t len = (int64_t)(word >> 4), r = (op == 0 || op == 2) ? len : 0, q = (op == 0 || op == 1) ? len : 0;
        const int64_t ri = d_wave_incl<int64_t>(r, lane), qi = d_wave_incl<int64_t>(q, lane), p = rbase + ri - r, u = qbase + qi - q;
        if (WANT_LO && !flo) {
            const uint64_t m = __ballot(i < n && p <= xlo && xlo <= p + r);
            if (m) { lo = __shfl(u + (op == 0 ? xlo - p : 0), __builtin_ctzll(m)); flo = true; }
        }
        if (WANT_HI) {
            const uint64_t m = __ballot(i < n && p <= xhi && xhi <= p + r);
            if (m) { hi = __shfl(u + (op == 0 ? xhi - p : op == 1 ? len : 0), 63 - __builtin_clzll(m)); fhi = true; }
        }
        if (WANT_LO && !WANT_HI && flo) break;
        rbase += __shfl(ri, 63); qbase += __shfl(qi, 63);
    }
}

// first i in [0, n) with (tid, pos) of signature i >= v (UPPER: > v); the signatures ascend by (tid, pos)
template <bool UPPER>
static __device__ __forceinline__ int32_t draft_sig_bound(const telr_ins_sig *__restrict__ sigs, int32_t n, uint64_t v)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t x = ((uint64_t)(uint32_t)sigs[mid].tid << 32) | (uint32_t)sigs[mid].pos;
        if (UPPER ? x <= v : x < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the signatures [s0, s1) within `reach` of call c: a contiguous run of the sorted array
static __device__ __forceinline__ void d_sig_window(const telr_ins_sig *__restrict__ sigs, int32_t ns, const telr_ins_call &c, int32_t reach, int32_t *s0, int32_t *s1)
{
    int64_t lo, hi;
    d_reach(c.pos, reach, &lo, &hi);
    const uint64_t t = (uint64_t)(uint32_t)c.tid << 32;
    *s0 = draft_sig_bound<false>(sigs, ns, t | (uint64_t)lo); *s1 = draft_sig_bound<true>(sigs, ns, t | (uint64_t)hi);
}

// One lane per signature: one whose kind is a bit of `kinds` (bit k = kind k) takes a lower and an upper bound in the calls' (tid, pos)
// keys -- the calls within `reach` of it are a contiguous run of the ascending keys: cnt of them from first (nullable) on; others 0.
__global__ void __launch_bounds__(256) k_cut_span(const telr_ins_sig *__restrict__ sigs, int32_t ns, const uint64_t *__restrict__ ckeys, int32_t ncall, int32_t reach,
                                                  uint32_t kinds, int32_t *__restrict__ first, int32_t *__restrict__ cnt)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ns) return;
    const telr_ins_sig s = sigs[j];
    int32_t f = 0, c = 0;
    if ((uint32_t)s.kind < 32u && ((kinds >> s.kind) & 1u)) {
        int64_t lo, hi;
        d_reach(s.pos, reach, &lo, &hi);
        d_span(ckeys, ncall, s.tid, lo, hi, &f, &c);
    }
    if (first) first[j] = f;
    cnt[j] = c;
}

// The input of telr_draft_contigs and telr_bridge_contigs -- a result, a call list, its signature array, the read set -- refused or
// brought to the device, in one set of context buffers (cut_*): a context that drafts and then bridges holds it once.  Every entry
// synchronises its stream before it returns, so the next call may overwrite them.
struct CutInput {
    telr_ctx *ctx; const char *who; const telr_result *r; const telr_ins_call *calls; const int64_t *read_off; const int32_t *reads; const telr_ins_sig *sigs;
    std::vector<uint64_t> ckeys; std::vector<CutRec> recs; int32_t nc = 0, ns = 0;      // check(): the calls' keys, a record per record of the result, the counts
    int64_t P = 0;                                                                // span(): the (signature, call) pairs; off = the scan of cnt
    telr_ins_sig *d_sig = nullptr; telr_ins_call *d_calls = nullptr; int32_t *d_first = nullptr, *d_cnt = nullptr; int64_t *d_off = nullptr;
    uint32_t *d_cig = nullptr; CutRec *d_rec = nullptr; int64_t *d_roff = nullptr; int32_t *d_reads = nullptr;      // prepare_pairs()

    // The host part, in the order a caller can observe: null arguments, the stage's own options (opt_fault: what the entry found wrong
    // with them, or null), the count limits, the calls, the records, the signatures (record_checks.h).  `who` opens every message.
    int check(telr_ctx *ctx_, const char *who_, const telr_result *r_, bool have_out, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls_,
              const int64_t *read_off_, const int32_t *reads_, int64_t n_sig, const telr_ins_sig *sigs_, const telr_seqset *read_set, const char *opt_fault)
    {
        ctx = ctx_; who = who_; r = r_; calls = calls_; read_off = read_off_; reads = reads_; sigs = sigs_;
        auto bad = [&](const std::string &why) { ctx->err = std::string(who) + ": " + why; return TELR_E_ARG; };
        auto many = [&](const char *what) { ctx->err = std::string(who) + ": too many " + what; return TELR_E_RANGE; };
        if (!r || !have_out || !read_set) return bad("null result, read set or output");
        if (n_targets <= 0) return bad("n_targets must be positive");
        if (n_calls < 0 || (n_calls > 0 && (!calls || !read_off))) return bad("null calls or read offsets");
        if (n_sig < 0 || (n_sig > 0 && !sigs)) return bad("null signatures");
        if (opt_fault) return bad(opt_fault);
        const size_t n = r->alns.size();
        if (n >= 0x7ffffff0u) return many("records");
        if (n_calls >= 0x7ffffff0LL) return many("calls");
        if (n_sig >= 0x7ffffff0LL) return many("signatures");
        std::string why;
        ckeys.resize((size_t)n_calls);
        if (!call_list_check(n_calls, calls, read_off, reads, n_targets, read_set->n, ckeys.data(), nullptr, &why)) return bad(why);
        recs.resize(n);
        for (size_t i = 0; i < n; ++i)
            if (!cut_rec_check(r->alns[i], i, n_targets, r->ncig, read_set->n, read_set->len.data(), &recs[i], &why)) return bad(why);
        if (!sig_list_check(n_sig, sigs, r->alns.data(), n, n_targets, read_set->n, &why)) return bad(why);
        nc = (int32_t)n_calls; ns = (int32_t)n_sig;
        return TELR_OK;
    }
    // signatures, calls and keys uploaded, k_cut_span (first is kept when want_first), the 64-bit scan, P and its limit; no calls or no
    // signatures: no pairs, and nothing is touched
    int span(int32_t reach, uint32_t kinds, bool want_first)
    {
        if (nc <= 0 || ns <= 0) return TELR_OK;
        hipStream_t st = ctx->stream;
        result_wait(r);
        uint64_t *d_ckeys; int64_t *d_tot;
        TRY(ctx_buf_t(ctx, "cut_sig", (size_t)ns, &d_sig));
        TRY(ctx_buf_t(ctx, "cut_calls", (size_t)nc, &d_calls));
        TRY(ctx_buf_t(ctx, "cut_ckeys", (size_t)nc, &d_ckeys));
        if (want_first) TRY(ctx_buf_t(ctx, "cut_first", (size_t)ns, &d_first));
        TRY(ctx_buf_t(ctx, "cut_cnt", (size_t)ns + 1, &d_cnt));
        TRY(ctx_buf_t(ctx, "cut_off", (size_t)ns + 1, &d_off));
        TRY(ctx_buf_t(ctx, "cut_tot", 4, &d_tot));
        HIPCHK(hipMemcpyAsync(d_sig, sigs, (size_t)ns * sizeof(telr_ins_sig), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_calls, calls, (size_t)nc * sizeof(telr_ins_call), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ckeys, ckeys.data(), (size_t)nc * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cut_span, grid256((int64_t)ns), dim3(256), 0, st, d_sig, ns, d_ckeys, nc, reach, kinds, d_first, d_cnt);
        HIPCHK(hipGetLastError());
        TRY((dev_qscan<int32_t, int64_t>(ctx, d_cnt, ns, d_off, d_tot, 0, nullptr, nullptr)));
        HIPCHK(hipMemcpyAsync(&P, d_tot, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (P >= 0x7ffffff0LL) { ctx->err = std::string(who) + ": too many (signature, call) pairs"; return TELR_E_RANGE; }
        return TELR_OK;
    }
    // P > 0: the CIGAR words (the result's own copy or an upload), the records, read_off and reads on the device; not waited for
    int prepare_pairs()
    {
        hipStream_t st = ctx->stream;
        TRY(result_dev_cigars(ctx, r, "cut_cig", true, &d_cig, nullptr));
        const int64_t nreads = read_off[nc];
        TRY(ctx_buf_t(ctx, "cut_rec", recs.size(), &d_rec));
        TRY(ctx_buf_t(ctx, "cut_roff", (size_t)nc + 1, &d_roff));
        TRY(ctx_buf_t(ctx, "cut_reads", (size_t)nreads, &d_reads));
        HIPCHK(hipMemcpyAsync(d_rec, recs.data(), recs.size() * sizeof(CutRec), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_roff, read_off, ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
        if (nreads) HIPCHK(hipMemcpyAsync(d_reads, reads, (size_t)nreads * 4, hipMemcpyHostToDevice, st));
        return TELR_OK;
    }
};

// ---- stable permutation sort --------------------------------------------------------------------------------------------------------
// LSD over a composite key, least significant group first: a permutation is carried from round to round, the keys of a round are
// gathered through it.  A key is a functor of the feature's own: uint64_t operator()(const T &element, uint32_t its_index).
struct PermSort {
    uint64_t *keys, *tkeys; uint32_t *perm, *tperm, *hist;
    // the buffers <prefix>keys, tkeys, perm, tperm, hist of the context, for up to n elements
    int alloc(telr_ctx *ctx, const std::string &prefix, size_t n)
    {
        TRY(ctx_buf_t(ctx, (prefix + "keys").c_str(), n, &keys));
        TRY(ctx_buf_t(ctx, (prefix + "tkeys").c_str(), n, &tkeys));
        TRY(ctx_buf_t(ctx, (prefix + "perm").c_str(), n, &perm));
        TRY(ctx_buf_t(ctx, (prefix + "tperm").c_str(), n, &tperm));
        return ctx_buf_t(ctx, (prefix + "hist").c_str(), rs_hist_words(n), &hist);
    }
};
__global__ void __launch_bounds__(256) k_perm_iota(uint32_t *__restrict__ perm, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}
template <typename T, typename KEY>
__global__ void __launch_bounds__(256) k_perm_key(const T *__restrict__ v, const uint32_t *__restrict__ perm, int64_t n, KEY key, uint64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = perm[i];
    keys[i] = key(v[p], p);
}
template <typename T>
__global__ void __launch_bounds__(256) k_perm_gather(const T *__restrict__ in, const uint32_t *__restrict__ perm, int64_t n, T *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}
static inline void perm_iota(telr_ctx *ctx, PermSort &S, int64_t n) { hipLaunchKernelGGL(k_perm_iota, grid256(n), dim3(256), 0, ctx->stream, S.perm, n); }
template <typename T>
static inline void perm_gather(telr_ctx *ctx, const PermSort &S, const T *in, int64_t n, T *out)
{
    hipLaunchKernelGGL((k_perm_gather<T>), grid256(n), dim3(256), 0, ctx->stream, in, S.perm, n, out);
}
// one stable round: sorts the permutation by `nbits` bits of the elements' keys
template <typename T, typename KEY>
static int perm_sort_round(telr_ctx *ctx, PermSort &S, const T *v, int64_t n, KEY key, int nbits)
{
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL((k_perm_key<T, KEY>), grid256(n), dim3(256), 0, st, v, S.perm, n, key, S.keys);
    if (radix_sort_passes<uint64_t, true>(S.keys, S.perm, S.tkeys, S.tperm, n, nbits, S.hist, st)) { std::swap(S.keys, S.tkeys); std::swap(S.perm, S.tperm); }
    HIPCHK(hipGetLastError());
    return TELR_OK;
}
