// Insertion candidates from a mapped read set, on the device (include/telr_hip.h: telr_call_insertions).  Stands where
// the reference shells out to Sniffles (`detect_sv`, src/telr/TELR_sv.py:49-51) -- with an own, fully specified definition, NOT a
// restatement of Sniffles: signatures (an I run inside a record, a same-strand split between two records of a read, a clipped read
// end) are sorted by (target, position), single-linkage clustered, and a cluster with enough distinct reads is a call.
//
//   k_ins_cigar    one wave per eligible record, 64 CIGAR words per step (coalesced dwords), wave prefix sums of the reference and
//                  query lengths; run once to count the qualifying I runs of every record and, after a scan, once to write them: a
//                  signature's place is (records before) + (qualifying runs before it in its record), never an atomic's arrival order;
//   k_ins_query    one lane per eligible record: its clipped ends and the splits it starts (its read's other records are a short
//                  contiguous run of the list), counted and written the same way;
//   sorts          LSD over the complete key with radix.hip.h (stable; a permutation is carried, the keys of a round are gathered
//                  through it): (kind, len, mate), then rec, then (tid, pos);
//   clusters       head flags + scan; the distinct reads of a cluster from a sort by (cluster, read, unsized); its representative
//                  from a sort by (cluster, unsized, len, read, rec, mate); counts are differences of scanned flags at the cluster's
//                  bounds; calls and their read lists are compacted by two more scans.
// The entry is three parts: InsFront (refusals, eligible records, signatures, the sort), the clusters, ins_collect (distinct reads,
// representatives, calls).  telr_call_at_sites (sitecall.hip.h) shares the first and the last and puts the caller's sites in the middle.
#pragma once

struct InsRec {                 // an eligible record; qs / qe on the record's own strand
    int32_t qid, tid, ts, te, qs, qe, qlen, rev;
    int32_t n_cigar, rec, g0, g1;     // [g0, g1): the records of the same read in this list
    int64_t cigar_off;
};

struct telr_ins_calls {
    std::vector<telr_ins_call> calls;
    std::vector<telr_ins_sig> sigs;
    std::vector<int64_t> read_off;
    std::vector<int32_t> reads;
};

template <bool EMIT>
__global__ void __launch_bounds__(256) k_ins_cigar(const InsRec *__restrict__ recs, int32_t ne, const uint32_t *__restrict__ cig, int32_t min_len,
                                                   int32_t *__restrict__ cnt, const int64_t *__restrict__ off, telr_ins_sig *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (w >= ne) return;
    const InsRec R = recs[w];
    const uint32_t *__restrict__ c = cig + R.cigar_off;
    const int32_t n = R.n_cigar;
    int32_t rbase = 0, qbase = 0, nout = 0;
    const int64_t o0 = EMIT ? off[w] : 0;
    for (int32_t i0 = 0; i0 < n; i0 += 64) {
        const int32_t i = i0 + lane;
        const uint32_t word = i < n ? c[i] : 0u;
        const int32_t op = (int32_t)(word & 15u), len = (int32_t)(word >> 4);
        const bool hit = i < n && op == 1 && len >= min_len;
        const uint64_t m = __ballot(hit);
        if (EMIT) {
            const int32_t r = (op == 0 || op == 2) ? len : 0, q = (op == 0 || op == 1) ? len : 0;
            const int32_t ri = d_wave_incl<int32_t>(r, lane), qi = d_wave_incl<int32_t>(q, lane);
            if (hit) {
                const int32_t rank = __builtin_popcountll(m & ((1ULL << lane) - 1ULL));
                const int32_t qb = qbase + qi - q;          // query bases of the record before the run, on the record's strand
                telr_ins_sig s;
                s.tid = R.tid; s.pos = R.ts + rbase + ri - r; s.len = len; s.qid = R.qid; s.kind = 0; s.rec = R.rec; s.mate = -1;
                s.seg_start = R.rev ? R.qlen - (R.qs + qb + len) : R.qs + qb; s.seg_len = len;
                out[o0 + nout + rank] = s;
            }
            rbase += __shfl(ri, 63); qbase += __shfl(qi, 63);
        }
        nout += __builtin_popcountll(m);
    }
    if (!EMIT && lane == 0) cnt[w] = nout;
}

template <bool EMIT>
__global__ void __launch_bounds__(256) k_ins_query(const InsRec *__restrict__ recs, int32_t ne, int32_t min_len, int32_t min_clip, int32_t max_ref_gap,
                                                   int32_t *__restrict__ cnt, const int64_t *__restrict__ off, telr_ins_sig *__restrict__ out)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= ne) return;
    const InsRec A = recs[a];
    telr_ins_sig *o = EMIT ? out + off[a] : nullptr;
    int32_t n = 0;
    telr_ins_sig s;
    s.tid = A.tid; s.qid = A.qid; s.rec = A.rec; s.mate = -1; s.kind = 2;
    if (A.qs >= min_clip) {
        if (EMIT) { s.pos = A.ts; s.len = s.seg_len = A.qs; s.seg_start = A.rev ? A.qlen - A.qs : 0; o[n] = s; }
        ++n;
    }
    if (A.qlen - A.qe >= min_clip) {
        if (EMIT) { s.pos = A.te; s.len = s.seg_len = A.qlen - A.qe; s.seg_start = A.rev ? 0 : A.qe; o[n] = s; }
        ++n;
    }
    s.kind = 1;
    for (int32_t b = A.g0; b < A.g1; ++b) {
        if (b == a) continue;
        const InsRec B = recs[b];
        if (B.tid != A.tid || B.rev != A.rev) continue;
        const int64_t qgap = (int64_t)B.qs - A.qe, tgap = (int64_t)B.ts - A.te;
        if (qgap < 0 || tgap > max_ref_gap || -tgap > max_ref_gap || qgap - tgap < min_len) continue;
        if (EMIT) {
            s.pos = A.te; s.len = (int32_t)(qgap - tgap); s.mate = B.rec; s.seg_len = (int32_t)qgap;
            s.seg_start = A.rev ? A.qlen - B.qs : A.qe;
            o[n] = s;
        }
        ++n;
    }
    if (!EMIT) cnt[a] = n;
}

// the keys of the sort rounds (stage2_common.hip.h: perm_sort_round); rb / qb: the bits of a record number + 1 / of a read number
struct InsKeyKLM { int rb; __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t) const { return ((((uint64_t)s.kind << 31) | (uint32_t)s.len) << rb) | (uint32_t)(s.mate + 1); } };
struct InsKeyREC { __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t) const { return (uint32_t)s.rec; } };
struct InsKeyTP  { __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t) const { return ((uint64_t)(uint32_t)s.tid << 32) | (uint32_t)s.pos; } };
struct InsKeyRM  { int rb; __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t) const { return ((uint64_t)(uint32_t)s.rec << rb) | (uint32_t)(s.mate + 1); } };
struct InsKeyLQ  { int qb; __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t) const { return ((uint64_t)(uint32_t)s.len << qb) | (uint32_t)s.qid; } };
// with the cluster id of the signature (cid, by the signature's index); unsized (a clipped end) sorts behind sized
struct InsKeyCQU { const int32_t *cid; int qb; __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t p) const { return ((((uint64_t)(uint32_t)cid[p] << qb) | (uint32_t)s.qid) << 1) | (s.kind == 2 ? 1u : 0u); } };
struct InsKeyCU  { const int32_t *cid; __device__ uint64_t operator()(const telr_ins_sig &s, uint32_t p) const { return ((uint64_t)(uint32_t)cid[p] << 1) | (s.kind == 2 ? 1u : 0u); } };
// head[i] = signature i starts a cluster, sized[i] = it carries a length; both with a trailing 0 for the scans
__global__ void __launch_bounds__(256) k_ins_heads(const telr_ins_sig *__restrict__ sig, int64_t n, int32_t dist, int32_t *__restrict__ head, int32_t *__restrict__ sized)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { head[i] = 0; sized[i] = 0; return; }
    const telr_ins_sig s = sig[i];
    int32_t h = 1;
    if (i > 0) { const telr_ins_sig p = sig[i - 1]; h = (p.tid != s.tid || (int64_t)s.pos - p.pos > dist) ? 1 : 0; }
    head[i] = h; sized[i] = s.kind != 2 ? 1 : 0;
}
// hx = exclusive scan of head (hx[n] = clusters): cid[i] and the clusters' first signatures (cstart[clusters] = n)
__global__ void __launch_bounds__(256) k_ins_cid(const int32_t *__restrict__ head, const int32_t *__restrict__ hx, int64_t n, int32_t *__restrict__ cid, int32_t *__restrict__ cstart)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { cstart[hx[n]] = (int32_t)n; return; }
    cid[i] = hx[i + 1] - 1;
    if (head[i]) cstart[hx[i]] = (int32_t)i;
}
// over the order of the (cluster, read, unsized) sort: dflag = first signature of its read in its cluster, sdflag = ... and it is sized
// (the sized ones of a read sort first, so the first is sized iff any is)
__global__ void __launch_bounds__(256) k_ins_distinct(const telr_ins_sig *__restrict__ sig, const int32_t *__restrict__ cid, const uint32_t *__restrict__ perm, int64_t n,
                                                      int32_t *__restrict__ dflag, int32_t *__restrict__ sdflag)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    if (j == n) { dflag[j] = 0; sdflag[j] = 0; return; }
    const uint32_t p = perm[j];
    int32_t d = 1;
    if (j > 0) { const uint32_t q = perm[j - 1]; d = (cid[q] != cid[p] || sig[q].qid != sig[p].qid) ? 1 : 0; }
    dflag[j] = d; sdflag[j] = d && sig[p].kind != 2 ? 1 : 0;
}
// per cluster: distinct reads, distinct sized reads, is it a call; qcnt = the reads it will list
__global__ void __launch_bounds__(256) k_ins_cluster(const int32_t *__restrict__ cstart, int32_t nc, const int32_t *__restrict__ dx, const int32_t *__restrict__ sdx,
                                                     int32_t min_support, int32_t min_sized, int32_t *__restrict__ cflag, int32_t *__restrict__ qcnt)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > nc) return;
    if (c == nc) { cflag[c] = 0; qcnt[c] = 0; return; }
    const int32_t lo = cstart[c], hi = cstart[c + 1];
    const int32_t sup = dx[hi] - dx[lo], nsz = sdx[hi] - sdx[lo];
    const int32_t ok = sup >= min_support && nsz >= min_sized ? 1 : 0;
    cflag[c] = ok; qcnt[c] = ok ? sup : 0;
}
// AT_SITES (telr_call_at_sites): cluster c is the caller's site c, which gives tid and pos; its run of signatures may be empty
template <bool AT_SITES>
__global__ void __launch_bounds__(256) k_ins_calls(const telr_ins_sig *__restrict__ sig, const int32_t *__restrict__ cstart, int32_t nc, const int32_t *__restrict__ dx,
                                                   const int32_t *__restrict__ sdx, const int32_t *__restrict__ sx, const uint32_t *__restrict__ perm_rep,
                                                   const int32_t *__restrict__ cflag, const int32_t *__restrict__ cx, const int64_t *__restrict__ qx,
                                                   const telr_ins_site *__restrict__ sites, telr_ins_call *__restrict__ calls, int64_t *__restrict__ read_off)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > nc) return;
    if (c == nc) { read_off[cx[nc]] = qx[nc]; return; }
    if (!cflag[c]) return;
    const int32_t lo = cstart[c], hi = cstart[c + 1], ns = sx[hi] - sx[lo];
    telr_ins_call k;
    if (AT_SITES) { k.tid = sites[c].tid; k.pos = sites[c].pos; }
    else { k.tid = sig[lo].tid; k.pos = sig[lo + (hi - lo - 1) / 2].pos; }
    k.support = dx[hi] - dx[lo]; k.n_sized = sdx[hi] - sdx[lo];
    k.rep = ns > 0 ? (int32_t)perm_rep[lo + (ns - 1) / 2] : -1;          // the sized signatures of the cluster come first in the representative sort
    k.len = ns > 0 ? sig[k.rep].len : 0;
    calls[cx[c]] = k; read_off[cx[c]] = qx[c];
}
__global__ void __launch_bounds__(256) k_ins_reads(const telr_ins_sig *__restrict__ sig, const int32_t *__restrict__ cid, const uint32_t *__restrict__ perm, int64_t n,
                                                   const int32_t *__restrict__ dflag, const int32_t *__restrict__ dx, const int32_t *__restrict__ cstart,
                                                   const int32_t *__restrict__ cflag, const int64_t *__restrict__ qx, int32_t *__restrict__ reads)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !dflag[j]) return;
    const uint32_t p = perm[j];
    const int32_t c = cid[p];
    if (cflag[c]) reads[qx[c] + (dx[j] - dx[cstart[c]])] = sig[p].qid;
}

extern "C" void telr_ins_opt_default(telr_ins_opt *o)
{
    if (!o) return;
    o->min_len = 50; o->min_mapq = 20; o->min_clip = 200; o->max_ref_gap = 200; o->cluster_dist = 50; o->min_support = 10; o->min_sized = 1; o->reserved = 0;
}
extern "C" int64_t telr_ins_calls_count(const telr_ins_calls *c) { return c ? (int64_t)c->calls.size() : 0; }
extern "C" const telr_ins_call *telr_ins_calls_calls(const telr_ins_calls *c) { return c ? c->calls.data() : nullptr; }
extern "C" int64_t telr_ins_calls_sig_count(const telr_ins_calls *c) { return c ? (int64_t)c->sigs.size() : 0; }
extern "C" const telr_ins_sig *telr_ins_calls_sigs(const telr_ins_calls *c) { return c ? c->sigs.data() : nullptr; }
extern "C" const int64_t *telr_ins_calls_read_off(const telr_ins_calls *c) { return c ? c->read_off.data() : nullptr; }
extern "C" const int32_t *telr_ins_calls_reads(const telr_ins_calls *c) { return c ? c->reads.data() : nullptr; }
extern "C" void telr_ins_calls_free(telr_ins_calls *c) { delete c; }

// The front half of the two entries on a result's signatures (telr_call_insertions here, telr_call_at_sites in sitecall.hip.h), stated
// once: check() refuses on the host or lists the eligible records; signatures() counts, writes and sorts them on the device.
struct InsFront {
    telr_ctx *ctx; std::string who; const telr_result *r; telr_ins_opt O;
    std::vector<InsRec> er; size_t n = 0; int32_t n_targets = 0, max_qid = 0;      // check(): the eligible records, grouped by read
    int64_t N = 0; telr_ins_sig *d_sig = nullptr; int64_t *d_tot = nullptr;       // signatures(): N of them at d_sig in key order; d_tot: 4 words of scan totals
    PermSort S; int rb = 0, qb = 0;                                                // the sort's buffers (ins_*), the bits of a record number + 1 / of a read number

    int bad(const std::string &why) { ctx->err = who + ": " + why; return TELR_E_ARG; }
    // null arguments, n_targets, the options (clusters: also those that only the clustering of telr_call_insertions reads), the record
    // count, every record -- in this order
    int check(telr_ctx *ctx_, const char *who_, const telr_result *r_, bool have_out, int32_t n_targets_, const telr_ins_opt *opt, bool clusters)
    {
        ctx = ctx_; who = who_; r = r_; n_targets = n_targets_;
        if (!r || !have_out) return bad("null result or output");
        if (n_targets <= 0) return bad("n_targets must be positive");
        if (opt) O = *opt; else telr_ins_opt_default(&O);
        if (O.min_len < 0 || O.min_mapq < 0 || O.min_clip < 0 || O.max_ref_gap < 0) return bad("negative option");
        if (clusters) {
            if (O.cluster_dist < 0 || O.min_support < 0 || O.min_sized < 0) return bad("negative option");
            if (O.min_sized > O.min_support) return bad("min_sized > min_support");
        }
        n = r->alns.size();
        if (n >= 0x7ffffff0u) { ctx->err = who + ": too many records"; return TELR_E_RANGE; }
        // the eligible records, grouped by read (a mapped result is in read order already)
        bool in_order = true;
        std::string why;
        for (size_t i = 0; i < n; ++i) {
            const telr_aln &a = r->alns[i];
            if (!record_check(a, i, n_targets, r->ncig, &why)) return bad(why);
            if ((a.flags & TELR_F_SECONDARY) || a.mapq < O.min_mapq) continue;
            InsRec e;
            const StrandCoords s = strand_coords(a);
            e.qid = a.qid; e.tid = a.tid; e.ts = a.ts; e.te = a.te; e.qlen = a.qlen; e.rev = s.rev; e.qs = s.qs; e.qe = s.qe;
            e.n_cigar = a.n_cigar; e.rec = (int32_t)i; e.g0 = e.g1 = 0; e.cigar_off = a.cigar_off;
            if (!er.empty() && er.back().qid > e.qid) in_order = false;
            max_qid = std::max(max_qid, a.qid);
            er.push_back(e);
        }
        if (!in_order) std::stable_sort(er.begin(), er.end(), [](const InsRec &x, const InsRec &y) { return x.qid < y.qid; });
        const size_t ne = er.size();
        for (size_t i = 0; i < ne; ) {
            size_t j = i + 1;
            while (j < ne && er[j].qid == er[i].qid) ++j;
            for (size_t k = i; k < j; ++k) { er[k].g0 = (int32_t)i; er[k].g1 = (int32_t)j; }
            i = j;
        }
        return TELR_OK;
    }
    // at least one eligible record: N and, when N > 0, the sorted signatures.  The stream is idle at N == 0, busy with the sort otherwise.
    int signatures()
    {
        const size_t ne = er.size();
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        result_wait(r);
        uint32_t *d_cig;
        TRY(result_dev_cigars(ctx, r, "ins_cig", true, &d_cig, nullptr));
        InsRec *d_rec; int32_t *d_cnt0, *d_cnt1; int64_t *d_off0, *d_off1;
        TRY(ctx_buf_t(ctx, "ins_rec", ne, &d_rec));
        TRY(ctx_buf_t(ctx, "ins_cnt0", ne + 1, &d_cnt0));
        TRY(ctx_buf_t(ctx, "ins_cnt1", ne + 1, &d_cnt1));
        TRY(ctx_buf_t(ctx, "ins_off0", ne + 1, &d_off0));
        TRY(ctx_buf_t(ctx, "ins_off1", ne + 1, &d_off1));
        TRY(ctx_buf_t(ctx, "ins_tot", 4, &d_tot));
        HIPCHK(hipMemcpyAsync(d_rec, er.data(), ne * sizeof(InsRec), hipMemcpyHostToDevice, st));
        const dim3 gw((unsigned)((ne + 3) / 4)), gl = grid256((int64_t)ne);
        hipLaunchKernelGGL((k_ins_cigar<false>), gw, dim3(256), 0, st, d_rec, (int32_t)ne, d_cig, O.min_len, d_cnt0, (const int64_t*)nullptr, (telr_ins_sig*)nullptr);
        hipLaunchKernelGGL((k_ins_query<false>), gl, dim3(256), 0, st, d_rec, (int32_t)ne, O.min_len, O.min_clip, O.max_ref_gap, d_cnt1, (const int64_t*)nullptr, (telr_ins_sig*)nullptr);
        HIPCHK(hipGetLastError());
        TRY((dev_qscan<int32_t, int64_t>(ctx, d_cnt0, (int32_t)ne, d_off0, d_tot, 0, nullptr, nullptr)));
        TRY((dev_qscan<int32_t, int64_t>(ctx, d_cnt1, (int32_t)ne, d_off1, d_tot + 1, 0, nullptr, nullptr)));
        int64_t tot[2];
        HIPCHK(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        N = tot[0] + tot[1];
        if (N == 0) return TELR_OK;
        if (N >= 0x7ffffff0LL) { ctx->err = who + ": too many signatures"; return TELR_E_RANGE; }
        telr_ins_sig *d_raw;
        TRY(ctx_buf_t(ctx, "ins_raw", (size_t)N, &d_raw));
        TRY(ctx_buf_t(ctx, "ins_sig", (size_t)N, &d_sig));
        hipLaunchKernelGGL((k_ins_cigar<true>), gw, dim3(256), 0, st, d_rec, (int32_t)ne, d_cig, O.min_len, d_cnt0, d_off0, d_raw);
        hipLaunchKernelGGL((k_ins_query<true>), gl, dim3(256), 0, st, d_rec, (int32_t)ne, O.min_len, O.min_clip, O.max_ref_gap, d_cnt1, d_off1, d_raw + tot[0]);
        HIPCHK(hipGetLastError());
        // sort by (tid, pos, rec, kind, len, mate): least significant group first
        TRY(S.alloc(ctx, "ins_", (size_t)N));
        rb = bits_of((uint64_t)n); qb = bits_of((uint64_t)max_qid);
        const int tb = bits_of((uint64_t)n_targets - 1);
        perm_iota(ctx, S, N);
        TRY(perm_sort_round(ctx, S, d_raw, N, InsKeyKLM{rb}, 33 + rb));
        TRY(perm_sort_round(ctx, S, d_raw, N, InsKeyREC{}, rb));
        TRY(perm_sort_round(ctx, S, d_raw, N, InsKeyTP{}, 32 + tb));
        perm_gather(ctx, S, d_raw, N, d_sig);
        return TELR_OK;
    }
};

// The back half of both: N > 0 signatures at d_sig in key order, in nc > 0 clusters -- cid[i] the cluster of signature i (non-decreasing),
// cstart[c] its first signature (cstart[nc] = N; a run may be empty), sx the exclusive scan of the sized flags.  The distinct reads and
// the representative of every cluster, then the calls: those of the clusters with enough support, or with d_sites (the caller's sites,
// one per cluster) one per cluster.  Signatures, calls and read lists are copied into C; the stream is idle on return.
static int ins_collect(InsFront &F, const telr_ins_sig *d_sig, int64_t N, const int32_t *d_cid, const int32_t *d_cstart, int32_t nc, const int32_t *d_sx,
                       int32_t min_support, int32_t min_sized, const telr_ins_site *d_sites, telr_ins_calls *C)
{
    telr_ctx *ctx = F.ctx;
    hipStream_t st = ctx->stream;
    PermSort &S = F.S;
    const int rb = F.rb, qb = F.qb, cb = bits_of((uint64_t)nc - 1);
    const dim3 gN = grid256(N), gN1 = grid256(N + 1);
    int32_t *d_dflag, *d_sdflag, *d_dx, *d_sdx;
    TRY(ctx_buf_t(ctx, "ins_dflag", (size_t)N + 1, &d_dflag));
    TRY(ctx_buf_t(ctx, "ins_sdflag", (size_t)N + 1, &d_sdflag));
    TRY(ctx_buf_t(ctx, "ins_dx", (size_t)N + 1, &d_dx));
    TRY(ctx_buf_t(ctx, "ins_sdx", (size_t)N + 1, &d_sdx));
    // the distinct reads of every cluster
    perm_iota(ctx, S, N);
    TRY(perm_sort_round(ctx, S, d_sig, N, InsKeyCQU{d_cid, qb}, cb + qb + 1));
    uint32_t *d_permd;
    TRY(ctx_buf_t(ctx, "ins_permd", (size_t)N, &d_permd));
    HIPCHK(hipMemcpyAsync(d_permd, S.perm, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_ins_distinct, gN1, dim3(256), 0, st, d_sig, d_cid, d_permd, N, d_dflag, d_sdflag);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_dflag, (int32_t)N, d_dx, nullptr, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_sdflag, (int32_t)N, d_sdx, nullptr, 0, nullptr, nullptr)));
    // the representative: (cluster, unsized, len, read, rec, mate)
    perm_iota(ctx, S, N);
    TRY(perm_sort_round(ctx, S, d_sig, N, InsKeyRM{rb}, 2 * rb));
    TRY(perm_sort_round(ctx, S, d_sig, N, InsKeyLQ{qb}, 31 + qb));
    TRY(perm_sort_round(ctx, S, d_sig, N, InsKeyCU{d_cid}, cb + 1));
    // calls
    int32_t *d_cflag, *d_qcnt, *d_cx; int64_t *d_qx, *d_tot = F.d_tot;
    TRY(ctx_buf_t(ctx, "ins_cflag", (size_t)nc + 1, &d_cflag));
    TRY(ctx_buf_t(ctx, "ins_qcnt", (size_t)nc + 1, &d_qcnt));
    TRY(ctx_buf_t(ctx, "ins_cx", (size_t)nc + 1, &d_cx));
    TRY(ctx_buf_t(ctx, "ins_qx", (size_t)nc + 1, &d_qx));
    const dim3 gC1 = grid256((int64_t)nc + 1);
    hipLaunchKernelGGL(k_ins_cluster, gC1, dim3(256), 0, st, d_cstart, nc, d_dx, d_sdx, min_support, min_sized, d_cflag, d_qcnt);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_cflag, nc, d_cx, d_tot, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_qcnt, nc, d_qx, d_tot + 1, 0, nullptr, nullptr)));
    int64_t tot[2];
    HIPCHK(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t ncall = tot[0], nread = tot[1];
    telr_ins_call *d_calls; int64_t *d_roff; int32_t *d_reads;
    TRY(ctx_buf_t(ctx, "ins_calls", (size_t)ncall, &d_calls));
    TRY(ctx_buf_t(ctx, "ins_roff", (size_t)ncall + 1, &d_roff));
    TRY(ctx_buf_t(ctx, "ins_reads", (size_t)nread, &d_reads));
    if (d_sites) hipLaunchKernelGGL((k_ins_calls<true>), gC1, dim3(256), 0, st, d_sig, d_cstart, nc, d_dx, d_sdx, d_sx, S.perm, d_cflag, d_cx, d_qx, d_sites, d_calls, d_roff);
    else hipLaunchKernelGGL((k_ins_calls<false>), gC1, dim3(256), 0, st, d_sig, d_cstart, nc, d_dx, d_sdx, d_sx, S.perm, d_cflag, d_cx, d_qx, d_sites, d_calls, d_roff);
    hipLaunchKernelGGL(k_ins_reads, gN, dim3(256), 0, st, d_sig, d_cid, d_permd, N, d_dflag, d_dx, d_cstart, d_cflag, d_qx, d_reads);
    HIPCHK(hipGetLastError());
    C->sigs.resize((size_t)N); C->calls.resize((size_t)ncall); C->read_off.resize((size_t)ncall + 1); C->reads.resize((size_t)nread);
    HIPCHK(hipMemcpyAsync(C->sigs.data(), d_sig, (size_t)N * sizeof(telr_ins_sig), hipMemcpyDeviceToHost, st));
    if (ncall) HIPCHK(hipMemcpyAsync(C->calls.data(), d_calls, (size_t)ncall * sizeof(telr_ins_call), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C->read_off.data(), d_roff, ((size_t)ncall + 1) * 8, hipMemcpyDeviceToHost, st));
    if (nread) HIPCHK(hipMemcpyAsync(C->reads.data(), d_reads, (size_t)nread * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return TELR_OK;
}

extern "C" int telr_call_insertions(telr_ctx *ctx, const telr_result *r, int32_t n_targets, const telr_ins_opt *opt, telr_ins_calls **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    InsFront F;
    TRY(F.check(ctx, "telr_call_insertions", r, out != nullptr, n_targets, opt, true));
    telr_ins_calls *C = new telr_ins_calls();
    C->read_off.assign(1, 0);
    std::unique_ptr<telr_ins_calls> guard(C);
    if (F.er.empty()) { *out = guard.release(); return TELR_OK; }
    TRY(F.signatures());
    const int64_t N = F.N;
    if (N == 0) { *out = guard.release(); return TELR_OK; }
    hipStream_t st = ctx->stream;
    // clusters
    int32_t *d_head, *d_hx, *d_sized, *d_sx, *d_cid, *d_cstart;
    TRY(ctx_buf_t(ctx, "ins_head", (size_t)N + 1, &d_head));
    TRY(ctx_buf_t(ctx, "ins_hx", (size_t)N + 1, &d_hx));
    TRY(ctx_buf_t(ctx, "ins_sized", (size_t)N + 1, &d_sized));
    TRY(ctx_buf_t(ctx, "ins_sx", (size_t)N + 1, &d_sx));
    TRY(ctx_buf_t(ctx, "ins_cid", (size_t)N + 1, &d_cid));
    TRY(ctx_buf_t(ctx, "ins_cstart", (size_t)N + 1, &d_cstart));
    const dim3 gN1 = grid256(N + 1);
    hipLaunchKernelGGL(k_ins_heads, gN1, dim3(256), 0, st, F.d_sig, N, F.O.cluster_dist, d_head, d_sized);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_head, (int32_t)N, d_hx, nullptr, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_sized, (int32_t)N, d_sx, nullptr, 0, nullptr, nullptr)));
    hipLaunchKernelGGL(k_ins_cid, gN1, dim3(256), 0, st, d_head, d_hx, N, d_cid, d_cstart);
    int32_t nc = 0;
    HIPCHK(hipMemcpyAsync(&nc, d_hx + N, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    TRY(ins_collect(F, F.d_sig, N, d_cid, d_cstart, nc, d_sx, F.O.min_support, F.O.min_sized, nullptr, C));
    *out = guard.release();
    return TELR_OK;
}

