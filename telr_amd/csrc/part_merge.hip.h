// part_merge.hip.h — the merge of a multi-part index (include/telr_hip.h has the definition, tests/part_merge_ref.py
// states it in plain Python integers).  The reads were mapped against every part of a target set that is too large for one index
// (part_plan.h); here the final selection -- the oracle's select_chains pass 2, flags and MAPQ -- runs again over every read's pooled
// records, and the kept records' CIGAR words are gathered from the parts' resident arrays into ONE resident array, which the BAM writer
// and the insertion caller then read in place.  No CIGAR word comes to the host but through the result's one mirror copy.
//
//   host    part_merge_check on every record (part_plan.h); the pool in (query, part, rank) order as 32-byte keys + 16-byte sources
//   device  k_pm_select   one wave per query: order by counting, parent scan with ballots, subsc / n_sub, the kept secondaries
//           dev_qscan     kept records per query -> where each query's kept records start
//           k_pm_place    the kept records in output order, their CIGAR lengths
//           dev_qscan     CIGAR lengths -> dense offsets
//           k_pm_gather   one wave per kept record: its words from the part's array to the merged one
//   host    the records from the kernel's output and the parts' host records; mapq_of (never a device logf)
//
// Every store goes to the lane's own index, to the record's place in the order (a permutation found by counting) or to a position a
// scan gave; there is no atomic, so the bytes are the same on every run.
#pragma once
#include "part_plan.h"

struct PmKey { int32_t dp, qs, qe, score, subsc, nsub, ppool, part; };      // ppool: the place in its query's pool of the record's part-level parent when it was SECONDARY there, else -1
struct PmSrc { int64_t off; int32_t ncig, pad; };                          // the record's words in its part's array
struct PmSel { int32_t src, parent, subsc, nsub, kidx, cls; };             // per place in the order: src = place in the pool; kidx = -1: dropped
struct PmOut { int32_t src, parent, subsc, nsub, cls; };                   // per kept record, in output order: src = index in the whole pool

__device__ __forceinline__ bool pm_masks(int32_t qs_i, int32_t qe_i, int32_t qs_j, int32_t qe_j, float mask_level)
{
    const int32_t lo = qs_i > qs_j ? qs_i : qs_j, hi = qe_i < qe_j ? qe_i : qe_j;
    const int32_t ol = hi > lo ? hi - lo : 0;
    const int32_t li = qe_i - qs_i, lj = qe_j - qs_j, mn = li < lj ? li : lj;
    return (float)ol > mask_level * (float)mn;
}

// One wave (one 64-thread block) per query; its pool is key[qoff[q] .. qoff[q + 1]) in (part, rank) order.  skey (the keys in the
// order) and sel are the wave's own segment of two scratch arrays: what one phase stores there the next one reads behind a barrier.
__global__ void __launch_bounds__(64) k_pm_select(const PmKey *__restrict__ key, const int32_t *__restrict__ qoff, float mask_level, float pri_ratio,
                                                  int32_t best_n, int32_t secondary, PmKey *skey, PmSel *sel, int32_t *__restrict__ kcnt)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    const int32_t b = qoff[q], n = qoff[q + 1] - b;
    if (n == 0) { if (lane == 0) kcnt[q] = 0; return; }
    const uint64_t lt = (1ULL << lane) - 1;
    key += b; skey += b; sel += b;
    // 1. the order (dp_score descending, then part and rank ascending = the place in the pool): every lane counts the records before its own
    for (int32_t r0 = 0; r0 < n; r0 += 64) {
        const int32_t r = r0 + lane;
        PmKey mine = key[r < n ? r : n - 1];
        int32_t before = 0;
        for (int32_t x0 = 0; x0 < n; x0 += 64) {
            const int32_t xd = x0 + lane < n ? key[x0 + lane].dp : 0;
            const int32_t m = n - x0 < 64 ? n - x0 : 64;
            for (int32_t l = 0; l < m; ++l) {
                const int32_t d = __shfl(xd, l);
                before += (d > mine.dp || (d == mine.dp && x0 + l < r)) ? 1 : 0;
            }
        }
        if (r < n) { skey[before] = mine; sel[before].src = r; }
    }
    __syncthreads();
    // 2. parents: place i takes the first earlier place that is its own parent and masks it.  The own-parent flags of a finished tile are
    //    a ballot over its parents; the tile under way keeps its flags in `own` while i advances.
    for (int32_t i0 = 0; i0 < n; i0 += 64) {
        const int32_t i = i0 + lane, mi = n - i0 < 64 ? n - i0 : 64;
        const PmKey me = skey[i < n ? i : n - 1];
        int32_t par = -1;
        for (int32_t j0 = 0; j0 < i0; j0 += 64) {
            const int32_t j = j0 + lane;                    // (a whole tile: j0 + 64 <= i0 <= n)
            const int32_t jqs = skey[j].qs, jqe = skey[j].qe;
            uint64_t own = __ballot(sel[j].parent == j);
            while (own) {
                const int l = __ffsll((unsigned long long)own) - 1;
                own &= own - 1;
                const int32_t s = __shfl(jqs, l), e = __shfl(jqe, l);
                if (par < 0 && pm_masks(me.qs, me.qe, s, e, mask_level)) par = j0 + l;
            }
        }
        uint64_t own = 0;
        for (int32_t l = 0; l < mi; ++l) {
            const int32_t s = __shfl(me.qs, l), e = __shfl(me.qe, l), p = __shfl(par, l);
            if (p >= 0) continue;                           // (uniform: p is a broadcast)
            const uint64_t hit = __ballot(lane < l && ((own >> lane) & 1) && pm_masks(s, e, me.qs, me.qe, mask_level));
            if (hit) { if (lane == l) par = i0 + __ffsll((unsigned long long)hit) - 1; }
            else own |= 1ULL << l;
        }
        if (i < n) sel[i].parent = par < 0 ? i : par;
        __syncthreads();
    }
    // 3. subsc / n_sub of the own parents: what they had in their part, and every place they mask here -- but not the one that was the
    //    record's secondary in its part already (same part, part-level parent = this record: it is counted in what the record had)
    for (int32_t j0 = 0; j0 < n; j0 += 64) {
        const int32_t j = j0 + lane, jc = j < n ? j : n - 1;
        int32_t sub = skey[jc].subsc, cnt = skey[jc].nsub;
        const int32_t jsrc = sel[jc].src;
        const bool jown = sel[jc].parent == jc;
        for (int32_t i0 = j0; i0 < n; i0 += 64) {
            const int32_t ic = i0 + lane < n ? i0 + lane : n - 1, mi = n - i0 < 64 ? n - i0 : 64;
            const int32_t ip = sel[ic].parent, isc = skey[ic].score, ipp = skey[ic].ppool;
            for (int32_t l = 0; l < mi; ++l) {
                const int32_t p = __shfl(ip, l), s = __shfl(isc, l), pp = __shfl(ipp, l);
                if (p == j && i0 + l != j && pp != jsrc) { sub = s > sub ? s : sub; ++cnt; }
            }
        }
        if (j < n) { sel[j].subsc = jown ? sub : 0; sel[j].nsub = jown ? cnt : 0; }
    }
    // 4. kept: every own parent, and the first best_n secondaries within pri_ratio of their parent's score
    int32_t n_elig = 0, n_kept = 0;
    for (int32_t i0 = 0; i0 < n; i0 += 64) {
        const int32_t i = i0 + lane, ic = i < n ? i : n - 1;
        const int32_t p = sel[ic].parent;
        const bool own = i < n && p == i;
        const bool elig = i < n && !own && secondary && (float)skey[ic].dp >= (float)skey[p].dp * pri_ratio;
        const uint64_t em = __ballot(elig);
        const bool keep = own || (elig && n_elig + __popcll(em & lt) < best_n);
        const uint64_t km = __ballot(keep);
        if (i < n) { sel[i].kidx = keep ? n_kept + __popcll(km & lt) : -1; sel[i].cls = i == 0 ? TELR_F_PRIMARY : own ? TELR_F_SUPPL : TELR_F_SECONDARY; }
        n_elig += __popcll(em); n_kept += __popcll(km);
    }
    if (lane == 0) kcnt[q] = n_kept;
    __syncthreads();
    // 5. parent = the parent's index among the query's kept records (an own parent is always kept)
    for (int32_t i = lane; i < n; i += 64) sel[i].parent = sel[sel[i].parent].kidx;
}

// the kept records in output order (koff: where each query's start, from the scan of kcnt), and the lengths the next scan takes
__global__ void __launch_bounds__(64) k_pm_place(const PmSel *__restrict__ sel, const PmSrc *__restrict__ src, const int32_t *__restrict__ qoff,
                                                 const int32_t *__restrict__ koff, PmOut *__restrict__ out, int32_t *__restrict__ kncig)
{
    const int q = blockIdx.x;
    const int32_t b = qoff[q], n = qoff[q + 1] - b, k0 = koff[q];
    for (int32_t i = threadIdx.x; i < n; i += 64) {
        const PmSel s = sel[b + i];
        if (s.kidx < 0) continue;
        PmOut o; o.src = b + s.src; o.parent = s.parent; o.subsc = s.subsc; o.nsub = s.nsub; o.cls = s.cls;
        out[k0 + s.kidx] = o;
        kncig[k0 + s.kidx] = src[b + s.src].ncig;
    }
}

// One wave per kept record: its words from its part's array (base[part] + off) to coff[k] of the merged array.  Coalesced dword
// copies; where source and destination sit alike in their 16 bytes, the middle goes as dwordx4.
__global__ void __launch_bounds__(256) k_pm_gather(const PmOut *__restrict__ out, const PmKey *__restrict__ key, const PmSrc *__restrict__ src,
                                                   const uint32_t *const *__restrict__ base, const int64_t *__restrict__ coff, int32_t nk, uint32_t *__restrict__ dst)
{
    const int32_t k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= nk) return;
    const int32_t s = out[k].src;
    const PmSrc ps = src[s];
    const uint32_t *sp = base[key[s].part] + ps.off;
    uint32_t *dp = dst + coff[k];
    const int32_t n = ps.ncig;
    if ((((uintptr_t)sp ^ (uintptr_t)dp) & 15) == 0) {
        int32_t head = (int32_t)((16 - ((uintptr_t)dp & 15)) & 15) >> 2;
        if (head > n) head = n;
        if (lane < head) dp[lane] = sp[lane];
        const int32_t n4 = (n - head) >> 2;
        const uint4 *s4 = (const uint4*)(sp + head); uint4 *d4 = (uint4*)(dp + head);
        for (int32_t x = lane; x < n4; x += 64) d4[x] = s4[x];
        for (int32_t x = head + n4 * 4 + lane; x < n; x += 64) dp[x] = sp[x];
    } else {
        for (int32_t x = lane; x < n; x += 64) dp[x] = sp[x];
    }
}

// wall-clock milliseconds of the last telr_merge_parts call: checks, upload, select, scans (+ place), gather, host assembly, mirror copy, total,
// and the allocation of the result's pinned host array and its device array (which lies between scans and gather and is in neither).
// The device phases are separated by stream waits only under TELR_TRACE=merge (tools/part_merge_time.py sets it); without it they run back to back and
// only the sum of select / scans / gather is meaningful.
static float g_pm_ms[9] = {0};
extern "C" int telr_debug_merge_ms(float *out) { if (!out) return TELR_E_ARG; memcpy(out, g_pm_ms, sizeof(g_pm_ms)); return TELR_OK; }

static thread_local std::string g_part_plan_err;
extern "C" int telr_part_plan(int32_t n_targets, const int32_t *target_len, int64_t max_bases, int32_t *part_of, int32_t *n_parts)
{
    g_part_plan_err.clear();
    return part_plan(n_targets, target_len, max_bases, part_of, n_parts, &g_part_plan_err);
}
extern "C" const char *telr_part_plan_error(void) { return g_part_plan_err.c_str(); }

extern "C" int telr_merge_parts(telr_ctx *ctx, int32_t n_parts, const telr_result *const *parts, const int32_t *const *tid_map, const int32_t *n_part_targets,
                                int32_t n_queries, const telr_map_opt *mo, telr_result **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    auto bad = [&](const std::string &why) { ctx->err = "telr_merge_parts: " + why; return TELR_E_ARG; };
    if (!mo || !out) return bad("null options or output");
    if (mo->flags & TELR_MF_PER_TARGET) return bad("TELR_MF_PER_TARGET: per-target calls never compete across targets");
    if (n_parts < 0 || n_queries < 0 || (n_parts > 0 && (!parts || !tid_map || !n_part_targets))) return bad("a null pointer or a negative count");
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(now() - t0).count(); };
    static const bool trace = trace_on("merge");
    static const bool no_twin = ab_on("bam_no_twin");
    const auto t_all = now();
    auto t0 = t_all;
    memset(g_pm_ms, 0, sizeof(g_pm_ms));
    // ---- checks: every record of every part, before anything reaches the device
    const int P = n_parts, nq = n_queries;
    std::vector<const telr_aln*> pa((size_t)P); std::vector<int64_t> pn((size_t)P), pw((size_t)P);
    for (int p = 0; p < P; ++p) {
        if (!parts[p]) return bad("part " + std::to_string(p) + ": null result");
        result_wait(parts[p]);
        pa[p] = parts[p]->alns.data(); pn[p] = (int64_t)parts[p]->alns.size(); pw[p] = (int64_t)parts[p]->ncig;
    }
    { std::string why; const int rc = part_merge_check(P, pa.data(), pn.data(), pw.data(), tid_map, n_part_targets, nq, &why); if (rc != TELR_OK) { ctx->err = why; return rc; } }
    // ---- the pool: query-major, then part, then rank
    std::vector<int32_t> cnt((size_t)nq + 1, 0);
    for (int p = 0; p < P; ++p) for (int64_t i = 0; i < pn[p]; ++i) ++cnt[pa[p][i].qid];
    std::vector<int32_t> qoff((size_t)nq + 1);
    { int32_t o = 0; for (int q = 0; q < nq; ++q) { qoff[q] = o; o += cnt[q]; } qoff[nq] = o; }
    const int32_t np = qoff[nq];
    std::vector<PmKey> key((size_t)np); std::vector<PmSrc> src((size_t)np);
    std::vector<int32_t> ref_part((size_t)np), ref_idx((size_t)np), fill((size_t)nq, 0);
    for (int p = 0; p < P; ++p) {
        const telr_aln *a = pa[p];
        for (int64_t i = 0; i < pn[p]; ) {
            const int32_t q = a[i].qid, f0 = fill[q];
            int64_t j = i;
            for (; j < pn[p] && a[j].qid == q; ++j) {
                const telr_aln &r = a[j];
                const int32_t x = qoff[q] + fill[q]++;
                const bool sec = (r.flags & TELR_F_SECONDARY) != 0;
                PmKey &k = key[x];
                k.dp = r.dp_score; k.qs = r.qs; k.qe = r.qe; k.score = r.score; k.subsc = sec ? 0 : r.subsc; k.nsub = sec ? 0 : r.n_sub;
                k.ppool = sec ? f0 + r.parent : -1; k.part = p;
                src[x].off = r.cigar_off; src[x].ncig = r.n_cigar; src[x].pad = 0;
                ref_part[x] = p; ref_idx[x] = (int32_t)j;
            }
            i = j;
        }
    }
    g_pm_ms[0] = ms_since(t0); t0 = now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<telr_result> R(new telr_result());
    R->ctx = ctx;
    if (np == 0) {
        R->cig = cig_alloc(1);
        if (!R->cig) return TELR_E_NOMEM;
        R->cap = 1; R->ncig = 0;
        if (hipMalloc(&R->d_cig, 16) != hipSuccess) { (void)hipGetLastError(); return TELR_E_NOMEM; }      // an empty resident copy is a complete one
        R->d_cap = 4; R->twin_n = 0; R->twin_off = false;
        g_pm_ms[7] = ms_since(t_all);
        *out = R.release();
        return TELR_OK;
    }
    // ---- upload: keys, sources, counts; the words of the parts that hold no complete device copy
    PmKey *d_key, *d_skey; PmSrc *d_src; PmSel *d_sel; int32_t *d_cnt, *d_qoff, *d_kcnt, *d_koff; int64_t *d_tot; const uint32_t **d_base;
    TRY(ctx_buf_t(ctx, "pm_key", (size_t)np, &d_key)); TRY(ctx_buf_t(ctx, "pm_skey", (size_t)np, &d_skey)); TRY(ctx_buf_t(ctx, "pm_src", (size_t)np, &d_src));
    TRY(ctx_buf_t(ctx, "pm_sel", (size_t)np, &d_sel)); TRY(ctx_buf_t(ctx, "pm_cnt", (size_t)nq + 1, &d_cnt)); TRY(ctx_buf_t(ctx, "pm_qoff", (size_t)nq + 1, &d_qoff));
    TRY(ctx_buf_t(ctx, "pm_kcnt", (size_t)nq + 1, &d_kcnt)); TRY(ctx_buf_t(ctx, "pm_koff", (size_t)nq + 1, &d_koff)); TRY(ctx_buf_t(ctx, "pm_tot", 4, &d_tot));
    TRY(ctx_buf_t(ctx, "pm_base", (size_t)P, &d_base));
    std::vector<const uint32_t*> base((size_t)P, nullptr);
    size_t up_words = 0; bool any_twin = false;
    std::vector<char> twin((size_t)P);
    for (int p = 0; p < P; ++p) {
        const telr_result *r = parts[p];
        twin[p] = !no_twin && result_cigars_resident(r);
        if (twin[p]) any_twin = true; else up_words += (r->ncig + 3) & ~(size_t)3;
    }
    if (any_twin) HIPCHK(hipDeviceSynchronize());        // the last pieces of a mapped result's device copy were made on other streams
    uint32_t *d_up;
    TRY(ctx_buf_t(ctx, "pm_words", up_words, &d_up));
    { size_t o = 0;
      for (int p = 0; p < P; ++p) {
          const telr_result *r = parts[p];
          if (twin[p]) { base[p] = r->d_cig; continue; }
          base[p] = d_up + o;
          if (r->ncig) HIPCHK(hipMemcpyAsync(d_up + o, r->cig, r->ncig * 4, hipMemcpyHostToDevice, st));
          o += (r->ncig + 3) & ~(size_t)3;
      } }
    HIPCHK(hipMemcpyAsync(d_key, key.data(), (size_t)np * sizeof(PmKey), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_src, src.data(), (size_t)np * sizeof(PmSrc), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_cnt, cnt.data(), ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_base, base.data(), (size_t)P * sizeof(uint32_t*), hipMemcpyHostToDevice, st));
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_cnt, nq, d_qoff, nullptr, 0, nullptr, nullptr)));
    if (trace) HIPCHK(hipStreamSynchronize(st));
    g_pm_ms[1] = ms_since(t0); t0 = now();
    // ---- the selection
    hipLaunchKernelGGL(k_pm_select, dim3((unsigned)nq), dim3(64), 0, st, d_key, d_qoff, mo->mask_level, mo->pri_ratio, mo->best_n, mo->secondary, d_skey, d_sel, d_kcnt);
    HIPCHK(hipGetLastError());
    if (trace) HIPCHK(hipStreamSynchronize(st));
    g_pm_ms[2] = ms_since(t0); t0 = now();
    // ---- where the kept records and their words go
    int64_t tot[2] = {0, 0};
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_kcnt, nq, d_koff, d_tot, 0, nullptr, nullptr)));
    HIPCHK(hipMemcpyAsync(tot, d_tot, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int32_t nk = (int32_t)tot[0];
    if (nk < 1 || nk > np) { ctx->err = "telr_merge_parts: the kept count is out of range"; return TELR_E_HIP; }
    PmOut *d_out; int32_t *d_kncig; int64_t *d_coff;
    TRY(ctx_buf_t(ctx, "pm_out", (size_t)nk, &d_out)); TRY(ctx_buf_t(ctx, "pm_kncig", (size_t)nk + 1, &d_kncig)); TRY(ctx_buf_t(ctx, "pm_coff", (size_t)nk + 1, &d_coff));
    hipLaunchKernelGGL(k_pm_place, dim3((unsigned)nq), dim3(64), 0, st, d_sel, d_src, d_qoff, d_koff, d_out, d_kncig);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_kncig, nk, d_coff, d_tot + 1, 0, nullptr, nullptr)));
    HIPCHK(hipMemcpyAsync(tot + 1, d_tot + 1, 8, hipMemcpyDeviceToHost, st));
    std::vector<PmOut> h_out((size_t)nk); std::vector<int64_t> h_coff((size_t)nk + 1);
    HIPCHK(hipMemcpyAsync(h_out.data(), d_out, (size_t)nk * sizeof(PmOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_coff.data(), d_coff, ((size_t)nk + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t nw = tot[1];
    { int64_t have = 0; for (int p = 0; p < P; ++p) have += pw[p]; if (nw < 0 || nw > have) { ctx->err = "telr_merge_parts: the word count is out of range"; return TELR_E_HIP; } }
    g_pm_ms[3] = ms_since(t0); t0 = now();
    // ---- the words: gathered on the device into the result's own array
    R->cig = cig_alloc((size_t)nw + 1);
    if (!R->cig) return TELR_E_NOMEM;
    R->cap = (size_t)nw + 1; R->ncig = (size_t)nw;
    if (hipMalloc(&R->d_cig, ((size_t)nw + 4) * 4) != hipSuccess) { (void)hipGetLastError(); ctx->err = "telr_merge_parts: no device memory for the merged CIGAR array"; return TELR_E_NOMEM; }
    R->d_cap = (size_t)nw + 4;
    g_pm_ms[8] = ms_since(t0); t0 = now();
    hipLaunchKernelGGL(k_pm_gather, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, d_out, d_key, d_src, d_base, d_coff, nk, R->d_cig);
    HIPCHK(hipGetLastError());
    if (trace) HIPCHK(hipStreamSynchronize(st));
    g_pm_ms[4] = ms_since(t0); t0 = now();
    // ---- the records (the gather runs underneath)
    R->alns.resize((size_t)nk);
    telr_aln *dst = R->alns.data();
    parallel_ranges(host_threads(), nk, [&](int, int k0, int k1) {
        for (int k = k0; k < k1; ++k) {
            const PmOut &o = h_out[k];
            const int p = ref_part[o.src];
            telr_aln r = pa[p][ref_idx[o.src]];
            r.tid = tid_map[p][r.tid];
            r.parent = o.parent; r.subsc = o.subsc; r.n_sub = o.nsub;
            r.flags = (r.flags & ~(TELR_F_PRIMARY | TELR_F_SECONDARY | TELR_F_SUPPL)) | o.cls;
            r.cigar_off = h_coff[k];
            r.mapq = mapq_of(r, mo);
            dst[k] = r;
        }
    });
    g_pm_ms[5] = ms_since(t0); t0 = now();
    // ---- the one mirror copy
    if (nw) HIPCHK(hipMemcpyAsync(R->cig, R->d_cig, (size_t)nw * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    R->twin_n = R->ncig; R->twin_off = false;
    g_pm_ms[6] = ms_since(t0); g_pm_ms[7] = ms_since(t_all);
    *out = R.release();
    return TELR_OK;
}
