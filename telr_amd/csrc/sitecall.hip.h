// The supporters of insertion sites the caller names, on the device (include/telr_hip.h: telr_call_at_sites).  The
// signatures are those of telr_call_insertions (inscall.hip.h: InsFront); where that entry discovers clusters by single linkage and
// thresholds them, this one assigns every signature to the nearest of the given sites within reach and reports every site.  An own
// definition, NOT Sniffles' --genotype-vcf.  Count, scan, emit like the rest of the stage: every store goes to an index that a scan gave.
//
//   k_site_assign   one lane per sorted signature: a lower bound of its (tid, pos) key in the uploaded site keys, the two sites around
//                   it, the distance rule (64-bit, so pos +- reach cannot wrap), the length test: the site id or -1, and a keep flag;
//   k_site_compact  after a scan of the keep flags, the kept signatures gathered into a dense array with their site ids and sized flags;
//                   there the site id is non-decreasing, so a site's run is contiguous;
//   k_site_starts   one lane per site: cstart[c] = a lower bound of c in the site ids, cstart[n_sites] = the kept count;
//   then ins_collect (inscall.hip.h) with every site a call, whose tid and pos come from the site.
#pragma once

__global__ void __launch_bounds__(256) k_site_assign(const telr_ins_sig *__restrict__ sig, int64_t n, const uint64_t *__restrict__ skeys, const telr_ins_site *__restrict__ sites,
                                                     int32_t ns, int32_t reach, int32_t len_pct, int32_t *__restrict__ sid, int32_t *__restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { keep[i] = 0; return; }                      // the scan's trailing 0
    const telr_ins_sig s = sig[i];
    const int64_t b = d_bound<false>(skeys, ns, ((uint64_t)(uint32_t)s.tid << 32) | (uint32_t)s.pos);
    int64_t best = -1, bd = 0;
    if (b > 0) {                                              // the last site below the signature's key
        const telr_ins_site c = sites[b - 1];
        const int64_t d = (int64_t)s.pos - c.pos;
        if (c.tid == s.tid && d <= reach) { best = b - 1; bd = d; }
    }
    if (b < ns) {                                             // the first site at or above it: it wins only when strictly nearer
        const telr_ins_site c = sites[b];
        const int64_t d = (int64_t)c.pos - s.pos;
        if (c.tid == s.tid && d <= reach && (best < 0 || d < bd)) best = b;
    }
    if (best >= 0 && s.kind != 2 && len_pct > 0) {            // a rejected signature is not handed to the other site
        const int64_t L = sites[best].len, d = s.len > L ? (int64_t)s.len - L : L - s.len;
        if (L > 0 && 100 * d > (int64_t)len_pct * L) best = -1;
    }
    sid[i] = (int32_t)best; keep[i] = best >= 0 ? 1 : 0;
}
// kx = the exclusive scan of keep (kx[n] = the kept count): the dense arrays, sized with its trailing 0
__global__ void __launch_bounds__(256) k_site_compact(const telr_ins_sig *__restrict__ sig, int64_t n, const int32_t *__restrict__ sid, const int32_t *__restrict__ keep,
                                                      const int32_t *__restrict__ kx, telr_ins_sig *__restrict__ ksig, int32_t *__restrict__ kcid, int32_t *__restrict__ ksized)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { ksized[kx[n]] = 0; return; }
    if (!keep[i]) return;
    const telr_ins_sig s = sig[i];
    const int32_t o = kx[i];
    ksig[o] = s; kcid[o] = sid[i]; ksized[o] = s.kind != 2 ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_site_starts(const int32_t *__restrict__ kcid, int32_t nk, int32_t ns, int32_t *__restrict__ cstart)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > ns) return;
    int32_t lo = 0, hi = nk;                                  // first kept signature with a site id >= c (c == ns: nk)
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (kcid[mid] < (int32_t)c) lo = mid + 1; else hi = mid; }
    cstart[c] = lo;
}

extern "C" void telr_site_opt_default(telr_site_opt *o)
{
    if (!o) return;
    o->reach = 50; o->len_pct = 0; o->reserved[0] = o->reserved[1] = 0;
}

extern "C" int telr_call_at_sites(telr_ctx *ctx, const telr_result *r, int32_t n_targets, const telr_ins_opt *opt,
                                  const telr_ins_site *sites, int64_t n_sites, const telr_site_opt *sopt, telr_ins_calls **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    InsFront F;
    TRY(F.check(ctx, "telr_call_at_sites", r, out != nullptr, n_targets, opt, false));
    telr_site_opt SO;
    if (sopt) SO = *sopt; else telr_site_opt_default(&SO);
    if (SO.reach < 0) return F.bad("negative reach");
    if (SO.len_pct < 0 || SO.len_pct > 100) return F.bad("len_pct outside 0..100");
    if (SO.reserved[0] || SO.reserved[1]) return F.bad("non-zero reserved field");
    if (n_sites < 0) return F.bad("negative n_sites");
    if (n_sites > 0 && !sites) return F.bad("null sites");
    if (n_sites >= 0x7ffffff0LL) { ctx->err = "telr_call_at_sites: too many sites"; return TELR_E_RANGE; }
    std::vector<uint64_t> skeys((size_t)n_sites);
    for (int64_t c = 0; c < n_sites; ++c) {
        const telr_ins_site &s = sites[c];
        const char *what = (s.tid < 0 || s.tid >= n_targets) ? "tid outside n_targets" : s.pos < 0 ? "negative pos" : s.len < 0 ? "negative len" : nullptr;
        skeys[(size_t)c] = ((uint64_t)(uint32_t)s.tid << 32) | (uint32_t)s.pos;
        if (!what && c > 0 && skeys[(size_t)c] <= skeys[(size_t)c - 1]) what = "sites not strictly ascending by (tid, pos)";
        if (what) return F.bad("site " + std::to_string(c) + ": " + what);
    }
    // a call per site without a kept signature; the device fills them in below when there is one
    telr_ins_calls *C = new telr_ins_calls();
    std::unique_ptr<telr_ins_calls> guard(C);
    C->calls.resize((size_t)n_sites); C->read_off.assign((size_t)n_sites + 1, 0);
    for (int64_t c = 0; c < n_sites; ++c) C->calls[(size_t)c] = telr_ins_call{sites[c].tid, sites[c].pos, 0, 0, 0, -1};
    if (n_sites == 0 || F.er.empty()) { *out = guard.release(); return TELR_OK; }
    TRY(F.signatures());
    const int64_t N = F.N;
    if (N == 0) { *out = guard.release(); return TELR_OK; }
    hipStream_t st = ctx->stream;
    const int32_t ns = (int32_t)n_sites;
    uint64_t *d_skeys; telr_ins_site *d_sites; int32_t *d_sid, *d_keep, *d_kx;
    TRY(ctx_buf_t(ctx, "site_keys", (size_t)ns, &d_skeys));
    TRY(ctx_buf_t(ctx, "site_sites", (size_t)ns, &d_sites));
    TRY(ctx_buf_t(ctx, "site_sid", (size_t)N, &d_sid));
    TRY(ctx_buf_t(ctx, "site_keep", (size_t)N + 1, &d_keep));
    TRY(ctx_buf_t(ctx, "site_kx", (size_t)N + 1, &d_kx));
    HIPCHK(hipMemcpyAsync(d_skeys, skeys.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_sites, sites, (size_t)ns * sizeof(telr_ins_site), hipMemcpyHostToDevice, st));
    const dim3 gN1 = grid256(N + 1);
    hipLaunchKernelGGL(k_site_assign, gN1, dim3(256), 0, st, F.d_sig, N, d_skeys, d_sites, ns, SO.reach, SO.len_pct, d_sid, d_keep);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_keep, (int32_t)N, d_kx, nullptr, 0, nullptr, nullptr)));
    int32_t K = 0;
    HIPCHK(hipMemcpyAsync(&K, d_kx + N, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                         // (the uploads from skeys and sites are done too)
    if (K == 0) { *out = guard.release(); return TELR_OK; }
    telr_ins_sig *d_ksig; int32_t *d_kcid, *d_ksized, *d_sx, *d_cstart;
    TRY(ctx_buf_t(ctx, "site_ksig", (size_t)K, &d_ksig));
    TRY(ctx_buf_t(ctx, "site_kcid", (size_t)K, &d_kcid));
    TRY(ctx_buf_t(ctx, "site_ksized", (size_t)K + 1, &d_ksized));
    TRY(ctx_buf_t(ctx, "site_sx", (size_t)K + 1, &d_sx));
    TRY(ctx_buf_t(ctx, "site_cstart", (size_t)ns + 1, &d_cstart));
    hipLaunchKernelGGL(k_site_compact, gN1, dim3(256), 0, st, F.d_sig, N, d_sid, d_keep, d_kx, d_ksig, d_kcid, d_ksized);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_ksized, K, d_sx, nullptr, 0, nullptr, nullptr)));
    hipLaunchKernelGGL(k_site_starts, grid256((int64_t)ns + 1), dim3(256), 0, st, d_kcid, K, ns, d_cstart);
    HIPCHK(hipGetLastError());
    TRY(ins_collect(F, d_ksig, K, d_kcid, d_cstart, ns, d_sx, 0, 0, d_sites, C));
    *out = guard.release();
    return TELR_OK;
}
