// Several samples' insertion calls merged into one site list, on the device (include/telr_hip.h: telr_merge_sites).
// The machinery of inscall.hip.h one level up: many samples' calls -> clusters -> sites, in the shape telr_call_at_sites takes.  An own,
// fully specified definition, NOT bcftools merge, SURVIVOR or Jasmine.  Count, scan, emit like the rest of the stage: every store goes to
// an index that a scan gave (or to the lane's own), no atomic decides a position, and no lane loops over a cluster's members -- one
// cluster may hold every entry.
//
//   sort A         LSD over the complete key with perm_sort_round (stage2_common.hip.h): (sample, len), pos, (tid, group) from the
//                  identity, so the input index breaks the last tie; the bit counts come from the data's maxima;
//   clusters       k_coh_heads (head and sized flags, the gap in 64 bits), two scans, k_ins_cid (inscall.hip.h, as it is);
//   samples        within a cluster the key order is by position first, so a sample's entries are NOT adjacent there: one more sort by
//                  (cluster, sample), k_coh_distinct flags the first entry of every (cluster, sample) run, a scan counts them, and
//                  k_coh_dsamp writes the distinct sample numbers densely: a cluster's are a contiguous ascending run;
//   lengths        a sort by (cluster, unsized, len, sample, i): the median, len_min, len_max and rep are reads at computed indices;
//   sites          k_coh_sites, one lane per cluster, writes the site and the min_samples keep flag; a scan, k_coh_compact;
//   final order    a sort of the kept sites by (tid, pos, n_samples desc, n_members desc, group);
//   shadow, crowd  k_coh_shadow (one lane per site: its predecessor), a scan of the not-shadowed flags, k_coh_upos (the dense positions
//                  of the not-shadowed sites), k_coh_flags (the winner = the not-shadowed site before a shadowed one; the neighbours of
//                  a not-shadowed one are the dense array's entries around its own);
//   lists          the scans of n_members and n_samples in final order are the offsets; k_coh_members / k_coh_samples take one lane
//                  per OUTPUT slot, find its site by a bound in the offsets and read its value: coalesced stores, gathered loads.
#pragma once

struct telr_cohort_sites {
    std::vector<telr_cohort_site> sites;
    std::vector<int64_t> member_off, sample_off;
    std::vector<int32_t> members, samples;
};

// the keys of the sort rounds (perm_sort_round); sb / lb / gb / mb: the bits of the largest sample / len / group / of a count
struct CohKeySL { int lb; __device__ uint64_t operator()(const telr_cohort_entry &e, uint32_t) const { return ((uint64_t)(uint32_t)e.sample << lb) | (uint32_t)e.len; } };
struct CohKeyP  { __device__ uint64_t operator()(const telr_cohort_entry &e, uint32_t) const { return (uint32_t)e.pos; } };
struct CohKeyTG { int gb; __device__ uint64_t operator()(const telr_cohort_entry &e, uint32_t) const { return ((uint64_t)(uint32_t)e.tid << gb) | (uint32_t)e.group; } };
// over the entries in key order (p = the entry's place there): cid[p] its cluster, ord[p] its input index
struct CohKeyCS { const int32_t *cid; int sb; __device__ uint64_t operator()(const telr_cohort_entry &e, uint32_t p) const { return ((uint64_t)(uint32_t)cid[p] << sb) | (uint32_t)e.sample; } };
struct CohKeyI  { const uint32_t *ord; __device__ uint64_t operator()(const telr_cohort_entry &, uint32_t p) const { return ord[p]; } };
struct CohKeyLS { int sb; __device__ uint64_t operator()(const telr_cohort_entry &e, uint32_t) const { return ((uint64_t)(uint32_t)e.len << sb) | (uint32_t)e.sample; } };
struct CohKeyCU { const int32_t *cid; __device__ uint64_t operator()(const telr_cohort_entry &e, uint32_t p) const { return ((uint64_t)(uint32_t)cid[p] << 1) | (e.len > 0 ? 0u : 1u); } };
// over the kept sites: counts descend, so a count c sorts as top - c (top >= every count)
struct CohKeyMG { int32_t top; int gb; __device__ uint64_t operator()(const telr_cohort_site &s, uint32_t) const { return ((uint64_t)(uint32_t)(top - s.n_members) << gb) | (uint32_t)s.group; } };
struct CohKeyPS { int32_t top; int mb; __device__ uint64_t operator()(const telr_cohort_site &s, uint32_t) const { return ((uint64_t)(uint32_t)s.pos << mb) | (uint32_t)(top - s.n_samples); } };
struct CohKeyT  { __device__ uint64_t operator()(const telr_cohort_site &s, uint32_t) const { return (uint32_t)s.tid; } };

// s = the entries in key order: head[i] = entry i starts a cluster, sized[i] = it carries a length
__global__ void __launch_bounds__(256) k_coh_heads(const telr_cohort_entry *__restrict__ s, int64_t n, int32_t dist, int32_t *__restrict__ head, int32_t *__restrict__ sized)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const telr_cohort_entry e = s[i];
    int32_t h = 1;
    if (i > 0) { const telr_cohort_entry p = s[i - 1]; h = (p.tid != e.tid || p.group != e.group || (int64_t)e.pos - p.pos > dist) ? 1 : 0; }
    head[i] = h; sized[i] = e.len > 0 ? 1 : 0;
}
// over the order of the (cluster, sample) sort: dflag[j] = the first entry of its sample in its cluster
__global__ void __launch_bounds__(256) k_coh_distinct(const telr_cohort_entry *__restrict__ s, const int32_t *__restrict__ cid, const uint32_t *__restrict__ perm, int64_t n,
                                                      int32_t *__restrict__ dflag)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = perm[j];
    int32_t d = 1;
    if (j > 0) { const uint32_t q = perm[j - 1]; d = (cid[q] != cid[p] || s[q].sample != s[p].sample) ? 1 : 0; }
    dflag[j] = d;
}
// dx = the exclusive scan of dflag: the distinct (cluster, sample) pairs' sample numbers, densely; a cluster's are [dx[lo], dx[hi])
__global__ void __launch_bounds__(256) k_coh_dsamp(const telr_cohort_entry *__restrict__ s, const uint32_t *__restrict__ perm, int64_t n, const int32_t *__restrict__ dflag,
                                                   const int32_t *__restrict__ dx, int32_t *__restrict__ dsamp)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !dflag[j]) return;
    dsamp[dx[j]] = s[perm[j]].sample;
}
// one lane per cluster [lo, hi) of the key order: its site (flags and winner come later) and keep = enough samples.  zx = the scan of the
// sized flags; perm_len = the order of the length sort, where a cluster's sized members come first, ascending by (len, sample, i)
__global__ void __launch_bounds__(256) k_coh_sites(const telr_cohort_entry *__restrict__ s, const uint32_t *__restrict__ ord, const int32_t *__restrict__ cstart, int32_t nc,
                                                   const int32_t *__restrict__ dx, const int32_t *__restrict__ zx, const uint32_t *__restrict__ perm_len, int32_t min_samples,
                                                   telr_cohort_site *__restrict__ raw, int32_t *__restrict__ keep)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const int32_t lo = cstart[c], hi = cstart[c + 1], m = hi - lo, ns = zx[hi] - zx[lo], mid = lo + (m - 1) / 2;
    const telr_cohort_entry first = s[lo];
    telr_cohort_site k;
    k.tid = first.tid; k.group = first.group; k.pos = s[mid].pos; k.pos_min = first.pos; k.pos_max = s[hi - 1].pos;
    k.n_members = m; k.n_samples = dx[hi] - dx[lo]; k.n_sized = ns;
    if (ns > 0) {
        const uint32_t r = perm_len[lo + (ns - 1) / 2];
        k.len = s[r].len; k.rep = (int32_t)ord[r]; k.len_min = s[perm_len[lo]].len; k.len_max = s[perm_len[lo + ns - 1]].len;
    } else { k.len = k.len_min = k.len_max = 0; k.rep = (int32_t)ord[mid]; }
    k.flags = 0; k.winner = -1;
    raw[c] = k; keep[c] = k.n_samples >= min_samples ? 1 : 0;
}
// kx = the exclusive scan of keep: the kept sites densely, each with its cluster
__global__ void __launch_bounds__(256) k_coh_compact(const telr_cohort_site *__restrict__ raw, const int32_t *__restrict__ keep, const int32_t *__restrict__ kx, int32_t nc,
                                                     telr_cohort_site *__restrict__ out, int32_t *__restrict__ cl)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc || !keep[c]) return;
    const int32_t o = kx[c];
    out[o] = raw[c]; cl[o] = (int32_t)c;
}
// f = the kept sites in final order: open[k] = site k is not shadowed; mcnt / scnt = the lengths of its two lists
__global__ void __launch_bounds__(256) k_coh_shadow(const telr_cohort_site *__restrict__ f, int32_t K, int32_t *__restrict__ open, int32_t *__restrict__ mcnt, int32_t *__restrict__ scnt)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const telr_cohort_site a = f[k];
    int32_t o = 1;
    if (k > 0) { const telr_cohort_site b = f[k - 1]; o = (b.tid == a.tid && b.pos == a.pos) ? 0 : 1; }
    open[k] = o; mcnt[k] = a.n_members; scnt[k] = a.n_samples;
}
// ox = the exclusive scan of open: upos[r] = the output index of the r-th site that is not shadowed
__global__ void __launch_bounds__(256) k_coh_upos(const int32_t *__restrict__ open, const int32_t *__restrict__ ox, int32_t K, int32_t *__restrict__ upos)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K || !open[k]) return;
    upos[ox[k]] = (int32_t)k;
}
// a shadowed site: the first site of its (tid, pos) run is the last not-shadowed one before it; a not-shadowed one: its neighbours among
// the not-shadowed (ox[K] of them) are upos[r - 1] and upos[r + 1]
__global__ void __launch_bounds__(256) k_coh_flags(telr_cohort_site *__restrict__ f, int32_t K, const int32_t *__restrict__ open, const int32_t *__restrict__ ox,
                                                   const int32_t *__restrict__ upos, int32_t dist)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int32_t r = ox[k];
    if (!open[k]) { f[k].flags = TELR_COHORT_SHADOWED; f[k].winner = upos[r - 1]; return; }      // a shadowed site has a predecessor: r >= 1
    const int32_t tid = f[k].tid, pos = f[k].pos, nu = ox[K];
    bool crowded = false;
    // (only tid and pos of a neighbour are read: its flags and winner are another lane's to write)
    if (r > 0) { const int32_t b = upos[r - 1]; crowded = f[b].tid == tid && (int64_t)pos - f[b].pos <= dist; }
    if (!crowded && r + 1 < nu) { const int32_t b = upos[r + 1]; crowded = f[b].tid == tid && (int64_t)f[b].pos - pos <= dist; }
    f[k].flags = crowded ? TELR_COHORT_CROWDED : 0; f[k].winner = -1;
}
// one lane per member slot t of the output: its site k by a bound in the offsets, then the (t - moff[k])-th entry of k's cluster
__global__ void __launch_bounds__(256) k_coh_members(const int64_t *__restrict__ moff, int32_t K, int64_t M, const int32_t *__restrict__ cl, const int32_t *__restrict__ cstart,
                                                     const uint32_t *__restrict__ ord, int32_t *__restrict__ members)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= M) return;
    const int32_t k = d_pair_owner(moff, K, t);
    members[t] = (int32_t)ord[cstart[cl[k]] + (t - moff[k])];
}
__global__ void __launch_bounds__(256) k_coh_samples(const int64_t *__restrict__ soff, int32_t K, int64_t S, const int32_t *__restrict__ cl, const int32_t *__restrict__ cstart,
                                                     const int32_t *__restrict__ dx, const int32_t *__restrict__ dsamp, int32_t *__restrict__ samples)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= S) return;
    const int32_t k = d_pair_owner(soff, K, t);
    samples[t] = dsamp[dx[cstart[cl[k]]] + (t - soff[k])];
}

extern "C" void telr_cohort_opt_default(telr_cohort_opt *o)
{
    if (!o) return;
    o->dist = 50; o->min_samples = 1; o->reserved[0] = o->reserved[1] = 0;
}
extern "C" int64_t telr_cohort_sites_count(const telr_cohort_sites *s) { return s ? (int64_t)s->sites.size() : 0; }
extern "C" const telr_cohort_site *telr_cohort_sites_sites(const telr_cohort_sites *s) { return s ? s->sites.data() : nullptr; }
extern "C" const int64_t *telr_cohort_sites_member_off(const telr_cohort_sites *s) { return s ? s->member_off.data() : nullptr; }
extern "C" const int32_t *telr_cohort_sites_members(const telr_cohort_sites *s) { return s ? s->members.data() : nullptr; }
extern "C" const int64_t *telr_cohort_sites_sample_off(const telr_cohort_sites *s) { return s ? s->sample_off.data() : nullptr; }
extern "C" const int32_t *telr_cohort_sites_samples(const telr_cohort_sites *s) { return s ? s->samples.data() : nullptr; }
extern "C" void telr_cohort_sites_free(telr_cohort_sites *s) { delete s; }

extern "C" int telr_merge_sites(telr_ctx *ctx, const telr_cohort_entry *e, int64_t n, int32_t n_targets, const telr_cohort_opt *opt, telr_cohort_sites **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    auto bad = [&](const std::string &why) { ctx->err = "telr_merge_sites: " + why; return TELR_E_ARG; };
    if (!out) return bad("null output");
    if (n < 0) return bad("negative n");
    if (n > 0 && !e) return bad("null entries");
    telr_cohort_opt O;
    if (opt) O = *opt; else telr_cohort_opt_default(&O);
    if (O.dist < 0) return bad("negative dist");
    if (O.min_samples < 1) return bad("min_samples below 1");
    if (O.reserved[0] || O.reserved[1]) return bad("non-zero reserved field");
    if (n >= 0x7ffffff0LL) { ctx->err = "telr_merge_sites: too many entries"; return TELR_E_RANGE; }
    int32_t max_pos = 0, max_len = 0, max_sample = 0, max_group = 0;
    for (int64_t i = 0; i < n; ++i) {
        const telr_cohort_entry &x = e[i];
        const char *what = (x.tid < 0 || x.tid >= n_targets) ? "tid outside n_targets" : x.pos < 0 ? "negative pos" : x.len < 0 ? "negative len"
                         : x.sample < 0 ? "negative sample" : x.group < 0 ? "negative group" : nullptr;
        if (what) return bad("entry " + std::to_string(i) + ": " + what);
        max_pos = std::max(max_pos, x.pos); max_len = std::max(max_len, x.len); max_sample = std::max(max_sample, x.sample); max_group = std::max(max_group, x.group);
    }
    telr_cohort_sites *C = new telr_cohort_sites();
    std::unique_ptr<telr_cohort_sites> guard(C);
    C->member_off.assign(1, 0); C->sample_off.assign(1, 0);
    if (n == 0) { *out = guard.release(); return TELR_OK; }

    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)n;
    const int pb = bits_of((uint64_t)max_pos), lb = bits_of((uint64_t)max_len), sb = bits_of((uint64_t)max_sample), gb = bits_of((uint64_t)max_group);
    const int tb = bits_of((uint64_t)n_targets - 1);
    // ---- the entries in key order: d_s, with their input indices d_ord
    telr_cohort_entry *d_in, *d_s; uint32_t *d_ord; int64_t *d_tot;
    TRY(ctx_buf_t(ctx, "coh_in", N, &d_in));
    TRY(ctx_buf_t(ctx, "coh_s", N, &d_s));
    TRY(ctx_buf_t(ctx, "coh_ord", N, &d_ord));
    TRY(ctx_buf_t(ctx, "coh_tot", 4, &d_tot));
    HIPCHK(hipMemcpyAsync(d_in, e, N * sizeof(telr_cohort_entry), hipMemcpyHostToDevice, st));
    PermSort S;
    TRY(S.alloc(ctx, "coh_", N));
    perm_iota(ctx, S, n);
    TRY(perm_sort_round(ctx, S, d_in, n, CohKeySL{lb}, sb + lb));
    TRY(perm_sort_round(ctx, S, d_in, n, CohKeyP{}, pb));
    TRY(perm_sort_round(ctx, S, d_in, n, CohKeyTG{gb}, tb + gb));
    perm_gather(ctx, S, d_in, n, d_s);
    HIPCHK(hipMemcpyAsync(d_ord, S.perm, N * 4, hipMemcpyDeviceToDevice, st));
    // ---- clusters
    int32_t *d_head, *d_hx, *d_sized, *d_zx, *d_cid, *d_cstart;
    TRY(ctx_buf_t(ctx, "coh_head", N, &d_head));
    TRY(ctx_buf_t(ctx, "coh_hx", N + 1, &d_hx));
    TRY(ctx_buf_t(ctx, "coh_sized", N, &d_sized));
    TRY(ctx_buf_t(ctx, "coh_zx", N + 1, &d_zx));
    TRY(ctx_buf_t(ctx, "coh_cid", N, &d_cid));
    TRY(ctx_buf_t(ctx, "coh_cstart", N + 1, &d_cstart));
    const dim3 gN = grid256(n), gN1 = grid256(n + 1);
    hipLaunchKernelGGL(k_coh_heads, gN, dim3(256), 0, st, d_s, n, O.dist, d_head, d_sized);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_head, (int32_t)n, d_hx, nullptr, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_sized, (int32_t)n, d_zx, nullptr, 0, nullptr, nullptr)));
    hipLaunchKernelGGL(k_ins_cid, gN1, dim3(256), 0, st, d_head, d_hx, n, d_cid, d_cstart);
    int32_t nc = 0;
    HIPCHK(hipMemcpyAsync(&nc, d_hx + n, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                         // (the upload from e is done too)
    const int cb = bits_of((uint64_t)nc - 1);
    // ---- the distinct samples of every cluster
    int32_t *d_dflag, *d_dx, *d_dsamp; uint32_t *d_permd;
    TRY(ctx_buf_t(ctx, "coh_dflag", N, &d_dflag));
    TRY(ctx_buf_t(ctx, "coh_dx", N + 1, &d_dx));
    TRY(ctx_buf_t(ctx, "coh_dsamp", N, &d_dsamp));
    TRY(ctx_buf_t(ctx, "coh_permd", N, &d_permd));
    perm_iota(ctx, S, n);
    TRY(perm_sort_round(ctx, S, d_s, n, CohKeyCS{d_cid, sb}, cb + sb));
    HIPCHK(hipMemcpyAsync(d_permd, S.perm, N * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_coh_distinct, gN, dim3(256), 0, st, d_s, d_cid, d_permd, n, d_dflag);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_dflag, (int32_t)n, d_dx, nullptr, 0, nullptr, nullptr)));
    hipLaunchKernelGGL(k_coh_dsamp, gN, dim3(256), 0, st, d_s, d_permd, n, d_dflag, d_dx, d_dsamp);
    // ---- lengths: (cluster, unsized, len, sample, i)
    perm_iota(ctx, S, n);
    TRY(perm_sort_round(ctx, S, d_s, n, CohKeyI{d_ord}, bits_of((uint64_t)n - 1)));
    TRY(perm_sort_round(ctx, S, d_s, n, CohKeyLS{sb}, lb + sb));
    TRY(perm_sort_round(ctx, S, d_s, n, CohKeyCU{d_cid}, cb + 1));
    // ---- a site per cluster, the kept ones densely
    telr_cohort_site *d_raw, *d_kept, *d_f; int32_t *d_keep, *d_kx, *d_kcl, *d_cl;
    TRY(ctx_buf_t(ctx, "coh_raw", (size_t)nc, &d_raw));
    TRY(ctx_buf_t(ctx, "coh_keep", (size_t)nc, &d_keep));
    TRY(ctx_buf_t(ctx, "coh_kx", (size_t)nc + 1, &d_kx));
    const dim3 gC = grid256(nc);
    hipLaunchKernelGGL(k_coh_sites, gC, dim3(256), 0, st, d_s, d_ord, d_cstart, nc, d_dx, d_zx, S.perm, O.min_samples, d_raw, d_keep);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_keep, nc, d_kx, nullptr, 0, nullptr, nullptr)));
    int32_t K = 0;
    HIPCHK(hipMemcpyAsync(&K, d_kx + nc, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (K == 0) { *out = guard.release(); return TELR_OK; }
    TRY(ctx_buf_t(ctx, "coh_kept", (size_t)K, &d_kept));
    TRY(ctx_buf_t(ctx, "coh_f", (size_t)K, &d_f));
    TRY(ctx_buf_t(ctx, "coh_kcl", (size_t)K, &d_kcl));
    TRY(ctx_buf_t(ctx, "coh_cl", (size_t)K, &d_cl));
    hipLaunchKernelGGL(k_coh_compact, gC, dim3(256), 0, st, d_raw, d_keep, d_kx, nc, d_kept, d_kcl);
    HIPCHK(hipGetLastError());
    // ---- final order: (tid, pos, n_samples descending, n_members descending, group)
    const int32_t top_m = (int32_t)n, top_s = (int32_t)std::min<int64_t>(n, (int64_t)max_sample + 1);
    perm_iota(ctx, S, K);
    TRY(perm_sort_round(ctx, S, d_kept, K, CohKeyMG{top_m, gb}, bits_of((uint64_t)top_m) + gb));
    TRY(perm_sort_round(ctx, S, d_kept, K, CohKeyPS{top_s, bits_of((uint64_t)top_s)}, pb + bits_of((uint64_t)top_s)));
    TRY(perm_sort_round(ctx, S, d_kept, K, CohKeyT{}, tb));
    perm_gather(ctx, S, d_kept, K, d_f);
    perm_gather(ctx, S, d_kcl, K, d_cl);
    // ---- shadowed and crowded sites, the offsets of the lists
    int32_t *d_open, *d_ox, *d_upos, *d_mcnt, *d_scnt; int64_t *d_moff, *d_soff;
    TRY(ctx_buf_t(ctx, "coh_open", (size_t)K, &d_open));
    TRY(ctx_buf_t(ctx, "coh_ox", (size_t)K + 1, &d_ox));
    TRY(ctx_buf_t(ctx, "coh_upos", (size_t)K, &d_upos));
    TRY(ctx_buf_t(ctx, "coh_mcnt", (size_t)K, &d_mcnt));
    TRY(ctx_buf_t(ctx, "coh_scnt", (size_t)K, &d_scnt));
    TRY(ctx_buf_t(ctx, "coh_moff", (size_t)K + 1, &d_moff));
    TRY(ctx_buf_t(ctx, "coh_soff", (size_t)K + 1, &d_soff));
    const dim3 gK = grid256(K);
    hipLaunchKernelGGL(k_coh_shadow, gK, dim3(256), 0, st, d_f, K, d_open, d_mcnt, d_scnt);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_open, K, d_ox, nullptr, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_mcnt, K, d_moff, d_tot, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_scnt, K, d_soff, d_tot + 1, 0, nullptr, nullptr)));
    hipLaunchKernelGGL(k_coh_upos, gK, dim3(256), 0, st, d_open, d_ox, K, d_upos);
    hipLaunchKernelGGL(k_coh_flags, gK, dim3(256), 0, st, d_f, K, d_open, d_ox, d_upos, O.dist);
    HIPCHK(hipGetLastError());
    int64_t tot[2];
    HIPCHK(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t M = tot[0], NS = tot[1];                    // M <= n, NS <= M
    // ---- the member and sample lists
    int32_t *d_members, *d_samples;
    TRY(ctx_buf_t(ctx, "coh_members", (size_t)M, &d_members));
    TRY(ctx_buf_t(ctx, "coh_samples", (size_t)NS, &d_samples));
    hipLaunchKernelGGL(k_coh_members, grid256(M), dim3(256), 0, st, d_moff, K, M, d_cl, d_cstart, d_ord, d_members);
    hipLaunchKernelGGL(k_coh_samples, grid256(NS), dim3(256), 0, st, d_soff, K, NS, d_cl, d_cstart, d_dx, d_dsamp, d_samples);
    HIPCHK(hipGetLastError());
    C->sites.resize((size_t)K); C->member_off.resize((size_t)K + 1); C->sample_off.resize((size_t)K + 1); C->members.resize((size_t)M); C->samples.resize((size_t)NS);
    HIPCHK(hipMemcpyAsync(C->sites.data(), d_f, (size_t)K * sizeof(telr_cohort_site), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C->member_off.data(), d_moff, ((size_t)K + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C->sample_off.data(), d_soff, ((size_t)K + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C->members.data(), d_members, (size_t)M * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C->samples.data(), d_samples, (size_t)NS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = guard.release();
    return TELR_OK;
}
