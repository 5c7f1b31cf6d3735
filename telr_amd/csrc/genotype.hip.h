// Genotypes of the insertion calls, on the device (include/telr_hip.h: telr_genotype_insertions).  Stands where the
// reference reads %AF, %GT and %DR out of Sniffles' VCF (src/telr/TELR_sv.py:161) -- with an own, fully specified definition, NOT
// Sniffles' genotyper: a read that is no supporter of a call and crosses it with a clean window (few indel bases inside pos +- flank)
// is a reference read, one that crosses it only with unclean windows is ambiguous; GT comes from alt / (alt + ref) in integers.
//
//   k_geno_span    one lane per eligible record: two binary searches in the calls' (tid, pos) keys give the calls it spans (a
//                  contiguous run of the ascending keys); counted, then scanned;
//   k_geno_pairs   one lane per (call, record) pair: its record from a binary search in the scanned counts, its call from its rank
//                  in the record's run -- a pair's place is a scan's, never an atomic's arrival order;
//   k_geno_window  one wave per pair, 64 CIGAR words per step (coalesced dwords), a wave prefix sum of the reference lengths
//                  carried from step to step, every lane adds its own op's share of the window, the wave leaves once a step starts
//                  past pos + flank; one sort key (call, read, unclean) per pair;
//   sort           radix.hip.h over the bits the three fields can hold: the clean pair of a (call, read) run sorts first, so the
//                  run's first pair is clean iff any is;
//   k_geno_flags   run heads that are no supporter (binary search in the call's read list) -> reference / ambiguous flags; two
//                  scans give the counts as differences at the calls' bounds (k_geno_cstart) and the places of the read lists.
#pragma once

struct GenoRec { int32_t qid, tid, ts, te, n_cigar, pad; int64_t cigar_off; };      // an eligible record

struct telr_ins_geno {
    std::vector<telr_ins_gt> gt;
    std::vector<int64_t> ref_off, ambig_off;
    std::vector<int32_t> ref_reads, ambig_reads;
};

static __host__ __device__ __forceinline__ int32_t geno_gt(int32_t alt, int32_t ref, int32_t het_pct, int32_t hom_pct)
{
    const int64_t a = 100LL * alt, n = (int64_t)alt + ref;
    return a >= hom_pct * n ? 2 : a >= het_pct * n ? 1 : 0;
}

// the calls record a spans: the keys in [(tid, ts + flank) -- (tid, 0) when ts is 0: the max(0, .) rule --, (tid, te - flank)]
__global__ void __launch_bounds__(256) k_geno_span(const GenoRec *__restrict__ recs, int32_t ne, const uint64_t *__restrict__ ckeys, int32_t ncall, int32_t flank,
                                                   int32_t *__restrict__ first, int32_t *__restrict__ cnt)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= ne) return;
    const GenoRec R = recs[a];
    const int64_t lo = R.ts == 0 ? 0 : (int64_t)R.ts + flank, hi = (int64_t)R.te - flank;
    int32_t f = 0, c = 0;
    if (hi >= lo && lo <= 0x7fffffffLL) d_span(ckeys, ncall, R.tid, lo, hi, &f, &c);
    first[a] = f; cnt[a] = c;
}

// off = exclusive scan of cnt (off[ne] = np): pair p belongs to the last record with off <= p
__global__ void __launch_bounds__(256) k_geno_pairs(const int64_t *__restrict__ off, int32_t ne, const int32_t *__restrict__ first, int64_t np,
                                                    int32_t *__restrict__ pcall, int32_t *__restrict__ prec)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const int32_t a = d_pair_owner(off, ne, p);
    prec[p] = a; pcall[p] = first[a] + (int32_t)(p - off[a]);
}

// the window indel of every pair -> its sort key ((call << qbits | read) << 1) | unclean
__global__ void __launch_bounds__(256) k_geno_window(const GenoRec *__restrict__ recs, const uint32_t *__restrict__ cig, const uint64_t *__restrict__ ckeys,
                                                     const int32_t *__restrict__ pcall, const int32_t *__restrict__ prec, int64_t np, int32_t flank,
                                                     int32_t max_indel, int qbits, uint64_t *__restrict__ keys)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (w >= np) return;
    const int32_t k = pcall[w];
    const GenoRec R = recs[prec[w]];
    const int64_t pos = (int64_t)(uint32_t)ckeys[k], wlo = pos - flank, whi = pos + flank;
    const uint32_t *__restrict__ c = cig + R.cigar_off;
    const int32_t n = R.n_cigar;
    int64_t rbase = R.ts, sum = 0;                        // rbase: the reference position of the step's first op (the same in every lane)
    uint32_t next = lane < n ? c[lane] : 0u;
    for (int32_t i0 = 0; i0 < n && rbase <= whi; i0 += 64) {
        const int32_t i = i0 + lane;
        const uint32_t word = next;
        next = i < n - 64 ? c[i + 64] : 0u;               // the next step's words are on their way while this step's are summed
        const int32_t op = (int32_t)(word & 15u);
        const int64_t len = (int64_t)(word >> 4), r = (op == 0 || op == 2) ? len : 0;
        const int64_t ri = d_wave_incl<int64_t>(r, lane), p = rbase + ri - r;
        if (op == 1) { if (wlo <= p && p <= whi) sum += len; }
        else if (op == 2) {
            const int64_t e = (p + len < whi ? p + len : whi) - (p > wlo ? p : wlo);
            if (e > 0) sum += e;
        }
        rbase += __shfl(ri, 63);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) keys[w] = ((((uint64_t)(uint32_t)k << qbits) | (uint32_t)R.qid) << 1) | (sum > max_indel ? 1u : 0u);
}

// over the sorted keys: rflag / aflag = the first pair of its (call, read) run, the read no supporter of the call, and the run
// clean / unclean; both with a trailing 0 for the scans
__global__ void __launch_bounds__(256) k_geno_flags(const uint64_t *__restrict__ keys, int64_t np, int qbits, const int64_t *__restrict__ read_off,
                                                    const int32_t *__restrict__ reads, int32_t *__restrict__ rflag, int32_t *__restrict__ aflag)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > np) return;
    int32_t rf = 0, af = 0;
    if (j < np) {
        const uint64_t key = keys[j];
        if (j == 0 || (keys[j - 1] >> 1) != (key >> 1)) {
            const int32_t q = (int32_t)((key >> 1) & ((1ULL << qbits) - 1ULL));
            const int64_t k = (int64_t)(key >> (qbits + 1));
            if (!d_in_list(reads, read_off[k], read_off[k + 1], q)) { if (key & 1ULL) af = 1; else rf = 1; }
        }
    }
    rflag[j] = rf; aflag[j] = af;
}
// cstart[k] = the first sorted pair of call k or a later one (cstart[ncall] = np)
__global__ void __launch_bounds__(256) k_geno_cstart(const uint64_t *__restrict__ keys, int64_t np, int qbits, int32_t ncall, int32_t *__restrict__ cstart)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > ncall) return;
    cstart[k] = k == ncall ? (int32_t)np : (int32_t)d_bound<false>(keys, np, (uint64_t)k << (qbits + 1));
}
__global__ void __launch_bounds__(256) k_geno_calls(const int32_t *__restrict__ cstart, int32_t ncall, const int32_t *__restrict__ rx, const int32_t *__restrict__ ax,
                                                    const int32_t *__restrict__ support, int32_t het_pct, int32_t hom_pct, telr_ins_gt *__restrict__ gt,
                                                    int64_t *__restrict__ ref_off, int64_t *__restrict__ ambig_off)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > ncall) return;
    const int32_t lo = cstart[k];
    ref_off[k] = rx[lo]; ambig_off[k] = ax[lo];          // the pairs are sorted by call: the lists of the calls lie back to back
    if (k == ncall) return;
    const int32_t hi = cstart[k + 1];
    telr_ins_gt g;
    g.ref = rx[hi] - rx[lo]; g.ambig = ax[hi] - ax[lo]; g.alt = support[k]; g.gt = geno_gt(g.alt, g.ref, het_pct, hom_pct);
    gt[k] = g;
}
__global__ void __launch_bounds__(256) k_geno_reads(const uint64_t *__restrict__ keys, int64_t np, int qbits, const int32_t *__restrict__ rflag, const int32_t *__restrict__ aflag,
                                                    const int32_t *__restrict__ rx, const int32_t *__restrict__ ax, int32_t *__restrict__ ref_reads, int32_t *__restrict__ ambig_reads)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const int32_t q = (int32_t)((keys[j] >> 1) & ((1ULL << qbits) - 1ULL));
    if (rflag[j]) ref_reads[rx[j]] = q;
    if (aflag[j]) ambig_reads[ax[j]] = q;
}

extern "C" void telr_geno_opt_default(telr_geno_opt *o)
{
    if (!o) return;
    o->flank = 50; o->min_mapq = 20; o->max_window_indel = 20; o->het_pct = 30; o->hom_pct = 80; o->reserved[0] = o->reserved[1] = o->reserved[2] = 0;
}
extern "C" int64_t telr_ins_geno_count(const telr_ins_geno *g) { return g ? (int64_t)g->gt.size() : 0; }
extern "C" const telr_ins_gt *telr_ins_geno_gt(const telr_ins_geno *g) { return g ? g->gt.data() : nullptr; }
extern "C" const int64_t *telr_ins_geno_ref_off(const telr_ins_geno *g) { return g ? g->ref_off.data() : nullptr; }
extern "C" const int32_t *telr_ins_geno_ref_reads(const telr_ins_geno *g) { return g ? g->ref_reads.data() : nullptr; }
extern "C" const int64_t *telr_ins_geno_ambig_off(const telr_ins_geno *g) { return g ? g->ambig_off.data() : nullptr; }
extern "C" const int32_t *telr_ins_geno_ambig_reads(const telr_ins_geno *g) { return g ? g->ambig_reads.data() : nullptr; }
extern "C" void telr_ins_geno_free(telr_ins_geno *g) { delete g; }

extern "C" int telr_genotype_insertions(telr_ctx *ctx, const telr_result *r, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls,
                                        const int64_t *read_off, const int32_t *reads, const telr_geno_opt *opt, telr_ins_geno **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    auto bad = [&](const std::string &why) { ctx->err = "telr_genotype_insertions: " + why; return TELR_E_ARG; };
    if (!r || !out) return bad("null result or output");
    if (n_targets <= 0) return bad("n_targets must be positive");
    if (n_calls < 0 || (n_calls > 0 && (!calls || !read_off))) return bad("null calls or read offsets");
    telr_geno_opt O;
    if (opt) O = *opt; else telr_geno_opt_default(&O);
    if (O.flank < 0 || O.min_mapq < 0 || O.max_window_indel < 0 || O.het_pct < 0 || O.hom_pct < 0 || O.reserved[0] < 0 || O.reserved[1] < 0 || O.reserved[2] < 0)
        return bad("negative option");
    if (O.het_pct > O.hom_pct) return bad("het_pct > hom_pct");
    if (O.hom_pct > 100) return bad("a percentage above 100");
    const size_t n = r->alns.size();
    if (n >= 0x7ffffff0u) { ctx->err = "telr_genotype_insertions: too many records"; return TELR_E_RANGE; }
    if (n_calls >= 0x7ffffff0LL) { ctx->err = "telr_genotype_insertions: too many calls"; return TELR_E_RANGE; }
    // the calls: 64-bit (tid, pos) keys, strictly ascending; the supporter lists ascending and distinct
    std::vector<uint64_t> ckeys((size_t)n_calls);
    std::vector<int32_t> support((size_t)n_calls);
    std::string why;
    if (!call_list_check(n_calls, calls, read_off, reads, n_targets, -1, ckeys.data(), support.data(), &why)) return bad(why);
    // the eligible records
    std::vector<GenoRec> er;
    int32_t max_qid = 0;
    for (size_t i = 0; i < n; ++i) {
        const telr_aln &a = r->alns[i];
        if (!record_check(a, i, n_targets, r->ncig, &why)) return bad(why);
        if ((a.flags & TELR_F_SECONDARY) || a.mapq < O.min_mapq) continue;
        GenoRec e;
        e.qid = a.qid; e.tid = a.tid; e.ts = a.ts; e.te = a.te; e.n_cigar = a.n_cigar; e.pad = 0; e.cigar_off = a.cigar_off;
        max_qid = std::max(max_qid, a.qid);
        er.push_back(e);
    }
    const size_t ne = er.size();
    telr_ins_geno *G = new telr_ins_geno();
    std::unique_ptr<telr_ins_geno> guard(G);
    G->gt.resize((size_t)n_calls); G->ref_off.assign((size_t)n_calls + 1, 0); G->ambig_off.assign((size_t)n_calls + 1, 0);
    for (int64_t k = 0; k < n_calls; ++k) { telr_ins_gt &g = G->gt[k]; g.ref = g.ambig = 0; g.alt = support[k]; g.gt = geno_gt(g.alt, 0, O.het_pct, O.hom_pct); }
    if (n_calls == 0 || ne == 0) { *out = guard.release(); return TELR_OK; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    result_wait(r);
    const int32_t nc = (int32_t)n_calls;
    GenoRec *d_rec; uint64_t *d_ckeys; int32_t *d_first, *d_cnt; int64_t *d_off, *d_tot;
    TRY(ctx_buf_t(ctx, "geno_rec", ne, &d_rec));
    TRY(ctx_buf_t(ctx, "geno_ckeys", (size_t)nc, &d_ckeys));
    TRY(ctx_buf_t(ctx, "geno_first", ne, &d_first));
    TRY(ctx_buf_t(ctx, "geno_cnt", ne + 1, &d_cnt));
    TRY(ctx_buf_t(ctx, "geno_off", ne + 1, &d_off));
    TRY(ctx_buf_t(ctx, "geno_tot", 4, &d_tot));
    HIPCHK(hipMemcpyAsync(d_rec, er.data(), ne * sizeof(GenoRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ckeys, ckeys.data(), (size_t)nc * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_geno_span, grid256((int64_t)ne), dim3(256), 0, st, d_rec, (int32_t)ne, d_ckeys, nc, O.flank, d_first, d_cnt);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int64_t>(ctx, d_cnt, (int32_t)ne, d_off, d_tot, 0, nullptr, nullptr)));
    int64_t tot[2];
    HIPCHK(hipMemcpyAsync(tot, d_tot, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t P = tot[0];
    if (P == 0) { *out = guard.release(); return TELR_OK; }
    if (P >= 0x7ffffff0LL) { ctx->err = "telr_genotype_insertions: too many (call, record) pairs"; return TELR_E_RANGE; }
    uint32_t *d_cig;
    TRY(result_dev_cigars(ctx, r, "geno_cig", true, &d_cig, nullptr));
    const int64_t nreads = read_off[n_calls];
    int32_t *d_pcall, *d_prec, *d_support, *d_reads; int64_t *d_roff; uint64_t *d_keys, *d_tkeys; uint32_t *d_hist;
    TRY(ctx_buf_t(ctx, "geno_pcall", (size_t)P, &d_pcall));
    TRY(ctx_buf_t(ctx, "geno_prec", (size_t)P, &d_prec));
    TRY(ctx_buf_t(ctx, "geno_support", (size_t)nc, &d_support));
    TRY(ctx_buf_t(ctx, "geno_reads", (size_t)nreads, &d_reads));
    TRY(ctx_buf_t(ctx, "geno_roff", (size_t)nc + 1, &d_roff));
    TRY(ctx_buf_t(ctx, "geno_keys", (size_t)P, &d_keys));
    TRY(ctx_buf_t(ctx, "geno_tkeys", (size_t)P, &d_tkeys));
    TRY(ctx_buf_t(ctx, "geno_hist", rs_hist_words((size_t)P), &d_hist));
    HIPCHK(hipMemcpyAsync(d_support, support.data(), (size_t)nc * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_roff, read_off, ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
    if (nreads) HIPCHK(hipMemcpyAsync(d_reads, reads, (size_t)nreads * 4, hipMemcpyHostToDevice, st));
    const int qb = std::max(1, bits_of((uint64_t)max_qid)), cb = bits_of((uint64_t)nc - 1);
    const dim3 gP = grid256(P), gP1 = grid256(P + 1), gC1 = grid256((int64_t)nc + 1);
    hipLaunchKernelGGL(k_geno_pairs, gP, dim3(256), 0, st, d_off, (int32_t)ne, d_first, P, d_pcall, d_prec);
    hipLaunchKernelGGL(k_geno_window, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, d_rec, d_cig, d_ckeys, d_pcall, d_prec, P, O.flank, O.max_window_indel, qb, d_keys);
    HIPCHK(hipGetLastError());
    // the distinct reads of every call: sort by (call, read, unclean)
    if (radix_sort_passes<uint64_t, false>(d_keys, nullptr, d_tkeys, nullptr, P, cb + qb + 1, d_hist, st)) std::swap(d_keys, d_tkeys);
    HIPCHK(hipGetLastError());
    int32_t *d_rflag, *d_aflag, *d_rx, *d_ax, *d_cstart;
    TRY(ctx_buf_t(ctx, "geno_rflag", (size_t)P + 1, &d_rflag));
    TRY(ctx_buf_t(ctx, "geno_aflag", (size_t)P + 1, &d_aflag));
    TRY(ctx_buf_t(ctx, "geno_rx", (size_t)P + 1, &d_rx));
    TRY(ctx_buf_t(ctx, "geno_ax", (size_t)P + 1, &d_ax));
    TRY(ctx_buf_t(ctx, "geno_cstart", (size_t)nc + 1, &d_cstart));
    hipLaunchKernelGGL(k_geno_flags, gP1, dim3(256), 0, st, d_keys, P, qb, d_roff, d_reads, d_rflag, d_aflag);
    hipLaunchKernelGGL(k_geno_cstart, gC1, dim3(256), 0, st, d_keys, P, qb, nc, d_cstart);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_rflag, (int32_t)P, d_rx, d_tot, 0, nullptr, nullptr)));
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_aflag, (int32_t)P, d_ax, d_tot + 1, 0, nullptr, nullptr)));
    HIPCHK(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t nref = tot[0], namb = tot[1];
    telr_ins_gt *d_gt; int64_t *d_refoff, *d_amboff; int32_t *d_refreads, *d_ambreads;
    TRY(ctx_buf_t(ctx, "geno_gt", (size_t)nc, &d_gt));
    TRY(ctx_buf_t(ctx, "geno_refoff", (size_t)nc + 1, &d_refoff));
    TRY(ctx_buf_t(ctx, "geno_amboff", (size_t)nc + 1, &d_amboff));
    TRY(ctx_buf_t(ctx, "geno_refreads", (size_t)nref, &d_refreads));
    TRY(ctx_buf_t(ctx, "geno_ambreads", (size_t)namb, &d_ambreads));
    hipLaunchKernelGGL(k_geno_calls, gC1, dim3(256), 0, st, d_cstart, nc, d_rx, d_ax, d_support, O.het_pct, O.hom_pct, d_gt, d_refoff, d_amboff);
    hipLaunchKernelGGL(k_geno_reads, gP, dim3(256), 0, st, d_keys, P, qb, d_rflag, d_aflag, d_rx, d_ax, d_refreads, d_ambreads);
    HIPCHK(hipGetLastError());
    G->ref_reads.resize((size_t)nref); G->ambig_reads.resize((size_t)namb);
    HIPCHK(hipMemcpyAsync(G->gt.data(), d_gt, (size_t)nc * sizeof(telr_ins_gt), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(G->ref_off.data(), d_refoff, ((size_t)nc + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(G->ambig_off.data(), d_amboff, ((size_t)nc + 1) * 8, hipMemcpyDeviceToHost, st));
    if (nref) HIPCHK(hipMemcpyAsync(G->ref_reads.data(), d_refreads, (size_t)nref * 4, hipMemcpyDeviceToHost, st));
    if (namb) HIPCHK(hipMemcpyAsync(G->ambig_reads.data(), d_ambreads, (size_t)namb * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = guard.release();
    return TELR_OK;
}
