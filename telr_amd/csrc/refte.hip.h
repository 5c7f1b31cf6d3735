// The reference's TE copies as features, from the records of a tile map, on the device (include/telr_hip.h:
// telr_annotate_hits).  Stands where the reference masks the reference genome with RepeatMasker and hands the BED to the liftover
// (src/telr/telr.py:132-159, TELR_te.py:391-469) -- with an own, fully specified definition, NOT RepeatMasker: the library is the index,
// the reference is cut into overlapping tiles (tile_plan.h) that are mapped to it as queries, and the records of that map become
// features by an interval rule.  tests/refte_ref.py states it in plain Python.
//
//   Hit      a record that is not TELR_F_SECONDARY, with mapq >= min_mapq and qe - qs >= min_len: tid = tiles[qid].tid,
//            start = tiles[qid].start + qs, end = tiles[qid].start + qe, family = rec.tid, strand = 1 on TELR_F_REV, score = dp_score.
//   Order    ascending by (tid, family, strand, start, end); equal keys are interchangeable.
//   Feature  inside a run of equal (tid, family, strand) hit i opens a new feature iff it is the run's first or
//            start_i >= M_i + join_gap, M_i = the maximum end of ALL earlier hits of the run.  Fields: the start of its first hit,
//            the maximum end, the maximum score, the number of hits.
//   Output   ascending by (tid, start, end, family, strand).
//
//   k_rt_elig     one lane per record: is it a hit (with a trailing 0 for the scan);
//   k_rt_hits     one lane per record: a hit is written at its scanned place, never at an atomic's arrival order;
//   sorts         LSD over the complete key with radix.hip.h (stable; a permutation is carried, the keys of a round are gathered
//                 through it): (start, end), then (tid, family, strand); for the features (family, strand), (start, end), then tid;
//   k_rt_runs     one lane per hit: run head flag and the hit's end, as the two arrays the scan takes;
//   k_rt_segmax_* the segmented running maximum: out[i] = the maximum of val over [the last head at or before i, i].  A tile of 4,096
//                 values per workgroup, sixteen consecutive ones per lane; the lanes' (head seen, maximum) pairs are scanned in the wave
//                 with __shfl_up, the four waves' totals go through LDS; k_rt_segmax_sums leaves every tile's pair, k_rt_segmax_write
//                 finds its tile's carry among the pairs of the tiles before it (from the last one that holds a head on) and lays it over
//                 the values before the tile's first head -- as k_qscan_sums / k_qscan_write do for sums.  The one place where an answer
//                 depends on an element arbitrarily far to the left; run over the runs for `end` and over the features for `score`;
//   k_rt_fheads   one lane per hit: feature head flag from the scanned maximum before it; scanned to feature ids;
//   k_rt_fstart   the features' first hits (compaction by the scanned flags);
//   k_rt_feats    one lane per feature: end, score and n_hits from the scanned values at its bounds.
// Stores are plain vector stores at the lane's own index or at a scanned place; there is no atomic; no CIGAR is read.
#pragma once
#include "tile_plan.h"

struct RtHit { int32_t tid, start, end, family, strand, score; };      // the first five fields as telr_te_feat has them: one set of key functors

struct telr_te_feats { std::vector<telr_te_feat> f; };

#define RT_TILE 4096
#define RT_IPT (RT_TILE / 256)
#define RT_NONE INT32_MIN

__global__ void __launch_bounds__(256) k_rt_elig(const telr_aln *__restrict__ alns, int64_t n, int32_t min_len, int32_t min_mapq, int32_t *__restrict__ elig)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { elig[i] = 0; return; }
    const telr_aln a = alns[i];
    elig[i] = (!(a.flags & TELR_F_SECONDARY) && a.mapq >= min_mapq && a.qe - a.qs >= min_len) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_rt_hits(const telr_aln *__restrict__ alns, int64_t n, const telr_tile *__restrict__ tiles, const int32_t *__restrict__ elig,
                                                 const int32_t *__restrict__ off, RtHit *__restrict__ hits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !elig[i]) return;
    const telr_aln a = alns[i];
    const telr_tile t = tiles[a.qid];
    RtHit h;
    h.tid = t.tid; h.start = t.start + a.qs; h.end = t.start + a.qe; h.family = a.tid; h.strand = (a.flags & TELR_F_REV) ? 1 : 0; h.score = a.dp_score;
    hits[off[i]] = h;
}

// the keys of the sort rounds (stage2_common.hip.h: perm_sort_round), of a hit or of a feature; cb / fb: the bits of a coordinate / a family index
struct RtKeySE  { int cb; template <typename T> __device__ uint64_t operator()(const T &s, uint32_t) const { return ((uint64_t)(uint32_t)s.start << cb) | (uint32_t)s.end; } };
struct RtKeyTFS { int fb; template <typename T> __device__ uint64_t operator()(const T &s, uint32_t) const { return ((((uint64_t)(uint32_t)s.tid << fb) | (uint32_t)s.family) << 1) | (uint32_t)s.strand; } };
struct RtKeyFS  { template <typename T> __device__ uint64_t operator()(const T &s, uint32_t) const { return ((uint64_t)(uint32_t)s.family << 1) | (uint32_t)s.strand; } };
struct RtKeyT   { template <typename T> __device__ uint64_t operator()(const T &s, uint32_t) const { return (uint32_t)s.tid; } };

// over the sorted hits: head[i] = hit i is the first of its (tid, family, strand) run; end[i], score[i] = its fields
__global__ void __launch_bounds__(256) k_rt_runs(const RtHit *__restrict__ hits, int64_t n, int32_t *__restrict__ head, int32_t *__restrict__ end, int32_t *__restrict__ score)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RtHit h = hits[i];
    int32_t f = 1;
    if (i > 0) { const RtHit p = hits[i - 1]; f = (p.tid != h.tid || p.family != h.family || p.strand != h.strand) ? 1 : 0; }
    head[i] = f; end[i] = h.end; score[i] = h.score;
}

// (head seen, maximum since the last head) pairs: x before y
template <typename T> struct RtSeg { int32_t f; T m; };
template <typename T> static __device__ __forceinline__ RtSeg<T> rt_join(const RtSeg<T> x, const RtSeg<T> y)
{
    RtSeg<T> r; r.f = x.f | y.f; r.m = y.f ? y.m : (x.m > y.m ? x.m : y.m);
    return r;
}
// The tile's scan.  v[j] = the inclusive segmented maximum of the lane's own sixteen values on their own, own = the lane's pair;
// returns the pair of everything of the tile before the lane (f = 0, m = none for the tile's first lane); *total (every lane) = the tile's pair.
// A kernel calls it once: its LDS pairs are written once.
template <typename T>
static __device__ __forceinline__ RtSeg<T> rt_tile_scan(const int32_t *__restrict__ head, const T *__restrict__ val, int64_t n, int64_t lo, T none,
                                                        int32_t (&f)[RT_IPT], T (&v)[RT_IPT], RtSeg<T> *total)
{
    __shared__ int32_t wf[4];
    __shared__ T wm[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    RtSeg<T> own; own.f = 0; own.m = none;
#pragma unroll
    for (int j = 0; j < RT_IPT; ++j) {
        const bool in = lo + j < n;
        RtSeg<T> e; e.f = in ? head[lo + j] : 0; e.m = in ? val[lo + j] : none;
        own = rt_join(own, e);
        f[j] = e.f; v[j] = own.m;
    }
    RtSeg<T> inc = own;                                   // inclusive over the wave's lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        RtSeg<T> x; x.f = __shfl_up(inc.f, o); x.m = __shfl_up(inc.m, o);
        if (lane >= o) inc = rt_join(x, inc);
    }
    if (lane == 63) { wf[wv] = inc.f; wm[wv] = inc.m; }
    RtSeg<T> before; before.f = __shfl_up(inc.f, 1); before.m = __shfl_up(inc.m, 1);
    if (lane == 0) { before.f = 0; before.m = none; }
    __syncthreads();
    RtSeg<T> pre; pre.f = 0; pre.m = none;
    RtSeg<T> all = pre;
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        RtSeg<T> w; w.f = wf[z]; w.m = wm[z];
        if (z < wv) pre = rt_join(pre, w);
        all = rt_join(all, w);
    }
    *total = all;
    return rt_join(pre, before);
}

template <typename T>
__global__ void __launch_bounds__(256) k_rt_segmax_sums(const int32_t *__restrict__ head, const T *__restrict__ val, int64_t n, T none,
                                                        int32_t *__restrict__ tile_f, T *__restrict__ tile_m)
{
    int32_t f[RT_IPT]; T v[RT_IPT];
    RtSeg<T> total;
    (void)rt_tile_scan<T>(head, val, n, (int64_t)blockIdx.x * RT_TILE + threadIdx.x * RT_IPT, none, f, v, &total);
    if (threadIdx.x == 0) { tile_f[blockIdx.x] = total.f; tile_m[blockIdx.x] = total.m; }
}
template <typename T>
__global__ void __launch_bounds__(256) k_rt_segmax_write(const int32_t *__restrict__ head, const T *__restrict__ val, int64_t n, T none,
                                                         const int32_t *__restrict__ tile_f, const T *__restrict__ tile_m, T *__restrict__ out)
{
    __shared__ int32_t sj[256];
    __shared__ T sm[256];
    const int tid = threadIdx.x, b = (int)blockIdx.x;
    // the carry into this tile: the maximum over the tiles from the last one before it that holds a head (its pair's maximum is the one
    // behind its last head) up to the tile before this one
    int32_t j = -1;
    for (int t = tid; t < b; t += 256) if (tile_f[t]) j = t;      // (ascending: the lane's last)
    sj[tid] = j;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) { if (tid < o && sj[tid + o] > sj[tid]) sj[tid] = sj[tid + o]; __syncthreads(); }
    const int32_t from = sj[0] > 0 ? sj[0] : 0;
    T c = none;
    for (int t = from + tid; t < b; t += 256) { const T x = tile_m[t]; if (x > c) c = x; }
    sm[tid] = c;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) { if (tid < o && sm[tid + o] > sm[tid]) sm[tid] = sm[tid + o]; __syncthreads(); }
    RtSeg<T> carry; carry.f = 0; carry.m = sm[0];
    int32_t f[RT_IPT]; T v[RT_IPT];
    RtSeg<T> total;
    const int64_t lo = (int64_t)b * RT_TILE + tid * RT_IPT;
    RtSeg<T> pre = rt_join(carry, rt_tile_scan<T>(head, val, n, lo, none, f, v, &total));
    int32_t seen = 0;                                     // a head among the lane's own values so far
#pragma unroll
    for (int j2 = 0; j2 < RT_IPT; ++j2) {
        seen |= f[j2];
        if (lo + j2 < n) out[lo + j2] = (!seen && pre.m > v[j2]) ? pre.m : v[j2];
    }
}

// fh[i] = hit i opens a feature: its run's first, or start_i >= (the maximum end of the run's earlier hits) + join_gap; trailing 0
__global__ void __launch_bounds__(256) k_rt_fheads(const RtHit *__restrict__ hits, int64_t n, const int32_t *__restrict__ head, const int32_t *__restrict__ emax,
                                                   int32_t join_gap, int32_t *__restrict__ fh)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { fh[i] = 0; return; }
    int32_t f = head[i];                                  // (head[0] is set: emax[-1] is never read)
    if (!f) f = (int64_t)hits[i].start >= (int64_t)emax[i - 1] + join_gap ? 1 : 0;
    fh[i] = f;
}
// fx = exclusive scan of fh (fx[n] = features): the features' first hits, fstart[features] = n
__global__ void __launch_bounds__(256) k_rt_fstart(const int32_t *__restrict__ fh, const int32_t *__restrict__ fx, int64_t n, int32_t *__restrict__ fstart)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { fstart[fx[n]] = (int32_t)n; return; }
    if (fh[i]) fstart[fx[i]] = (int32_t)i;
}
__global__ void __launch_bounds__(256) k_rt_feats(const RtHit *__restrict__ hits, const int32_t *__restrict__ fstart, int32_t nf, const int32_t *__restrict__ emax,
                                                  const int32_t *__restrict__ smax, telr_te_feat *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nf) return;
    const int32_t lo = fstart[k], hi = fstart[k + 1];
    const RtHit h = hits[lo];
    telr_te_feat o;
    // the run's maximum at the feature's last hit is the feature's own: every earlier end of the run is <= the feature's start
    o.tid = h.tid; o.start = h.start; o.end = emax[hi - 1]; o.family = h.family; o.strand = h.strand; o.score = smax[hi - 1]; o.n_hits = hi - lo;
    out[k] = o;
}

// out[i] = max of val over [the last i' <= i with head[i'], i] (head[0] counts as set), n >= 1
template <typename T>
static int rt_segmax(telr_ctx *ctx, const int32_t *head, const T *val, int64_t n, T none, T *out)
{
    const int ntile = (int)((n + RT_TILE - 1) / RT_TILE);
    int32_t *d_tf; T *d_tm;
    TRY(ctx_buf_t(ctx, "rt_tile_f", (size_t)ntile, &d_tf));
    TRY(ctx_buf_t(ctx, "rt_tile_m", (size_t)ntile, &d_tm));
    hipLaunchKernelGGL((k_rt_segmax_sums<T>), dim3(ntile), dim3(256), 0, ctx->stream, head, val, n, none, d_tf, d_tm);
    hipLaunchKernelGGL((k_rt_segmax_write<T>), dim3(ntile), dim3(256), 0, ctx->stream, head, val, n, none, d_tf, d_tm, out);
    HIPCHK(hipGetLastError());
    return TELR_OK;
}

extern "C" int telr_tile_plan(int32_t n_targets, const int32_t *target_len, int32_t tile, int32_t stride, telr_tile *out, int64_t cap, int64_t *needed)
{
    return tile_plan(n_targets, target_len, tile, stride, out, cap, needed);
}
extern "C" void telr_refte_opt_default(telr_refte_opt *o)
{
    if (!o) return;
    o->min_len = 100; o->min_mapq = 0; o->join_gap = 0; o->reserved = 0;
}
extern "C" int64_t telr_te_feats_count(const telr_te_feats *f) { return f ? (int64_t)f->f.size() : 0; }
extern "C" const telr_te_feat *telr_te_feats_data(const telr_te_feats *f) { return f ? f->f.data() : nullptr; }
extern "C" void telr_te_feats_free(telr_te_feats *f) { delete f; }

extern "C" int telr_annotate_hits(telr_ctx *ctx, const telr_result *r, int64_t n_tiles, const telr_tile *tiles, int32_t n_targets, const int32_t *target_len,
                                  int32_t n_families, const telr_refte_opt *opt, telr_te_feats **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    if (!r || !out) { ctx->err = "telr_annotate_hits: null result or output"; return TELR_E_ARG; }
    telr_refte_opt O;
    if (opt) O = *opt; else telr_refte_opt_default(&O);
    const int64_t n = (int64_t)r->alns.size();
    int32_t max_end = 0;
    std::string why;
    const int chk = refte_check(r->alns.data(), n, n_tiles, tiles, n_targets, target_len, n_families, &O, &max_end, &why);
    if (chk != TELR_OK) { ctx->err = "telr_annotate_hits: " + why; return chk; }
    telr_te_feats *F = new telr_te_feats();
    std::unique_ptr<telr_te_feats> guard(F);
    if (n == 0) { *out = guard.release(); return TELR_OK; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the hits: eligibility, its scan, the write
    telr_aln *d_aln; telr_tile *d_tiles; int32_t *d_elig, *d_off;
    TRY(ctx_buf_t(ctx, "rt_aln", (size_t)n, &d_aln));
    TRY(ctx_buf_t(ctx, "rt_tiles", (size_t)n_tiles, &d_tiles));
    TRY(ctx_buf_t(ctx, "rt_elig", (size_t)n + 1, &d_elig));
    TRY(ctx_buf_t(ctx, "rt_off", (size_t)n + 1, &d_off));
    HIPCHK(hipMemcpyAsync(d_aln, r->alns.data(), (size_t)n * sizeof(telr_aln), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tiles, tiles, (size_t)n_tiles * sizeof(telr_tile), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rt_elig, grid256(n + 1), dim3(256), 0, st, d_aln, n, O.min_len, O.min_mapq, d_elig);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_elig, (int32_t)n, d_off, nullptr, 0, nullptr, nullptr)));
    int32_t nh = 0;
    HIPCHK(hipMemcpyAsync(&nh, d_off + n, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nh == 0) { *out = guard.release(); return TELR_OK; }
    const int64_t N = nh;
    RtHit *d_raw, *d_hit;
    TRY(ctx_buf_t(ctx, "rt_raw", (size_t)N, &d_raw));
    TRY(ctx_buf_t(ctx, "rt_hit", (size_t)N, &d_hit));
    hipLaunchKernelGGL(k_rt_hits, grid256(n), dim3(256), 0, st, d_aln, n, d_tiles, d_elig, d_off, d_raw);
    // sort by (tid, family, strand, start, end): least significant group first
    PermSort S;
    TRY(S.alloc(ctx, "rt_", (size_t)N));
    const int cb = bits_of((uint64_t)max_end), fb = bits_of((uint64_t)(n_families > 0 ? n_families - 1 : 0)), tb = bits_of((uint64_t)(n_targets > 0 ? n_targets - 1 : 0));
    const dim3 gN = grid256(N), gN1 = grid256(N + 1);
    perm_iota(ctx, S, N);
    TRY(perm_sort_round(ctx, S, d_raw, N, RtKeySE{cb}, 2 * cb));
    TRY(perm_sort_round(ctx, S, d_raw, N, RtKeyTFS{fb}, tb + fb + 1));
    perm_gather(ctx, S, d_raw, N, d_hit);
    // the running maximum of end over the runs, the feature heads, their scan
    int32_t *d_head, *d_end, *d_score, *d_emax, *d_smax, *d_fh, *d_fx, *d_fstart;
    TRY(ctx_buf_t(ctx, "rt_head", (size_t)N, &d_head));
    TRY(ctx_buf_t(ctx, "rt_end", (size_t)N, &d_end));
    TRY(ctx_buf_t(ctx, "rt_score", (size_t)N, &d_score));
    TRY(ctx_buf_t(ctx, "rt_emax", (size_t)N, &d_emax));
    TRY(ctx_buf_t(ctx, "rt_smax", (size_t)N, &d_smax));
    TRY(ctx_buf_t(ctx, "rt_fh", (size_t)N + 1, &d_fh));
    TRY(ctx_buf_t(ctx, "rt_fx", (size_t)N + 1, &d_fx));
    TRY(ctx_buf_t(ctx, "rt_fstart", (size_t)N + 1, &d_fstart));
    hipLaunchKernelGGL(k_rt_runs, gN, dim3(256), 0, st, d_hit, N, d_head, d_end, d_score);
    HIPCHK(hipGetLastError());
    TRY(rt_segmax<int32_t>(ctx, d_head, d_end, N, RT_NONE, d_emax));
    hipLaunchKernelGGL(k_rt_fheads, gN1, dim3(256), 0, st, d_hit, N, d_head, d_emax, O.join_gap, d_fh);
    HIPCHK(hipGetLastError());
    TRY((dev_qscan<int32_t, int32_t>(ctx, d_fh, (int32_t)N, d_fx, nullptr, 0, nullptr, nullptr)));
    hipLaunchKernelGGL(k_rt_fstart, gN1, dim3(256), 0, st, d_fh, d_fx, N, d_fstart);
    HIPCHK(hipGetLastError());
    TRY(rt_segmax<int32_t>(ctx, d_fh, d_score, N, RT_NONE, d_smax));      // the same scan over the feature segments
    int32_t nf = 0;
    HIPCHK(hipMemcpyAsync(&nf, d_fx + N, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the features, then their order
    telr_te_feat *d_fraw, *d_feat;
    TRY(ctx_buf_t(ctx, "rt_fraw", (size_t)nf, &d_fraw));
    TRY(ctx_buf_t(ctx, "rt_feat", (size_t)nf, &d_feat));
    const dim3 gF = grid256((int64_t)nf);
    hipLaunchKernelGGL(k_rt_feats, gF, dim3(256), 0, st, d_hit, d_fstart, nf, d_emax, d_smax, d_fraw);
    perm_iota(ctx, S, nf);
    TRY(perm_sort_round(ctx, S, d_fraw, nf, RtKeyFS{}, fb + 1));
    TRY(perm_sort_round(ctx, S, d_fraw, nf, RtKeySE{cb}, 2 * cb));
    TRY(perm_sort_round(ctx, S, d_fraw, nf, RtKeyT{}, tb));
    perm_gather(ctx, S, d_fraw, nf, d_feat);
    HIPCHK(hipGetLastError());
    F->f.resize((size_t)nf);
    HIPCHK(hipMemcpyAsync(F->f.data(), d_feat, (size_t)nf * sizeof(telr_te_feat), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = guard.release();
    return TELR_OK;
}
