// A bridge of two reads per insertion call that no single read spans (include/telr_hip.h: telr_bridge_contigs, where the
// definition stands; tests/bridge_ref.py restates it in plain Python).  A sibling of draft.hip.h: where every supporting read runs from one
// flank into the element and ends there, a call has clip signatures only and no draft.  A read that enters from the left and one that
// enters from the right are joined at ONE shared k-mer of their clips.  An own, fully specified definition that is NOT an assembler and
// NOT wtdbg2 or flye: no consensus is formed, polishing follows as it follows a draft.  Records only: telr_seqset_join makes the sequences.
//
//   CutInput         (stage2_common.hip.h) the input, its refusals and its uploads are those of telr_draft_contigs; its k_cut_span here
//                    counts the clips (kind 2): the (signature, call) pairs, and which clips lie within `reach` of a call at all;
//   k_bridge_cand   one wave per such clip: the one-coordinate walk of draft_walk (stage2_common.hip.h) -- lo_a(xL) of a tail clip,
//                    hi_b(xR) of a head clip; a candidate's validity, clip length and flank do not depend on the call;
//   k_bridge_top     one wave per call: the clips within `reach` of it are a contiguous run of the sorted signature array; the valid
//                    ones of its own reads counted, then the first `pairs` of each side by repeated butterfly minima over the total
//                    order (-clip, -flank, qid, rec, index): each round takes the smallest key behind the last one taken;
//   k_bridge_vote    one workgroup per (call, left rank, right rank) -- the hot kernel.  The window (the last min(window, cL) bases of the
//                    left clip) sits in LDS as packed words and mask bits; its N-free k-mers go into an open-addressed LDS table of 8,192
//                    slots (position + 1, bit 31 = the value occurs again; equality is tested against the window itself, so a slot needs
//                    no key; a second insert of a value only sets the flag, so the usable set does not depend on the order of the
//                    inserts).  V is streamed from the packed words in chunks of 4,096 start positions, 16 per lane from two funnel-
//                    shifted words (a rolling k-mer), whatever its length.  Matches add to integer LDS bin counters (order-independent);
//                    2,048 bins are held at a time, a longer diagonal range is taken in passes that overlap by one bin, each pass
//                    streaming only the part of V that can reach its bins.  Then V's part that can reach the band is streamed again and
//                    the band matches are ranked by a running workgroup prefix count to the lower median;
//   k_bridge_pick    one lane per call: the pair of the most votes (ties: the smaller left rank, then the smaller right rank), the
//                    thresholds, the record.
// No atomic decides an output position; the output is the same on every run.  Both strands go through d_strand16 and cost the same.
#pragma once

#define BR_SLOTS 8192            /* table slots: 32 KB; at most 4,096 - k + 1 entries, so never more than half full */
#define BR_NBIN 2048             /* diagonal bins of 128 held at a time: 8 KB */
#define BR_WWORDS (4096 / 16 + 2)
#define BR_CHUNK 4096            /* start positions of V per step: 16 per lane */
#define BR_MAX_PAIRS 8

struct BridgeCand { int32_t valid, clip, fl, x; };                                             // x = lo_a(xL) of a left, hi_b(xR) of a right candidate
struct BridgeTop { int32_t sl[BR_MAX_PAIRS], sr[BR_MAX_PAIRS], nl, nr; };                       // the kept signatures by rank (-1: none), the valid counts
struct BridgeVote { int32_t votes, i, j; };                                                    // votes -1: the pair is not voted

struct telr_bridges { std::vector<telr_bridge> d; };

__global__ void __launch_bounds__(256) k_bridge_cand(const telr_ins_sig *__restrict__ sigs, int32_t ns, const int32_t *__restrict__ cnt, const CutRec *__restrict__ recs,
                                                     const uint32_t *__restrict__ cig, int32_t flank, int32_t min_flank, int32_t k,
                                                     BridgeCand *__restrict__ candl, BridgeCand *__restrict__ candr)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (w >= ns) return;
    BridgeCand L, R;
    L.valid = 0; L.clip = 0; L.fl = 0; L.x = 0; R = L;
    const telr_ins_sig s = sigs[w];
    if (s.kind == 2 && cnt[w] > 0) {                      // (the same in every lane of the wave)
        const CutRec A = recs[s.rec];
        int64_t lo = 0, hi = 0; bool flo = false, fhi = false;
        if (s.pos == A.te) {                              // a tail clip: the read goes on to the right of the reference position
            const int64_t xL = (int64_t)s.pos - flank > A.ts ? (int64_t)s.pos - flank : (int64_t)A.ts;
            const int32_t cL = A.qlen - A.qe;
            if (A.n_cigar > 0 && s.pos - xL >= min_flank && cL >= k) {
                draft_walk<true, false>(cig + A.cigar_off, A.n_cigar, A.ts, A.qs, xL, xL, lane, lo, flo, hi, fhi);
                if (flo && lo >= 0) { L.valid = 1; L.clip = cL; L.fl = (int32_t)(s.pos - xL); L.x = (int32_t)lo; }
            }
        }
        if (s.pos == A.ts) {                              // a head clip
            const int64_t xR = (int64_t)s.pos + flank < A.te ? (int64_t)s.pos + flank : (int64_t)A.te;
            const int32_t cR = A.qs;
            if (A.n_cigar > 0 && xR - s.pos >= min_flank && cR >= k) {
                draft_walk<false, true>(cig + A.cigar_off, A.n_cigar, A.ts, A.qs, xR, xR, lane, lo, flo, hi, fhi);
                if (fhi && hi <= A.qlen) { R.valid = 1; R.clip = cR; R.fl = (int32_t)(xR - s.pos); R.x = (int32_t)hi; }
            }
        }
    }
    if (lane == 0) { candl[w] = L; candr[w] = R; }
}

struct BridgeKey { int32_t has, clip, fl, qid, rec, j; };
static __device__ __forceinline__ bool bridge_before(const BridgeKey &x, const BridgeKey &y)      // x before y in (-clip, -fl, qid, rec, j); none is last
{
    if (x.has != y.has) return x.has > y.has;
    if (x.clip != y.clip) return x.clip > y.clip;
    if (x.fl != y.fl) return x.fl > y.fl;
    if (x.qid != y.qid) return x.qid < y.qid;
    if (x.rec != y.rec) return x.rec < y.rec;
    return x.j < y.j;
}

// the valid candidates of one side among signatures [s0, s1) whose read is a supporter (reads[r0 .. r1)): their count, and the first
// `pairs` of them in the total order into top[0 .. pairs) (-1 behind the last one).  One wave; every lane returns the same.
static __device__ __forceinline__ int32_t bridge_top_side(const telr_ins_sig *__restrict__ sigs, int32_t s0, int32_t s1, const BridgeCand *__restrict__ cand,
                                                          const int32_t *__restrict__ reads, int64_t r0, int64_t r1, int32_t pairs, int lane, int32_t *top)
{
    int32_t n = 0;
    BridgeKey prev; prev.has = 0; prev.clip = 0; prev.fl = 0; prev.qid = 0; prev.rec = 0; prev.j = 0;
    for (int32_t rank = 0; rank < pairs; ++rank) {
        BridgeKey best; best.has = 0; best.clip = 0; best.fl = 0; best.qid = 0; best.rec = 0; best.j = 0;
        for (int32_t j = s0 + lane; j < s1; j += 64) {
            const BridgeCand c = cand[j];
            if (!c.valid) continue;
            const telr_ins_sig s = sigs[j];
            if (!d_in_list(reads, r0, r1, s.qid)) continue;
            if (rank == 0) ++n;
            BridgeKey x; x.has = 1; x.clip = c.clip; x.fl = c.fl; x.qid = s.qid; x.rec = s.rec; x.j = j;
            if (prev.has && !bridge_before(prev, x)) continue;      // taken in an earlier round (keys are distinct: j closes them)
            if (bridge_before(x, best)) best = x;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            BridgeKey y;
            y.has = __shfl_xor(best.has, o); y.clip = __shfl_xor(best.clip, o); y.fl = __shfl_xor(best.fl, o); y.qid = __shfl_xor(best.qid, o);
            y.rec = __shfl_xor(best.rec, o); y.j = __shfl_xor(best.j, o);
            if (bridge_before(y, best)) best = y;
        }
        if (lane == 0) top[rank] = best.has ? best.j : -1;
        if (rank == 0) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
        }
        prev = best;
        if (!best.has) { if (lane == 0) for (int32_t q = rank + 1; q < pairs; ++q) top[q] = -1; break; }
    }
    return n;
}

__global__ void __launch_bounds__(256) k_bridge_top(const telr_ins_sig *__restrict__ sigs, int32_t ns, const telr_ins_call *__restrict__ calls, int32_t ncall,
                                                    const BridgeCand *__restrict__ candl, const BridgeCand *__restrict__ candr, const int64_t *__restrict__ read_off,
                                                    const int32_t *__restrict__ reads, int32_t reach, int32_t pairs, BridgeTop *__restrict__ top)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (k >= ncall) return;
    const telr_ins_call c = calls[k];
    int32_t s0, s1;
    d_sig_window(sigs, ns, c, reach, &s0, &s1);
    BridgeTop *T = top + k;
    if (lane == 0) for (int q = 0; q < BR_MAX_PAIRS; ++q) { T->sl[q] = -1; T->sr[q] = -1; }
    const int32_t nl = bridge_top_side(sigs, s0, s1, candl, reads, read_off[k], read_off[k + 1], pairs, lane, T->sl);
    const int32_t nr = bridge_top_side(sigs, s0, s1, candr, reads, read_off[k], read_off[k + 1], pairs, lane, T->sr);
    if (lane == 0) { T->nl = nl; T->nr = nr; }
}

// the k-mer at window base x (x + k <= the window's bases): false when one of its bases is an N
static __device__ __forceinline__ bool bridge_wkmer(const uint32_t *wc, const uint32_t *wm, int32_t x, uint32_t kmask, uint32_t km1, uint32_t &v)
{
    const int w = x >> 4, sh = x & 15;
    const uint64_t c = ((uint64_t)wc[w + 1] << 32) | wc[w];
    const uint32_t m = (wm[w + 1] << 16) | wm[w];
    v = (uint32_t)(c >> (2 * sh)) & kmask;
    return ((m >> sh) & km1) == 0;
}
static __device__ __forceinline__ uint32_t bridge_hash(uint32_t v) { return (v * 2654435761u) >> 19; }      // 13 bits: BR_SLOTS
// is v a usable k-mer of the window, and where
static __device__ __forceinline__ bool bridge_lookup(const uint32_t *slot, const uint32_t *wc, const uint32_t *wm, uint32_t v, uint32_t kmask, uint32_t km1, int32_t &x)
{
    for (uint32_t h = bridge_hash(v);; h = (h + 1) & (BR_SLOTS - 1)) {
        const uint32_t cur = slot[h];
        if (!cur) return false;
        const int32_t pos = (int32_t)(cur & 0x7fffffffu) - 1;
        uint32_t v2;
        bridge_wkmer(wc, wm, pos, kmask, km1, v2);
        if (v2 == v) { x = pos; return !(cur >> 31); }
    }
}

// The 16 start positions jb .. jb + 15 of V that a lane holds (those <= jmax count): 32 bases from two funnel-shifted words.  f(i, j) is
// called for every match in ascending j, i as an offset in U.
template <typename F>
static __device__ __forceinline__ void bridge_group(const uint32_t *__restrict__ par2, const uint32_t *__restrict__ parn, int64_t srcB, int32_t qlenB, int revB,
                                                    int64_t jb, int64_t jmax, const uint32_t *slot, const uint32_t *wc, const uint32_t *wm, int k, uint32_t kmask,
                                                    uint32_t km1, int32_t ilo, F f)
{
    if (jb > jmax) return;
    uint32_t c0, m0, c1 = 0, m1 = 0xffffu;
    d_strand16(par2, parn, srcB, qlenB, revB, jb, c0, m0);                        // jb <= jmax < qlen
    if (jb + 16 < qlenB) d_strand16(par2, parn, srcB, qlenB, revB, jb + 16, c1, m1);
    const uint64_t code = ((uint64_t)c1 << 32) | c0;
    const uint32_t mask = (m1 << 16) | m0;
    for (int r = 0; r < 16 && jb + r <= jmax; ++r) {
        if ((mask >> r) & km1) continue;
        int32_t x;
        if (bridge_lookup(slot, wc, wm, (uint32_t)(code >> (2 * r)) & kmask, kmask, km1, x)) f(ilo + x, (int32_t)(jb + r));
    }
}

__global__ void __launch_bounds__(256) k_bridge_vote(const uint32_t *__restrict__ par2, const uint32_t *__restrict__ parn, const int64_t *__restrict__ sboff,
                                                     const telr_ins_sig *__restrict__ sigs, const CutRec *__restrict__ recs, const BridgeTop *__restrict__ top,
                                                     const uint8_t *__restrict__ want, int32_t pairs, int32_t k, int32_t window, BridgeVote *__restrict__ out)
{
    __shared__ uint32_t wc[BR_WWORDS], wm[BR_WWORDS];
    __shared__ uint32_t slot[BR_SLOTS];
    __shared__ int32_t bins[BR_NBIN];
    __shared__ unsigned long long red[4];
    __shared__ int32_t part[4], found[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int32_t pp = pairs * pairs, kc = (int32_t)(blockIdx.x / (unsigned)pp), sl = (int32_t)(blockIdx.x % (unsigned)pp);
    const int32_t jl = top[kc].sl[sl / pairs], jr = top[kc].sr[sl % pairs];
    BridgeVote res; res.votes = -1; res.i = 0; res.j = 0;
    bool go = (!want || want[kc]) && jl >= 0 && jr >= 0;                          // (everything up to the first barrier is the same in every lane)
    if (go) go = sigs[jl].qid != sigs[jr].qid;
    if (!go) { if (tid == 0) out[blockIdx.x] = res; return; }
    const telr_ins_sig SL = sigs[jl], SR = sigs[jr];
    const CutRec A = recs[SL.rec], B = recs[SR.rec];
    const int32_t cL = A.qlen - A.qe, cR = B.qs;                                  // both >= k: the candidates are valid
    const int32_t Wn = window < cL ? window : cL, ilo = cL - Wn;
    const int64_t srcA = sboff[SL.qid], srcB = sboff[SR.qid], t0 = (int64_t)A.qlen - Wn;      // the window = the read's last Wn strand bases
    const uint32_t kmask = (1u << (2 * k)) - 1u, km1 = (1u << k) - 1u;
    const int nww = (Wn + 15) >> 4;
    for (int w = tid; w < BR_WWORDS; w += 256) {
        uint32_t c = 0, m = 0xffffu;
        if (w < nww) {
            d_strand16(par2, parn, srcA, A.qlen, A.rev, t0 + 16 * w, c, m);
            const int left = Wn - 16 * w;
            if (left < 16) m |= 0xffffu & ~((1u << left) - 1u);                   // behind the read's end: as N
        }
        wc[w] = c; wm[w] = m;
    }
    for (int s = tid; s < BR_SLOTS; s += 256) slot[s] = 0u;
    __syncthreads();
    for (int32_t x = tid; x + k <= Wn; x += 256) {
        uint32_t v;
        if (!bridge_wkmer(wc, wm, x, kmask, km1, v)) continue;
        for (uint32_t h = bridge_hash(v);; h = (h + 1) & (BR_SLOTS - 1)) {
            const uint32_t old = atomicCAS(&slot[h], 0u, (uint32_t)x + 1u);
            if (old == 0u) break;
            uint32_t v2;
            bridge_wkmer(wc, wm, (int32_t)(old & 0x7fffffffu) - 1, kmask, km1, v2);
            if (v2 == v) { atomicOr(&slot[h], 0x80000000u); break; }
        }
    }
    __syncthreads();
    // the bins: d = i - j, i in [ilo, ihi], j in [0, jmax]
    const int64_t ihi = (int64_t)cL - k, jmax = (int64_t)cR - k;
    const int64_t bmin = (ilo - jmax) >> 7, bmax = ihi >> 7;
    int32_t best_s = 0; int64_t best_b = 0;
    for (int64_t B0 = bmin - 1; B0 <= bmax; B0 += BR_NBIN - 1) {
        for (int b = tid; b < BR_NBIN; b += 256) bins[b] = 0;
        __syncthreads();
        const int64_t dlo = B0 * 128, dhi = (B0 + BR_NBIN) * 128 - 1;
        const int64_t ja = ilo - dhi > 0 ? ilo - dhi : 0, jb = ihi - dlo < jmax ? ihi - dlo : jmax;
        for (int64_t c0 = ja; c0 <= jb; c0 += BR_CHUNK)
            bridge_group(par2, parn, srcB, B.qlen, B.rev, c0 + 16 * tid, jb, slot, wc, wm, k, kmask, km1, ilo, [&](int32_t i, int32_t j) {
                const int64_t b = (int64_t)((i - j) >> 7) - B0;
                if (b >= 0 && b < BR_NBIN) atomicAdd(&bins[b], 1);
            });
        __syncthreads();
        unsigned long long key = 0;                       // (score, the smaller bin first)
        for (int b = tid; b < BR_NBIN - 1; b += 256) {
            const unsigned long long x = ((unsigned long long)(uint32_t)(bins[b] + bins[b + 1]) << 32) | (uint32_t)(BR_NBIN - b);
            if (x > key) key = x;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const unsigned long long y = __shfl_xor(key, o); if (y > key) key = y; }
        if (lane == 0) red[wv] = key;
        __syncthreads();
        key = red[0];
        for (int q = 1; q < 4; ++q) if (red[q] > key) key = red[q];
        const int32_t sc = (int32_t)(key >> 32);
        if (sc > best_s) { best_s = sc; best_b = B0 + (BR_NBIN - (int64_t)(uint32_t)key); }      // passes ascend: a tie keeps the smaller bin
        __syncthreads();
    }
    res.votes = best_s;
    if (best_s > 0) {
        // the band matches in ascending j, counted to the lower median
        const int32_t target = (best_s - 1) >> 1;
        const int64_t dlo = best_b * 128, dhi = dlo + 255;
        const int64_t ja = ilo - dhi > 0 ? ilo - dhi : 0, jb = ihi - dlo < jmax ? ihi - dlo : jmax;
        int32_t running = 0;
        for (int64_t c0 = ja; c0 <= jb; c0 += BR_CHUNK) {
            int32_t n = 0;
            bridge_group(par2, parn, srcB, B.qlen, B.rev, c0 + 16 * tid, jb, slot, wc, wm, k, kmask, km1, ilo, [&](int32_t i, int32_t j) {
                const int64_t d = (int64_t)i - j;
                if (d >= dlo && d <= dhi) ++n;
            });
            const int32_t incl = d_wave_incl<int32_t>(n, lane);
            if (lane == 63) part[wv] = incl;
            __syncthreads();
            int32_t before = running, total = 0;
            for (int q = 0; q < 4; ++q) { if (q < wv) before += part[q]; total += part[q]; }
            before += incl - n;
            if (before <= target && target < before + n) {
                int32_t seen = before;
                bridge_group(par2, parn, srcB, B.qlen, B.rev, c0 + 16 * tid, jb, slot, wc, wm, k, kmask, km1, ilo, [&](int32_t i, int32_t j) {
                    const int64_t d = (int64_t)i - j;
                    if (d >= dlo && d <= dhi) { if (seen == target) { found[0] = i; found[1] = j; } ++seen; }
                });
            }
            __syncthreads();
            if (running + total > target) break;
            running += total;
        }
        res.i = found[0]; res.j = found[1];
    }
    if (tid == 0) out[blockIdx.x] = res;
}

__global__ void __launch_bounds__(256) k_bridge_pick(const telr_ins_sig *__restrict__ sigs, const CutRec *__restrict__ recs, const BridgeCand *__restrict__ candl,
                                                     const BridgeCand *__restrict__ candr, const BridgeTop *__restrict__ top, const BridgeVote *__restrict__ votes,
                                                     const uint8_t *__restrict__ want, int32_t ncall, int32_t pairs, int32_t min_votes, int32_t max_len,
                                                     telr_bridge *__restrict__ out)
{
    const int64_t kc = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (kc >= ncall) return;
    telr_bridge o;
    o.sig_l = o.sig_r = -1; o.qid_l = o.start_l = o.len_l = o.rc_l = o.qid_r = o.start_r = o.len_r = o.rc_r = 0; o.votes = o.diag = o.ins_off = o.ins_len = 0;
    o.n_left = top[kc].nl; o.n_right = top[kc].nr;
    if (!want || want[kc]) {
        const int32_t pp = pairs * pairs;
        int32_t best = -1; BridgeVote bv; bv.votes = -1; bv.i = 0; bv.j = 0;
        for (int32_t s = 0; s < pp; ++s) {                // left rank major: a tie keeps the smaller left rank, then the smaller right rank
            const BridgeVote v = votes[kc * pp + s];
            if (v.votes > bv.votes) { bv = v; best = s; }
        }
        if (best >= 0 && bv.votes >= min_votes) {         // otherwise the call has none: no second pair is tried
            const int32_t jl = top[kc].sl[best / pairs], jr = top[kc].sr[best % pairs];
            const telr_ins_sig SL = sigs[jl], SR = sigs[jr];
            const CutRec A = recs[SL.rec], B = recs[SR.rec];
            const int64_t lo_l = candl[jl].x, hi_l = (int64_t)A.qe + bv.i, lo_r = bv.j, hi_r = candr[jr].x;
            const int64_t len_l = hi_l - lo_l, len_r = hi_r - lo_r;
            if (len_l + len_r >= 1 && len_l + len_r <= max_len) {
                o.sig_l = jl; o.sig_r = jr; o.qid_l = SL.qid; o.qid_r = SR.qid; o.rc_l = A.rev; o.rc_r = B.rev;
                o.len_l = (int32_t)len_l; o.len_r = (int32_t)len_r;
                o.start_l = (int32_t)(A.rev ? A.qlen - hi_l : lo_l); o.start_r = (int32_t)(B.rev ? B.qlen - hi_r : lo_r);
                o.votes = bv.votes; o.diag = bv.i - bv.j;
                o.ins_off = (int32_t)(A.qe - lo_l); o.ins_len = bv.i + (B.qs - bv.j);
            }
        }
    }
    out[kc] = o;
}

extern "C" void telr_bridge_opt_default(telr_bridge_opt *o)
{
    if (!o) return;
    o->flank = 2000; o->min_flank = 500; o->reach = 50; o->max_len = 100000; o->k = 13; o->window = 4096; o->min_votes = 8; o->pairs = 4;
}
extern "C" int64_t telr_bridges_count(const telr_bridges *b) { return b ? (int64_t)b->d.size() : 0; }
extern "C" const telr_bridge *telr_bridges_data(const telr_bridges *b) { return b ? b->d.data() : nullptr; }
extern "C" void telr_bridge_contigs_free(telr_bridges *b) { delete b; }

extern "C" int telr_bridge_contigs(telr_ctx *ctx, const telr_result *r, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls, const int64_t *read_off,
                                   const int32_t *reads, int64_t n_sig, const telr_ins_sig *sigs, const telr_seqset *read_set, const uint8_t *want,
                                   const telr_bridge_opt *opt, telr_bridges **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    telr_bridge_opt O;
    if (opt) O = *opt; else telr_bridge_opt_default(&O);
    const char *fault = (O.flank < 0 || O.min_flank < 0 || O.reach < 0 || O.max_len < 0) ? "negative option"
                        : O.min_flank > O.flank ? "min_flank > flank"
                        : (O.k < 11 || O.k > 15) ? "k outside 11 .. 15"
                        : (O.window < O.k || O.window > 4096) ? "window outside k .. 4096"
                        : (O.pairs < 1 || O.pairs > BR_MAX_PAIRS) ? "pairs outside 1 .. 8"
                        : O.min_votes < 1 ? "min_votes below 1" : nullptr;
    CutInput in;
    TRY(in.check(ctx, "telr_bridge_contigs", r, out != nullptr, n_targets, n_calls, calls, read_off, reads, n_sig, sigs, read_set, fault));
    const int64_t pp = (int64_t)O.pairs * O.pairs;
    if (n_calls * pp >= 0x7ffffff0LL) { ctx->err = "telr_bridge_contigs: too many (call, pair) workgroups"; return TELR_E_RANGE; }
    telr_bridges *D = new telr_bridges();
    std::unique_ptr<telr_bridges> guard(D);
    telr_bridge none;
    memset(&none, 0, sizeof none); none.sig_l = none.sig_r = -1;
    D->d.assign((size_t)n_calls, none);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int32_t nc = in.nc, ns = in.ns;
    TRY(in.span(O.reach, 1u << 2, false));                                        // the clips: kind 2
    if (in.P > 0) {
        TRY(in.prepare_pairs());
        BridgeCand *d_cl, *d_cr; BridgeTop *d_top; BridgeVote *d_votes; uint8_t *d_want = nullptr; telr_bridge *d_out;
        TRY(ctx_buf_t(ctx, "bridge_candl", (size_t)ns, &d_cl));
        TRY(ctx_buf_t(ctx, "bridge_candr", (size_t)ns, &d_cr));
        TRY(ctx_buf_t(ctx, "bridge_top", (size_t)nc, &d_top));
        TRY(ctx_buf_t(ctx, "bridge_votes", (size_t)(nc * pp), &d_votes));
        TRY(ctx_buf_t(ctx, "bridge_out", (size_t)nc, &d_out));
        if (want) {
            TRY(ctx_buf_t(ctx, "bridge_want", (size_t)nc, &d_want));
            HIPCHK(hipMemcpyAsync(d_want, want, (size_t)nc, hipMemcpyHostToDevice, st));
        }
        hipLaunchKernelGGL(k_bridge_cand, dim3((unsigned)(((int64_t)ns + 3) / 4)), dim3(256), 0, st, in.d_sig, ns, in.d_cnt, in.d_rec, in.d_cig, O.flank, O.min_flank, O.k, d_cl, d_cr);
        hipLaunchKernelGGL(k_bridge_top, dim3((unsigned)(((int64_t)nc + 3) / 4)), dim3(256), 0, st, in.d_sig, ns, in.d_calls, nc, d_cl, d_cr, in.d_roff, in.d_reads, O.reach, O.pairs, d_top);
        hipLaunchKernelGGL(k_bridge_vote, dim3((unsigned)(nc * pp)), dim3(256), 0, st, read_set->d_seq2, read_set->d_nmask, read_set->d_boff, in.d_sig, in.d_rec, d_top,
                           d_want, O.pairs, O.k, O.window, d_votes);
        hipLaunchKernelGGL(k_bridge_pick, grid256((int64_t)nc), dim3(256), 0, st, in.d_sig, in.d_rec, d_cl, d_cr, d_top, d_votes, d_want, nc, O.pairs, O.min_votes, O.max_len, d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(D->d.data(), d_out, (size_t)nc * sizeof(telr_bridge), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    *out = guard.release();
    return TELR_OK;
}
