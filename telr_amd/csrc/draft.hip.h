// A draft contig per insertion call, cut out of one of its supporting reads on the device (include/telr_hip.h:
// telr_draft_contigs).  Stands where the reference shells out to wtdbg2 or flye (`run_wtdbg2_assembly` / `run_flye_assembly`,
// src/telr/TELR_assembly.py:264-382) -- with an own, fully specified definition that is NOT an assembler and NOT wtdbg2 or flye: for
// every call one supporting read is the backbone, and the piece of it that carries the insertion between reference-aligned flanks is
// the draft, on the reference strand.
//
//   CutInput         (stage2_common.hip.h, the input that telr_bridge_contigs takes too) the refusals, the uploads, k_cut_span over the
//                    sized signatures (kinds 0 and 1) and the 64-bit scan of its counts: the (signature, call) pairs;
//   k_draft_pairs    one lane per (signature, call) pair: its signature from a binary search in the scanned counts, its call from its
//                    rank in the run, membership of the signature's read in the call's supporter list from a binary search;
//   k_draft_walk     one wave per pair, 64 CIGAR words per step (coalesced dwords), wave prefix sums of the reference and query lengths
//                    carried from step to step: lo_a(xL) and hi_b(xR) -- one walk of one record for kind 0, one walk each of a and b for
//                    kind 1; the wave leaves once a step starts past the coordinate it looks for;
//   k_draft_select   one wave per call: the signatures within `reach` of it are a contiguous run of the sorted signature array, a
//                    pair's place is (its signature's scanned offset) + (the call's rank in the signature's run); the smallest key by a
//                    wave reduction over a total order (the signature's index closes it), so no atomic and no arrival order decides;
//   k_draft_extract  one lane per 2-bit output word (16 bases): a funnel shift of two words of the parent set, for rc the base-reversed
//                    complement of the words read from the other end; the two lanes of a 32-base unit join their halves of the
//                    ambiguity word; padding behind a draft is zero in both arrays.
#pragma once

struct DraftCand { int64_t dlen; int32_t valid, fl, lo, n; };                         // a pair's share of the key and its piece of the read

struct telr_drafts { std::vector<telr_draft> d; };

// off = exclusive scan of cnt (off[ns] = np).  pcall[p] = the pair's call, or ~call when the signature's read is no supporter of it
__global__ void __launch_bounds__(256) k_draft_pairs(const int64_t *__restrict__ off, int32_t ns, const int32_t *__restrict__ first, int64_t np,
                                                     const telr_ins_sig *__restrict__ sigs, const int64_t *__restrict__ read_off, const int32_t *__restrict__ reads,
                                                     int32_t *__restrict__ psig, int32_t *__restrict__ pcall)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const int32_t j = d_pair_owner(off, ns, p), k = first[j] + (int32_t)(p - off[j]), q = sigs[j].qid;
    psig[p] = j; pcall[p] = d_in_list(reads, read_off[k], read_off[k + 1], q) ? k : ~k;
}

__global__ void __launch_bounds__(256) k_draft_walk(const telr_ins_sig *__restrict__ sigs, const telr_ins_call *__restrict__ calls, const CutRec *__restrict__ recs,
                                                    const uint32_t *__restrict__ cig, const int32_t *__restrict__ psig, const int32_t *__restrict__ pcall, int64_t np,
                                                    int32_t flank, int32_t min_flank, int32_t max_len, DraftCand *__restrict__ cand)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (w >= np) return;
    const int32_t k = pcall[w];
    DraftCand out; out.dlen = 0; out.valid = 0; out.fl = 0; out.lo = 0; out.n = 0;
    if (k >= 0) {                                         // (the same in every lane of the wave)
        const telr_ins_sig s = sigs[psig[w]];
        const CutRec A = recs[s.rec], B = s.kind == 0 ? A : recs[s.mate];
        const int64_t lpos = s.pos, rpos = s.kind == 0 ? (int64_t)s.pos : (int64_t)B.ts;
        const int64_t xL = lpos - flank > A.ts ? lpos - flank : (int64_t)A.ts, xR = rpos + flank < B.te ? rpos + flank : (int64_t)B.te;
        const int64_t fl = lpos - xL < xR - rpos ? lpos - xL : xR - rpos;
        if (A.n_cigar > 0 && B.n_cigar > 0 && fl >= min_flank) {
            int64_t lo = 0, hi = 0; bool flo = false, fhi = false;
            if (s.kind == 0) draft_walk<true, true>(cig + A.cigar_off, A.n_cigar, A.ts, A.qs, xL, xR, lane, lo, flo, hi, fhi);
            else {
                draft_walk<true, false>(cig + A.cigar_off, A.n_cigar, A.ts, A.qs, xL, xL, lane, lo, flo, hi, fhi);
                draft_walk<false, true>(cig + B.cigar_off, B.n_cigar, B.ts, B.qs, xR, xR, lane, lo, flo, hi, fhi);
            }
            const int64_t n = hi - lo, d = (int64_t)s.len - calls[k].len;
            if (flo && fhi && n >= 1 && n <= max_len && lo >= 0 && hi <= A.qlen) {
                out.valid = 1; out.dlen = d < 0 ? -d : d; out.fl = (int32_t)fl; out.lo = (int32_t)lo; out.n = (int32_t)n;
            }
        }
    }
    if (lane == 0) cand[w] = out;
}

struct DraftBest { int64_t dlen; int32_t has, fl, qid, rec, mate, j, lo, n; };
static __device__ __forceinline__ bool draft_better(const DraftBest &x, const DraftBest &y)      // x before y in (dlen, -fl, qid, rec, mate, j)
{
    if (x.has != y.has) return x.has > y.has;
    if (x.dlen != y.dlen) return x.dlen < y.dlen;
    if (x.fl != y.fl) return x.fl > y.fl;
    if (x.qid != y.qid) return x.qid < y.qid;
    if (x.rec != y.rec) return x.rec < y.rec;
    if (x.mate != y.mate) return x.mate < y.mate;
    return x.j < y.j;
}

__global__ void __launch_bounds__(256) k_draft_select(const telr_ins_sig *__restrict__ sigs, int32_t ns, const telr_ins_call *__restrict__ calls, int32_t ncall,
                                                      const CutRec *__restrict__ recs, const int32_t *__restrict__ first, const int32_t *__restrict__ cnt,
                                                      const int64_t *__restrict__ off, const DraftCand *__restrict__ cand, int32_t reach, telr_draft *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (k >= ncall) return;
    const telr_ins_call c = calls[k];
    int32_t s0, s1;
    d_sig_window(sigs, ns, c, reach, &s0, &s1);
    DraftBest best; best.has = 0; best.dlen = 0; best.fl = 0; best.qid = 0; best.rec = 0; best.mate = 0; best.j = 0; best.lo = 0; best.n = 0;
    for (int32_t j = s0 + lane; j < s1; j += 64) {
        const int32_t f = first[j], r = (int32_t)k - f;
        if (r < 0 || r >= cnt[j]) continue;               // an unsized signature has no pairs
        const DraftCand d = cand[off[j] + r];
        if (!d.valid) continue;
        const telr_ins_sig s = sigs[j];
        DraftBest x; x.has = 1; x.dlen = d.dlen; x.fl = d.fl; x.qid = s.qid; x.rec = s.rec; x.mate = s.mate; x.j = j; x.lo = d.lo; x.n = d.n;
        if (draft_better(x, best)) best = x;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        DraftBest y;
        y.dlen = __shfl_xor(best.dlen, o); y.has = __shfl_xor(best.has, o); y.fl = __shfl_xor(best.fl, o); y.qid = __shfl_xor(best.qid, o);
        y.rec = __shfl_xor(best.rec, o); y.mate = __shfl_xor(best.mate, o); y.j = __shfl_xor(best.j, o); y.lo = __shfl_xor(best.lo, o); y.n = __shfl_xor(best.n, o);
        if (draft_better(y, best)) best = y;
    }
    if (lane != 0) return;
    telr_draft d;
    d.sig = -1; d.qid = 0; d.start = 0; d.len = 0; d.rc = 0; d.ins_off = 0; d.ins_len = 0; d.set_index = -1;
    if (best.has) {
        const telr_ins_sig s = sigs[best.j];
        const CutRec A = recs[s.rec];
        d.sig = best.j; d.qid = s.qid; d.len = best.n; d.rc = A.rev;
        d.start = A.rev ? A.qlen - (best.lo + best.n) : best.lo;
        d.ins_len = s.seg_len;
        d.ins_off = (A.rev ? A.qlen - (s.seg_start + s.seg_len) : s.seg_start) - best.lo;
        d.set_index = 0;                                  // its place in the set: the host's scan of the calls that have a draft
    }
    out[k] = d;
}

// boff[nd + 1]: the drafts' base offsets in the output set (multiples of 64; boff[nd] = its padded bases = 16 * nw, nw even)
__global__ void __launch_bounds__(256) k_draft_extract(const uint32_t *__restrict__ par2, const uint32_t *__restrict__ parn, const DraftPiece *__restrict__ piece,
                                                       const int64_t *__restrict__ boff, int32_t nd, int64_t nw, uint32_t *__restrict__ out2, uint32_t *__restrict__ outn)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;                                  // (nw is even: the two lanes of a 32-base unit stay or leave together)
    const int64_t b0 = w * 16;
    int32_t lo = 0, hi = nd;                              // first draft with boff > b0
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (boff[mid] <= b0) lo = mid + 1; else hi = mid; }
    const int32_t d = lo - 1;
    const DraftPiece P = piece[d];
    const int64_t j0 = b0 - boff[d];
    const int kb = P.len - j0 >= 16 ? 16 : P.len - j0 > 0 ? (int)(P.len - j0) : 0;      // bases of the draft in this word
    uint32_t code = 0, m16 = 0;
    if (kb > 0) {
        const int64_t S = P.rc ? P.src + P.len - 16 - j0 : P.src + j0;
        code = d_window2(par2, S); m16 = d_window1(parn, S);
        if (P.rc) { code = ~d_rev16x2(code); m16 = __brev(m16) >> 16; }
        const uint32_t keep = kb == 16 ? 0xffffu : (1u << kb) - 1u;
        m16 &= keep;
        code &= d_spread16(keep & ~m16) * 3u;         // an N keeps its mask bit and code 0, as the packers write it
    }
    out2[w] = code;
    const uint32_t other = __shfl_xor(m16, 1);
    if (!(w & 1)) outn[w >> 1] = m16 | (other << 16);
}

extern "C" void telr_draft_opt_default(telr_draft_opt *o)
{
    if (!o) return;
    o->flank = 2000; o->min_flank = 500; o->reach = 50; o->max_len = 100000; o->reserved[0] = o->reserved[1] = o->reserved[2] = o->reserved[3] = 0;
}
extern "C" int64_t telr_drafts_count(const telr_drafts *d) { return d ? (int64_t)d->d.size() : 0; }
extern "C" const telr_draft *telr_drafts_data(const telr_drafts *d) { return d ? d->d.data() : nullptr; }
extern "C" void telr_draft_contigs_free(telr_drafts *d) { delete d; }

// an output set of the given lengths (seqset_alloc: layout, arrays, zeroed slack words, offsets uploaded); the words are the caller's to write
static int draft_make_set(telr_ctx *ctx, const char *what, const std::vector<int32_t> &lens, telr_seqset **out)
{
    telr_seqset *s = new telr_seqset();
    s->ctx = ctx; s->n = (int32_t)lens.size(); s->len = lens;
    TRY(seqset_alloc(ctx, s, what, true, ctx->stream));
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string(what) + ": " + hipGetErrorString(e); telr_seqset_free(s); return TELR_E_HIP; }
    *out = s;
    return TELR_OK;
}

// A new set whose sequence k is piece k of `parent` (pieces[k].src = its first base in the parent's base layout, checked by the caller),
// each at a 64-base-aligned offset, cut by k_draft_extract: the one way a set is made of pieces of another (telr_draft_contigs,
// telr_seqset_pieces).  A piece of length 0 is an empty sequence; no pieces: an empty set.
static int draft_cut_set(telr_ctx *ctx, const char *what, const telr_seqset *parent, const std::vector<int32_t> &lens, const std::vector<DraftPiece> &pieces, telr_seqset **out)
{
    hipStream_t st = ctx->stream;
    telr_seqset *S = nullptr;
    TRY(draft_make_set(ctx, what, lens, &S));
    if (S->padded_bases > 0) {
        const int32_t nd = (int32_t)pieces.size();
        const int64_t nw = S->padded_bases / 16;
        DraftPiece *d_piece = nullptr;
        int rc_ = ctx_buf_t(ctx, "draft_piece", (size_t)nd, &d_piece);
        if (rc_ != TELR_OK) { telr_seqset_free(S); return rc_; }
        hipError_t e = hipMemcpyAsync(d_piece, pieces.data(), (size_t)nd * sizeof(DraftPiece), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_draft_extract, grid256(nw), dim3(256), 0, st, parent->d_seq2, parent->d_nmask, d_piece, S->d_boff, nd, nw, S->d_seq2, S->d_nmask);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { ctx->err = std::string(what) + ": " + hipGetErrorString(e); telr_seqset_free(S); return TELR_E_HIP; }
    }
    *out = S;
    return TELR_OK;
}

extern "C" int telr_draft_contigs(telr_ctx *ctx, const telr_result *r, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls, const int64_t *read_off,
                                  const int32_t *reads, int64_t n_sig, const telr_ins_sig *sigs, const telr_seqset *read_set, const telr_draft_opt *opt,
                                  telr_drafts **out, telr_seqset **out_set)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    telr_draft_opt O;
    if (opt) O = *opt; else telr_draft_opt_default(&O);
    const char *fault = (O.flank < 0 || O.min_flank < 0 || O.reach < 0 || O.max_len < 0 || O.reserved[0] < 0 || O.reserved[1] < 0 || O.reserved[2] < 0 || O.reserved[3] < 0)
                            ? "negative option" : O.min_flank > O.flank ? "min_flank > flank" : nullptr;
    CutInput in;
    TRY(in.check(ctx, "telr_draft_contigs", r, out && out_set, n_targets, n_calls, calls, read_off, reads, n_sig, sigs, read_set, fault));
    telr_drafts *D = new telr_drafts();
    std::unique_ptr<telr_drafts> guard(D);
    telr_draft none; none.sig = -1; none.qid = 0; none.start = 0; none.len = 0; none.rc = 0; none.ins_off = 0; none.ins_len = 0; none.set_index = -1;
    D->d.assign((size_t)n_calls, none);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int32_t nc = in.nc, ns = in.ns;
    TRY(in.span(O.reach, 1u << 0 | 1u << 1, true));                               // the sized signatures: kinds 0 and 1
    const int64_t P = in.P;
    if (P > 0) {
        TRY(in.prepare_pairs());
        int32_t *d_psig, *d_pcall; DraftCand *d_cand; telr_draft *d_out;
        TRY(ctx_buf_t(ctx, "draft_psig", (size_t)P, &d_psig));
        TRY(ctx_buf_t(ctx, "draft_pcall", (size_t)P, &d_pcall));
        TRY(ctx_buf_t(ctx, "draft_cand", (size_t)P, &d_cand));
        TRY(ctx_buf_t(ctx, "draft_out", (size_t)nc, &d_out));
        hipLaunchKernelGGL(k_draft_pairs, grid256(P), dim3(256), 0, st, in.d_off, ns, in.d_first, P, in.d_sig, in.d_roff, in.d_reads, d_psig, d_pcall);
        hipLaunchKernelGGL(k_draft_walk, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, in.d_sig, in.d_calls, in.d_rec, in.d_cig, d_psig, d_pcall, P, O.flank, O.min_flank, O.max_len, d_cand);
        hipLaunchKernelGGL(k_draft_select, dim3((unsigned)(((int64_t)nc + 3) / 4)), dim3(256), 0, st, in.d_sig, ns, in.d_calls, nc, in.d_rec, in.d_first, in.d_cnt, in.d_off, d_cand, O.reach, d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(D->d.data(), d_out, (size_t)nc * sizeof(telr_draft), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // the output set: the drafts in call order, each at a 64-base-aligned offset
    std::vector<int32_t> lens;
    std::vector<DraftPiece> pieces;
    for (int64_t k = 0; k < n_calls; ++k) {
        telr_draft &d = D->d[k];
        if (d.sig < 0) continue;
        d.set_index = (int32_t)lens.size();
        DraftPiece p; p.src = read_set->boff[d.qid] + d.start; p.len = d.len; p.rc = d.rc;
        lens.push_back(d.len); pieces.push_back(p);
    }
    telr_seqset *S = nullptr;
    TRY(draft_cut_set(ctx, "telr_draft_contigs", read_set, lens, pieces, &S));
    *out = guard.release(); *out_set = S;
    return TELR_OK;
}

extern "C" int telr_seqset_pieces(telr_ctx *ctx, const telr_seqset *parent, int32_t n, const int32_t *idx, const int32_t *start, const int32_t *len,
                                  const uint8_t *rc, telr_seqset **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    auto bad = [&](const std::string &why) { ctx->err = "telr_seqset_pieces: " + why; return TELR_E_ARG; };
    if (!parent || !out) return bad("null set or output");
    if (n < 0) return bad("negative n");
    if (n > 0 && (!idx || !start || !len)) return bad("null idx, start or len");
    if (n >= 0x7ffffff0) { ctx->err = "telr_seqset_pieces: too many pieces"; return TELR_E_RANGE; }
    std::vector<int32_t> lens((size_t)n);
    std::vector<DraftPiece> pieces((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        const std::string who = "piece " + std::to_string(k);
        if (idx[k] < 0 || idx[k] >= parent->n) return bad(who + ": idx outside the set");
        if (start[k] < 0) return bad(who + ": negative start");
        if (len[k] < 0) return bad(who + ": negative len");
        if ((int64_t)start[k] + len[k] > parent->len[(size_t)idx[k]]) return bad(who + ": start + len beyond the sequence");
        DraftPiece &p = pieces[(size_t)k];
        p.src = parent->boff[(size_t)idx[k]] + start[k]; p.len = len[k]; p.rc = (rc && rc[k]) ? 1 : 0;
        lens[(size_t)k] = len[k];
    }
    HIPCHK(hipSetDevice(ctx->device));
    return draft_cut_set(ctx, "telr_seqset_pieces", parent, lens, pieces, out);
}
