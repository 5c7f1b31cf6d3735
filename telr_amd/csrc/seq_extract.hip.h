// seq_extract.hip.h -- telr_seqset_extract: pieces of a resident sequence set as text (the definition is in
// include/telr_hip.h and, as plain Python, in tests/seq_extract_ref.py).  What telr_sv.call_insertions (the ALT sequences) and
// telr_assembly.draft_loci (the contigs) cut out of the reads: some thousand pieces of a few kb, where the set itself is gigabases
// and exists in packed form only.
//
//   host      every argument checked; the pieces' lengths scanned: piece k gets a slot of (len + 15) / 16 units of 16 bytes in the
//             device text, so no store straddles two pieces; one DraftPiece (first base in the set's layout, len, rc) per piece and
//             the scanned unit offsets go up
//   device    k_seq_extract    one lane per unit: its piece from a binary search in the scanned offsets (as k_draft_extract), the
//             16 2-bit codes and 16 mask bits at the piece's base offset by the funnel shifts of stage2_common.hip.h (d_window2 /
//             d_window1), for rc read from the other end, base-reversed and complemented; four dwords of letters, one 16-byte store
//   host      the slotted text comes back in one copy (pinned) and is compacted into the caller's dense buffer
// Every store position is the lane's own index; there is no atomic; the bytes are the same on every run.  The set is not copied.
#pragma once

#define SX_MAX_UNITS (1LL << 31)      /* 16-byte units of one call: 2^35 bytes of slots */

// four letters from 8 code bits and 4 mask bits (base i: bits 2i .. 2i + 1, mask bit i); `A C G T` = 0x41 0x43 0x47 0x54
static __device__ __forceinline__ uint32_t sx_letters4(uint32_t c8, uint32_t m4)
{
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t ch = (m4 >> b & 1u) ? 0x4Eu : (0x54474341u >> (8u * (c8 >> (2 * b) & 3u))) & 0xffu;
        v |= ch << (8 * b);
    }
    return v;
}

// uoff[np + 1]: the pieces' unit offsets in the text (uoff[np] = nu); bytes of a slot behind its piece's end are zero
__global__ void __launch_bounds__(256) k_seq_extract(const uint32_t *__restrict__ seq2, const uint32_t *__restrict__ nmask, const DraftPiece *__restrict__ piece,
                                                     const int64_t *__restrict__ uoff, int32_t np, int64_t nu, uint4 *__restrict__ text)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= nu) return;
    int32_t lo = 0, hi = np;                              // first piece with uoff > u; the one before it holds u (empty pieces have no unit)
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (uoff[mid] <= u) lo = mid + 1; else hi = mid; }
    const int32_t d = lo - 1;
    const DraftPiece P = piece[d];
    const int64_t j0 = (u - uoff[d]) * 16;
    const int kb = P.len - j0 >= 16 ? 16 : (int)(P.len - j0);      // 1 .. 16: a slot has no unit behind its piece
    const int64_t S = P.rc ? P.src + P.len - 16 - j0 : P.src + j0;      // >= -15: what lies before the set reads as zero
    uint32_t code = d_window2(seq2, S), m16 = d_window1(nmask, S);
    if (P.rc) { code = ~d_rev16x2(code); m16 = __brev(m16) >> 16; }
    uint4 o;
    o.x = sx_letters4(code & 0xffu, m16 & 0xfu);
    o.y = sx_letters4(code >> 8 & 0xffu, m16 >> 4 & 0xfu);
    o.z = sx_letters4(code >> 16 & 0xffu, m16 >> 8 & 0xfu);
    o.w = sx_letters4(code >> 24, m16 >> 12 & 0xfu);
    if (kb < 16) {                                        // the piece's last unit: zero behind its end
        const uint32_t full = 0xffffffffu;
        const int q = kb >> 2, r = (kb & 3) * 8;
        const uint32_t part = r ? (1u << r) - 1u : 0u;
        o.x &= q > 0 ? full : part;
        o.y &= q > 1 ? full : q == 1 ? part : 0u;
        o.z &= q > 2 ? full : q == 2 ? part : 0u;
        o.w &= q == 3 ? part : 0u;
    }
    text[u] = o;
}

extern "C" int telr_seqset_extract(telr_ctx *ctx, const telr_seqset *s, int64_t n, const int32_t *idx, const int32_t *start, const int32_t *len,
                                   const uint8_t *rc, char *out, const int64_t *out_off)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    auto bad = [&](const std::string &why) { ctx->err = "telr_seqset_extract: " + why; return TELR_E_ARG; };
    if (!s) return bad("null set");
    if (n < 0) return bad("negative n");
    if (n == 0) return TELR_OK;
    if (!idx || !start || !len || !out || !out_off) return bad("null idx, start, len, out or out_off");
    if (n >= 0x7ffffff0LL) { ctx->err = "telr_seqset_extract: too many pieces"; return TELR_E_RANGE; }
    std::vector<DraftPiece> pieces((size_t)n);
    std::vector<int64_t> uoff((size_t)n + 1);
    int64_t nu = 0, total = 0;
    if (out_off[0] < 0) return bad("negative out_off");
    for (int64_t k = 0; k < n; ++k) {
        const std::string who = "piece " + std::to_string(k);
        if (idx[k] < 0 || idx[k] >= s->n) return bad(who + ": idx outside the set");
        if (start[k] < 0) return bad(who + ": negative start");
        if (len[k] < 0) return bad(who + ": negative len");
        if ((int64_t)start[k] + len[k] > s->len[(size_t)idx[k]]) return bad(who + ": start + len beyond the sequence");
        if (out_off[k + 1] - out_off[k] != len[k]) return bad(who + ": out_off does not match len");
        DraftPiece &p = pieces[(size_t)k];
        p.src = s->boff[(size_t)idx[k]] + start[k]; p.len = len[k]; p.rc = (rc && rc[k]) ? 1 : 0;
        uoff[(size_t)k] = nu; nu += ((int64_t)len[k] + 15) >> 4; total += len[k];
    }
    uoff[(size_t)n] = nu;
    if (nu >= SX_MAX_UNITS) { ctx->err = "telr_seqset_extract: the pieces' 16-byte slots reach 2^35 bytes"; return TELR_E_RANGE; }
    if (total == 0) return TELR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DraftPiece *d_piece; int64_t *d_uoff; uint4 *d_text; uint8_t *h_text;
    TRY(ctx_buf_t(ctx, "sx_piece", (size_t)n, &d_piece));
    TRY(ctx_buf_t(ctx, "sx_uoff", (size_t)n + 1, &d_uoff));
    TRY(ctx_buf_t(ctx, "sx_text", (size_t)nu, &d_text));
    TRY(ctx_hbuf_t(ctx, "sx_text_host", (size_t)nu * 16, &h_text));
    HIPCHK(hipMemcpyAsync(d_piece, pieces.data(), (size_t)n * sizeof(DraftPiece), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_uoff, uoff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_seq_extract, grid256(nu), dim3(256), 0, st, s->d_seq2, s->d_nmask, d_piece, d_uoff, (int32_t)n, nu, d_text);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_text, d_text, (size_t)nu * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t k = 0; k < n; ++k)
        if (len[k]) memcpy(out + out_off[k], h_text + uoff[(size_t)k] * 16, (size_t)len[k]);
    return TELR_OK;
}

// ---- telr_seqset_join: a new set whose sequences are concatenations of pieces of a resident set (the definition is in
// include/telr_hip.h and, as plain Python, in tests/bridge_ref.py).  What telr_assembly.draft_loci makes its contig set with when a
// locus may be a bridge of two reads (telr_bridge_contigs): one piece for a draft, two for a bridge.
//
//   host      every argument checked; the pieces' first bases in the OUTPUT set's base layout scanned (ppos[g], ppos[np] = the padded
//             bases): the pieces of one sequence follow each other without a gap, the next sequence starts at its 64-base-aligned offset
//   device    k_seq_join   one lane per 2-bit output word: the piece holding its first base = the last one with ppos <= that base (a
//             binary search; empty pieces share a ppos, the last of them is the one that goes on), then on through as many pieces as
//             the word touches (a piece may be shorter than 16 bases) while the next piece starts where the last one ended -- a piece of
//             another sequence starts past the word, since sequences start at multiples of 64.  Every piece's bases come through the
//             funnel shifts and the reverse complement of stage2_common.hip.h as in k_draft_extract, shifted to their place in the word;
//             mask words as there: the two lanes of a 32-base unit join their halves.
// Every store position is the lane's own index; there is no atomic; the bytes are the same on every run.
__global__ void __launch_bounds__(256) k_seq_join(const uint32_t *__restrict__ par2, const uint32_t *__restrict__ parn, const DraftPiece *__restrict__ piece,
                                                  const int64_t *__restrict__ ppos, int32_t np, int64_t nw, uint32_t *__restrict__ out2, uint32_t *__restrict__ outn)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;                                  // (nw is even: the two lanes of a 32-base unit stay or leave together)
    const int64_t b0 = w * 16;
    int32_t lo = 0, hi = np;                              // first piece with ppos > b0 (ppos[0] = 0: there is one before it)
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (ppos[mid] <= b0) lo = mid + 1; else hi = mid; }
    uint32_t code = 0, m16 = 0;
    int filled = 0;
    for (int32_t g = lo - 1; filled < 16 && g < np; ++g) {
        const int64_t j0 = b0 + filled - ppos[g];         // the word's next base within piece g
        if (j0 < 0) break;                                // piece g opens another sequence: padding from here on
        const DraftPiece P = piece[g];
        if (j0 >= P.len) continue;                        // used up (or empty): the next piece goes on, if it starts here
        const int take = P.len - j0 >= 16 - filled ? 16 - filled : (int)(P.len - j0);
        const int64_t S = P.rc ? P.src + P.len - 16 - j0 : P.src + j0;      // >= -15: what lies before the set reads as zero
        uint32_t c = d_window2(par2, S), m = d_window1(parn, S);
        if (P.rc) { c = ~d_rev16x2(c); m = __brev(m) >> 16; }
        const uint32_t keep = take == 16 ? 0xffffu : (1u << take) - 1u;
        m &= keep;
        c &= d_spread16(keep & ~m) * 3u;              // an N keeps its mask bit and code 0, as the packers write it
        code |= c << (2 * filled); m16 |= m << filled;
        filled += take;
    }
    out2[w] = code;
    const uint32_t other = __shfl_xor(m16, 1);
    if (!(w & 1)) outn[w >> 1] = m16 | (other << 16);
}

extern "C" int telr_seqset_join(telr_ctx *ctx, const telr_seqset *parent, int32_t n_out, const int64_t *piece_off, const int32_t *idx, const int32_t *start,
                                const int32_t *len, const uint8_t *rc, telr_seqset **out)
{
    (void)hipGetLastError();
    if (!ctx) return TELR_E_ARG;
    auto bad = [&](const std::string &why) { ctx->err = "telr_seqset_join: " + why; return TELR_E_ARG; };
    if (!parent || !out) return bad("null set or output");
    if (n_out < 0) return bad("negative n_out");
    if (n_out > 0 && !piece_off) return bad("null piece_off");
    if (n_out >= 0x7ffffff0) { ctx->err = "telr_seqset_join: too many sequences"; return TELR_E_RANGE; }
    if (n_out > 0 && piece_off[0] != 0) return bad("piece_off does not start at 0");
    for (int32_t o = 0; o < n_out; ++o)
        if (piece_off[o + 1] < piece_off[o]) return bad("sequence " + std::to_string(o) + ": piece_off decreases");
    const int64_t np = n_out > 0 ? piece_off[n_out] : 0;
    if (np > 0 && (!idx || !start || !len)) return bad("null idx, start or len");
    if (np >= 0x7ffffff0LL) { ctx->err = "telr_seqset_join: too many pieces"; return TELR_E_RANGE; }
    std::vector<int32_t> lens((size_t)n_out);
    std::vector<DraftPiece> pieces((size_t)np);
    std::vector<int64_t> ppos((size_t)np + 1);
    int64_t tot = 0;                                      // the output's padded bases so far (seqset_alloc's layout)
    for (int32_t o = 0; o < n_out; ++o) {
        int64_t joined = 0;
        for (int64_t g = piece_off[o]; g < piece_off[o + 1]; ++g) {
            const std::string who = "piece " + std::to_string(g);
            if (idx[g] < 0 || idx[g] >= parent->n) return bad(who + ": idx outside the set");
            if (start[g] < 0) return bad(who + ": negative start");
            if (len[g] < 0) return bad(who + ": negative len");
            if ((int64_t)start[g] + len[g] > parent->len[(size_t)idx[g]]) return bad(who + ": start + len beyond the sequence");
            DraftPiece &p = pieces[(size_t)g];
            p.src = parent->boff[(size_t)idx[g]] + start[g]; p.len = len[g]; p.rc = (rc && rc[g]) ? 1 : 0;
            ppos[(size_t)g] = tot + joined; joined += len[g];
            if (joined > 0x7fffffffLL) { ctx->err = "telr_seqset_join: sequence " + std::to_string(o) + ": joined length above INT32_MAX"; return TELR_E_RANGE; }
        }
        lens[(size_t)o] = (int32_t)joined; tot += (joined + 63) & ~63LL;
    }
    ppos[(size_t)np] = tot;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    telr_seqset *S = nullptr;
    TRY(draft_make_set(ctx, "telr_seqset_join", lens, &S));
    if (S->padded_bases > 0) {
        const int64_t nw = S->padded_bases / 16;
        DraftPiece *d_piece = nullptr; int64_t *d_ppos = nullptr;
        int rc_ = ctx_buf_t(ctx, "join_piece", (size_t)np, &d_piece);
        if (rc_ == TELR_OK) rc_ = ctx_buf_t(ctx, "join_ppos", (size_t)np + 1, &d_ppos);
        if (rc_ != TELR_OK) { telr_seqset_free(S); return rc_; }
        hipError_t e = hipMemcpyAsync(d_piece, pieces.data(), (size_t)np * sizeof(DraftPiece), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_ppos, ppos.data(), ((size_t)np + 1) * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_seq_join, grid256(nw), dim3(256), 0, st, parent->d_seq2, parent->d_nmask, d_piece, d_ppos, (int32_t)np, nw, S->d_seq2, S->d_nmask);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { ctx->err = std::string("telr_seqset_join: ") + hipGetErrorString(e); telr_seqset_free(S); return TELR_E_HIP; }
    }
    *out = S;
    return TELR_OK;
}
