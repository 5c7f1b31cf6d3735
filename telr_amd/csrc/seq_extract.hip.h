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
