// inflate_core.h -- the serial part of the BGZF member decoder (RFC 1951): bit reader, table builder and symbol loop, written as
// plain functions that compile for the device (bam_in.hip.h: k_bgzf_inflate, one workgroup per member) and for the host
// (tools/ubench/inflate_host.cpp, the sanitizer twin).  What differs between the two is behind two small policies:
//   Src   where the compressed bytes come from:  get8(pos), get32(pos) with pos + 1 / pos + 4 <= the member's deflate bytes
//   Sink  where the output window lives:         lit(pos, byte), match(pos, dist, len), stored(pos, ipos, len)
// Every index that comes out of the stream -- table index, distance, output position, input position -- is checked before it is
// used; a bad stream returns its INFL_E_* code and nothing past the window or the member has been touched.
#ifndef TELR_INFLATE_CORE_H
#define TELR_INFLATE_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define INFL_HD __host__ __device__ inline
#else
#define INFL_HD inline
#endif

enum {
    INFL_OK = 0,
    INFL_E_INPUT = 1,     // the stream reads past its member
    INFL_E_BTYPE = 2,     // block type 3
    INFL_E_STORED = 3,    // LEN / NLEN of a stored block disagree
    INFL_E_CODELEN = 4,   // a code-length set that is over-subscribed, too long, or without the end-of-block code
    INFL_E_SYMBOL = 5,    // bits that are no code of the table, or a length / distance symbol that does not exist
    INFL_E_DIST = 6,      // a distance that reaches before the member's start
    INFL_E_LONG = 7,      // more output than ISIZE
    INFL_E_SHORT = 8,     // less output than ISIZE
    INFL_E_CRC = 9        // the CRC-32 of the output is not the trailer's
};

#define INFL_LBITS 10
#define INFL_DBITS 8
struct InflTables {
    uint16_t lcount[16], lsym[288];
    uint16_t dcount[16], dsym[32];
    uint16_t lfast[1 << INFL_LBITS];     // (symbol << 4 | code length) of every code of at most INFL_LBITS bits, by its bits as they arrive; 0: a longer code
    uint16_t dfast[1 << INFL_DBITS];
    uint8_t lens[352];                  // 19 code-length lengths, then up to 286 + 30 lengths read behind them
};

struct InflBits { uint64_t bits; uint32_t n; uint32_t pos; };       // `n` valid bits in `bits`, next input byte `pos`

// at least 32 valid bits unless the input ends before
template <class Src> INFL_HD void infl_refill(InflBits &B, Src &S, uint32_t in_len)
{
    if (B.n > 32) return;
    if (B.pos + 4 <= in_len) { B.bits |= (uint64_t)S.get32(B.pos) << B.n; B.pos += 4; B.n += 32; return; }
    while (B.n <= 56 && B.pos < in_len) { B.bits |= (uint64_t)S.get8(B.pos) << B.n; ++B.pos; B.n += 8; }
}
// take k <= 16 bits; false: the input has fewer
template <class Src> INFL_HD bool infl_take(InflBits &B, Src &S, uint32_t in_len, uint32_t k, uint32_t *out)
{
    infl_refill(B, S, in_len);
    if (B.n < k) return false;
    *out = (uint32_t)(B.bits & ((1u << k) - 1u));
    B.bits >>= k; B.n -= k;
    return true;
}

// canonical code of lens[0 .. n): counts per length, symbols in code order, and the fast table of `fb` bits.
// false: over-subscribed (the only defect that could index outside a table); an incomplete set is accepted, its unassigned bit
// patterns decode to INFL_E_SYMBOL.
INFL_HD bool infl_build(const uint8_t *lens, int n, uint16_t *count, uint16_t *sym, uint16_t *fast, int fb)
{
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) ++count[lens[i] & 15];
    int left = 1;
    for (int l = 1; l < 16; ++l) { left <<= 1; left -= count[l]; if (left < 0) return false; }
    uint16_t offs[16]; uint32_t next[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    uint32_t code = 0; count[0] = 0;
    for (int l = 1; l < 16; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
    for (int i = 0; i < (1 << fb); ++i) fast[i] = 0;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (!l) continue;
        sym[offs[l]++] = (uint16_t)i;                         // at most n symbols have a length: inside sym[n]
        const uint32_t c = next[l]++;                         // < 2^l: the set is not over-subscribed
        if (l <= fb) {
            uint32_t r = 0;
            for (int b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);
            for (uint32_t j = r; j < (1u << fb); j += 1u << l) fast[j] = (uint16_t)(i << 4 | l);
        }
    }
    return true;
}

// one symbol; < 0: INFL_E_INPUT (negated) or INFL_E_SYMBOL (negated)
template <class Src> INFL_HD int infl_symbol(InflBits &B, Src &S, uint32_t in_len, const uint16_t *count, const uint16_t *sym, int nsym,
                                             const uint16_t *fast, int fb)
{
    infl_refill(B, S, in_len);
    const uint32_t e = fast[B.bits & ((1u << fb) - 1u)];
    if (e) {
        const uint32_t l = e & 15u;
        if (l > B.n) return -INFL_E_INPUT;
        B.bits >>= l; B.n -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((B.bits >> (l - 1)) & 1u);
        const int c = count[l];
        if (code - c < first) {
            if ((uint32_t)l > B.n) return -INFL_E_INPUT;
            const int k = index + (code - first);
            if (k < 0 || k >= nsym) return -INFL_E_SYMBOL;
            B.bits >>= l; B.n -= l;
            return sym[k];
        }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return B.n < 15 ? -INFL_E_INPUT : -INFL_E_SYMBOL;
}

INFL_HD uint32_t infl_len_base(int s)  { const uint16_t t[29] = {3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258}; return t[s]; }
INFL_HD uint32_t infl_len_extra(int s) { return s < 8 ? 0u : s == 28 ? 0u : (uint32_t)((s - 4) >> 2); }
INFL_HD uint32_t infl_dist_base(int s) { return s < 4 ? (uint32_t)s + 1u : ((2u + (uint32_t)(s & 1)) << ((s >> 1) - 1)) + 1u; }
INFL_HD uint32_t infl_dist_extra(int s) { return s < 4 ? 0u : (uint32_t)((s >> 1) - 1); }

// the member: in_len deflate bytes behind Src, exactly isize bytes into Sink.  -> INFL_OK or the first defect
template <class Src, class Sink> INFL_HD int infl_member(Src &S, uint32_t in_len, uint32_t isize, InflTables *T, Sink &W)
{
    InflBits B; B.bits = 0; B.n = 0; B.pos = 0;
    uint32_t opos = 0, v = 0;
    for (;;) {
        uint32_t last, type;
        if (!infl_take(B, S, in_len, 1, &last) || !infl_take(B, S, in_len, 2, &type)) return INFL_E_INPUT;
        if (type == 3) return INFL_E_BTYPE;
        if (type == 0) {
            const uint32_t drop = B.n & 7u;                   // to the byte boundary
            B.bits >>= drop; B.n -= drop;
            uint32_t len, nlen;
            if (!infl_take(B, S, in_len, 16, &len) || !infl_take(B, S, in_len, 16, &nlen)) return INFL_E_INPUT;
            if ((len ^ 0xffffu) != nlen) return INFL_E_STORED;
            const uint32_t ipos = B.pos - (B.n >> 3);          // whole bytes are buffered: give them back
            if (ipos + len > in_len) return INFL_E_INPUT;
            if (opos + len > isize) return INFL_E_LONG;
            W.stored(opos, ipos, len);
            opos += len;
            B.bits = 0; B.n = 0; B.pos = ipos + len;
        } else {
            int nl, nd;
            if (type == 1) {
                for (int i = 0; i < 144; ++i) T->lens[i] = 8;
                for (int i = 144; i < 256; ++i) T->lens[i] = 9;
                for (int i = 256; i < 280; ++i) T->lens[i] = 7;
                for (int i = 280; i < 288; ++i) T->lens[i] = 8;
                for (int i = 288; i < 318; ++i) T->lens[i] = 5;
                nl = 288; nd = 30;
            } else {
                uint32_t hl, hd, hc;
                if (!infl_take(B, S, in_len, 5, &hl) || !infl_take(B, S, in_len, 5, &hd) || !infl_take(B, S, in_len, 4, &hc)) return INFL_E_INPUT;
                nl = (int)hl + 257; nd = (int)hd + 1;
                const int nc = (int)hc + 4;
                if (nl > 286 || nd > 30) return INFL_E_CODELEN;
                const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                for (int i = 0; i < 19; ++i) T->lens[i] = 0;
                for (int i = 0; i < nc; ++i) { if (!infl_take(B, S, in_len, 3, &v)) return INFL_E_INPUT; T->lens[order[i]] = (uint8_t)v; }
                if (!infl_build(T->lens, 19, T->dcount, T->dsym, T->dfast, 7)) return INFL_E_CODELEN;      // the code-length code borrows the distance tables
                int i = 0;
                while (i < nl + nd) {
                    const int s = infl_symbol(B, S, in_len, T->dcount, T->dsym, 19, T->dfast, 7);
                    if (s < 0) return -s;
                    if (s < 16) { T->lens[19 + i++] = (uint8_t)s; continue; }
                    uint32_t prev = 0, rep;
                    if (s == 16) {
                        if (i == 0) return INFL_E_CODELEN;
                        prev = T->lens[19 + i - 1];
                        if (!infl_take(B, S, in_len, 2, &rep)) return INFL_E_INPUT;
                        rep += 3;
                    } else if (s == 17) { if (!infl_take(B, S, in_len, 3, &rep)) return INFL_E_INPUT; rep += 3; }
                    else { if (!infl_take(B, S, in_len, 7, &rep)) return INFL_E_INPUT; rep += 11; }
                    if (i + (int)rep > nl + nd) return INFL_E_CODELEN;
                    while (rep--) T->lens[19 + i++] = (uint8_t)prev;
                }
                for (int k = 0; k < nl + nd; ++k) T->lens[k] = T->lens[19 + k];          // (moves down: k < 19 + k)
                if (T->lens[256] == 0) return INFL_E_CODELEN;
            }
            if (!infl_build(T->lens, nl, T->lcount, T->lsym, T->lfast, INFL_LBITS)) return INFL_E_CODELEN;
            if (!infl_build(T->lens + nl, nd, T->dcount, T->dsym, T->dfast, INFL_DBITS)) return INFL_E_CODELEN;
            for (;;) {
                const int s = infl_symbol(B, S, in_len, T->lcount, T->lsym, nl, T->lfast, INFL_LBITS);
                if (s < 0) return -s;
                if (s < 256) {
                    if (opos >= isize) return INFL_E_LONG;
                    W.lit(opos, (uint8_t)s); ++opos;
                    continue;
                }
                if (s == 256) break;
                const int ls = s - 257;
                if (ls >= 29) return INFL_E_SYMBOL;
                if (!infl_take(B, S, in_len, infl_len_extra(ls), &v)) return INFL_E_INPUT;
                const uint32_t len = infl_len_base(ls) + v;
                const int ds = infl_symbol(B, S, in_len, T->dcount, T->dsym, nd, T->dfast, INFL_DBITS);
                if (ds < 0) return -ds;
                if (ds >= 30) return INFL_E_SYMBOL;
                if (!infl_take(B, S, in_len, infl_dist_extra(ds), &v)) return INFL_E_INPUT;
                const uint32_t dist = infl_dist_base(ds) + v;
                if (dist > opos) return INFL_E_DIST;
                if (opos + len > isize) return INFL_E_LONG;
                W.match(opos, dist, len);
                opos += len;
            }
        }
        if (last) break;
    }
    return opos == isize ? INFL_OK : INFL_E_SHORT;
}

// ---- CRC-32 of the window by 64 lanes: lane t takes the bytes [n - (64 - t) * 64m, n - (63 - t) * 64m) that exist, m = ceil(n / 4096), so
// that a whole number of 64-byte units lies behind every piece and the writer's table xpow64[k] = x^(8 * 64 * k) moves its register to
// the end: the CRC is ~(XOR over the lanes of infl_crc_lane).  The lane holding byte 0 starts from 0xffffffff, the others from 0.
INFL_HD uint32_t infl_gf2_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) { if (a & m) p ^= b; b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1; }
    return p;
}
INFL_HD uint32_t infl_crc_lane(const uint8_t *win, uint32_t n, int lane, const uint32_t *byte_tab, const uint32_t *xpow64)
{
    const uint32_t m = (n + 4095u) >> 12;                     // <= 16 for n <= 65,536: table index <= 16 * 63 < 1024
    const int64_t full = 64 * (int64_t)m;
    const int64_t hi = (int64_t)n - (63 - lane) * full;
    int64_t lo = hi - full;
    if (hi <= 0) return 0;
    uint32_t s = 0;
    if (lo <= 0) { lo = 0; s = 0xffffffffu; }
    for (int64_t i = lo; i < hi; ++i) s = byte_tab[(s ^ win[i]) & 0xffu] ^ (s >> 8);
    return infl_gf2_mulmod(xpow64[m * (uint32_t)(63 - lane)], s);
}
#endif
