// reads_text_core.h -- FASTA / FASTQ text -> a read set's words: what one record and one word need, as plain functions for host and
// device (the definition is in include/telr_hip.h and, as plain Python, in tests/reads_in_ref.py).  The kernels of
// reads_in.hip.h call them with one lane per record / word; tools/ubench/reads_text_host.cpp calls them in loops on the CPU, under
// the sanitizers.
//
// The text.  `len` bytes that start `bias` bytes (0 .. 15) behind a 16-byte aligned address, with 64 zero bytes behind them inside
// the same allocation.  Every load is a whole aligned qword: a byte is cut out of one, 4 / 8 / 16 bytes at any byte position come
// out of two or three neighbours and a funnel shift.  The last load of the last base ends 23 bytes behind it at the most: the 64 bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

enum { RTS_OK = 0, RTS_NO_AT = 1, RTS_SHORT = 2, RTS_NO_PLUS = 3, RTS_LEN = 4, RTS_QUAL = 5, RTS_LONG = 6, RTS_NONE = 7 };
#define RT_TEXTS { "", "no '@' where a record starts", "the text ends inside the record", "no '+' line behind the bases", \
                   "bases and qualities differ in number", "a quality character outside 33..126", "more than 2^31 - 1 bases", "" }

struct RtText { const uint64_t *q; int64_t bias, len; };
// one record.  seq_pos / qual_pos: text offsets of the first base / quality character; FASTA: first_line = its header line,
// n_lines = the lines behind it, multi = bases on more than the first of them
struct RtRec { int64_t seq_pos, qual_pos; int32_t len, name_len, status, multi; int64_t first_line, n_lines; };

RT_HD uint32_t rt_byte(const RtText &T, int64_t p)
{
    const int64_t k = T.bias + p;
    return (uint32_t)(T.q[k >> 3] >> ((k & 7) * 8)) & 0xffu;
}
RT_HD uint64_t rt_load8(const RtText &T, int64_t p)
{
    const int64_t k = T.bias + p;
    const uint32_t sh = (uint32_t)(k & 7) * 8u;
    const uint64_t a = T.q[k >> 3], b = T.q[(k >> 3) + 1];
    return sh ? (a >> sh) | (b << (64u - sh)) : a;
}
RT_HD void rt_load16(const RtText &T, int64_t p, uint64_t &lo, uint64_t &hi)
{
    const int64_t k = T.bias + p;
    const uint32_t sh = (uint32_t)(k & 7) * 8u;
    const uint64_t a = T.q[k >> 3], b = T.q[(k >> 3) + 1], c = T.q[(k >> 3) + 2];
    lo = sh ? (a >> sh) | (b << (64u - sh)) : a;
    hi = sh ? (b >> sh) | (c << (64u - sh)) : b;
}

// 8 text bytes -> 16 bits of 2-bit codes and 8 mask bits (the arithmetic of pack8 in telr_engine.hip: A C G T/U in either case 0 1 2 3;
// anything else code 0, mask 1)
RT_HD void rt_pack8(uint64_t x, uint32_t &code16, uint32_t &amb8)
{
    const uint64_t L = 0x0101010101010101ULL, H = 0x8080808080808080ULL, M7 = 0x7F7F7F7F7F7F7F7FULL;
    uint64_t t = (x >> 1) & (3 * L);
    t ^= (t >> 1) & L;
    const uint64_t u = x | (0x20 * L);
    uint64_t ok = 0;
    const unsigned char letters[5] = { 'a', 'c', 'g', 't', 'u' };
    for (int i = 0; i < 5; ++i) { const uint64_t v = u ^ (letters[i] * L); ok |= ~(((v & M7) + M7) | v | M7); }
    const uint64_t inv = ~ok & H;
    t &= ~((inv >> 7) * 3);
    t = (t | (t >> 6)) & 0x000F000F000F000FULL;
    t = (t | (t >> 12)) & 0x000000FF000000FFULL;
    t = (t | (t >> 24)) & 0xFFFFULL;
    code16 = (uint32_t)t;
    amb8 = (uint32_t)(((inv >> 7) * 0x0102040810204080ULL) >> 56);
}
// the first v (0 .. 8) bytes of x, 'A' (code 0, mask 0) in the others
RT_HD uint64_t rt_keep(uint64_t x, int v)
{
    const uint64_t m = v >= 8 ? ~0ULL : v <= 0 ? 0ULL : (1ULL << (8 * v)) - 1ULL;
    return (x & m) | (0x4141414141414141ULL & ~m);
}
// 16 text bytes of which the first v (0 .. 16) are bases -> one 2-bit word and its 16 mask bits
RT_HD void rt_pack16(uint64_t lo, uint64_t hi, int v, uint32_t &code, uint32_t &m16)
{
    uint32_t c0, a0, c1, a1;
    rt_pack8(rt_keep(lo, v), c0, a0);
    rt_pack8(rt_keep(hi, v - 8), c1, a1);
    code = c0 | c1 << 16; m16 = a0 | a1 << 8;
}
// 4 quality characters of which the first v (0 .. 4) count -> 4 Phred bytes (zero in the others); *bad: one of them outside 33..126
RT_HD uint32_t rt_qual4(uint32_t x, int v, bool *bad)
{
    uint32_t out = 0; bool b = false;
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = (x >> (8 * i)) & 0xffu, ph = c - 33u;
        const bool in = i < v;
        b |= in && ph > 93u;
        out |= (in ? ph & 0xffu : 0u) << (8 * i);
    }
    *bad = b;
    return out;
}

// line j of a text with nl line feeds: ls[0] = 0, ls[k] = the offset behind the k-th line feed.  -> [*s, *e) without its terminator
// ("\n", "\r\n", or a lone "\r" in front of the text's end)
RT_HD void rt_line(const RtText &T, const int64_t *ls, int64_t nl, int64_t j, int64_t *s, int64_t *e)
{
    const int64_t a = ls[j];
    int64_t b = j < nl ? ls[j + 1] - 1 : T.len;
    if (b > a && rt_byte(T, b - 1) == '\r') --b;
    *s = a; *e = b;
}
// a header line [s, e): the name's length -- the bytes behind the '@' or '>' up to the first space, tab or '\r'
RT_HD int32_t rt_name_len(const RtText &T, int64_t s, int64_t e)
{
    int64_t p = s + 1;
    while (p < e) { const uint32_t c = rt_byte(T, p); if (c == ' ' || c == '\t' || c == '\r') break; ++p; }
    const int64_t n = p - (s + 1);
    return (int32_t)(n > 0x7fffffff ? 0x7fffffff : n);
}
// FASTQ record r of a text of `nlines` lines: lines 4r .. 4r + 3.  RTS_NONE: the text has no line 4r
RT_HD RtRec rt_fastq_record(const RtText &T, const int64_t *ls, int64_t nl, int64_t nlines, int64_t r)
{
    RtRec R; R.seq_pos = R.qual_pos = 0; R.len = R.name_len = 0; R.status = RTS_OK; R.multi = 0; R.first_line = 4 * r; R.n_lines = 1;
    const int64_t have = nlines - 4 * r;
    if (have <= 0) { R.status = RTS_NONE; return R; }
    int64_t s, e;
    rt_line(T, ls, nl, 4 * r, &s, &e);
    if (e == s || rt_byte(T, s) != '@') { R.status = RTS_NO_AT; return R; }
    R.name_len = rt_name_len(T, s, e);
    if (have < 4) { R.status = RTS_SHORT; return R; }
    int64_t s1, e1, s2, e2, s3, e3;
    rt_line(T, ls, nl, 4 * r + 1, &s1, &e1); rt_line(T, ls, nl, 4 * r + 2, &s2, &e2); rt_line(T, ls, nl, 4 * r + 3, &s3, &e3);
    if (e2 == s2 || rt_byte(T, s2) != '+') { R.status = RTS_NO_PLUS; return R; }
    if (e1 - s1 != e3 - s3) { R.status = RTS_LEN; return R; }
    if (e1 - s1 > 0x7fffffffLL) { R.status = RTS_LONG; return R; }
    R.seq_pos = s1; R.qual_pos = s3; R.len = (int32_t)(e1 - s1);
    return R;
}
// FASTA record between header line `first` and the next header line (or the number of lines) `next`; S[j] = the bases on the lines
// before j (a header line has none)
RT_HD RtRec rt_fasta_record(const RtText &T, const int64_t *ls, int64_t nl, const int64_t *S, int64_t first, int64_t next)
{
    RtRec R; R.qual_pos = 0; R.status = RTS_OK; R.first_line = first; R.n_lines = next - first - 1;
    int64_t s, e;
    rt_line(T, ls, nl, first, &s, &e);
    R.name_len = rt_name_len(T, s, e);
    const int64_t n = S[next] - S[first];
    R.seq_pos = R.n_lines > 0 ? ls[first + 1] : 0;
    R.multi = R.n_lines > 0 && S[first + 2] - S[first + 1] != n ? 1 : 0;
    R.len = 0;
    if (n > 0x7fffffffLL) R.status = RTS_LONG; else R.len = (int32_t)n;
    return R;
}
// the FASTA line step: base number A of the text (A = S[first] + the base's index in its record, below S[next]) lies on the last line j
// in (first, next) with S[j] <= A; -> that line, *pos = the base's text offset
RT_HD int64_t rt_fasta_seek(const int64_t *ls, const int64_t *S, int64_t first, int64_t next, int64_t A, int64_t *pos)
{
    int64_t lo = first + 1, hi = next;                       // first line with S > A
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (S[mid] <= A) lo = mid + 1; else hi = mid; }
    const int64_t j = lo - 1;
    *pos = ls[j] + (A - S[j]);
    return j;
}
// 16 bases from base number A on (v of them count), across line ends: whole 16-byte loads where a line holds all that is left, bytes
// over the seams
RT_HD void rt_fasta_gather16(const RtText &T, const int64_t *ls, const int64_t *S, int64_t first, int64_t next, int64_t A, int v, uint64_t &lo, uint64_t &hi)
{
    int64_t pos;
    int64_t j = rt_fasta_seek(ls, S, first, next, A, &pos);
    if (S[j + 1] - A >= v) { rt_load16(T, pos, lo, hi); return; }
    lo = hi = 0;
    int64_t end = ls[j] + (S[j + 1] - S[j]);
    for (int b = 0; b < v; ++b) {
        while (pos >= end) { ++j; pos = ls[j]; end = pos + (S[j + 1] - S[j]); }          // (A + b < S[next]: a line with bases follows)
        const uint64_t c = rt_byte(T, pos++);
        if (b < 8) lo |= c << (8 * b); else hi |= c << (8 * (b - 8));
    }
}
