// bam_in.hip.h -- a BAM file becomes what the stage-1 consumers take, on the device (the definition is in
// include/telr_hip.h and, as plain Python, in tests/bam_in_ref.py).  Here: the kernels, the hop over the file, the header, what the host
// decides, and the handle.  The load itself -- one load for telr_bam_load and telr_bam_load_chunked: the whole file is the plan of one
// chunk -- is bam_load in bam_in_chunked.hip.h.  Per chunk:
//
//   host      (once) map the file, hop the BGZF member headers -> table of (deflate bytes, their length, ISIZE, CRC)
//   device    k_bgzf_inflate   one workgroup (one wave) per member: RFC 1951 into a 64-KiB window in LDS, CRC-32, window -> buffer
//   host      the BAM header (copied back: it is small)
//   device    k_bam_chain      the record offsets: record i + 1 starts block_size(i) behind record i -- one lane walks
//             k_bam_rec        one wave per record: fixed fields, tags, CIGAR rules (count pass), name length
//             k_bam_names      the names into one compact buffer
//   host      (once, all chunks' records) names -> read numbers (hash map), which records are kept, their order and CIGAR offsets
//   device    k_bam_cig        the normalised CIGAR words of the kept records (emit pass) into the result's device array
//             k_bam_seq / k_bam_qual   the reads' 2-bit words, mask words and Phred bytes in the set's layout
//             k_bam_ascii      the set as text, on demand
// Every store position is a scan's or the lane's own index; there is no atomic; the bytes are the same on every run.
//
// The window is in LDS, not in the member's global output: a match copy reads what the symbol before it wrote, and the turn-around
// of an LDS store -> load inside one wave is some hundred cycles where a global one is a microsecond or more.  64 KiB of window +
// 2 KiB of input + 4.6 KiB of tables leave two workgroups per CU (160 KiB); the decoder is latency-bound either way, the window is
// what keeps the latency short.
#include "inflate_core.h"

#define BGZF_INCH 2048          /* bytes of compressed input staged in LDS */

struct BgzfMember { int64_t off; uint32_t clen, isize, crc, pad; };          // off: file offset of the deflate bytes

struct BgzfSrc {
    const uint32_t *file4;      // the file as aligned dwords (padded behind its end by BGZF_INCH + 8 bytes)
    int64_t off;                // file offset of the member's deflate bytes
    uint32_t *buf;              // LDS [BGZF_INCH / 4]
    int64_t base;               // file offset of buf[0] (a multiple of 4), -1: nothing staged
    __device__ __forceinline__ void stage(int64_t a)
    {
        if (a >= base && a + 8 <= base + BGZF_INCH && base >= 0) return;
        base = a & ~(int64_t)3;
        __syncthreads();
        for (int k = threadIdx.x; k < BGZF_INCH / 4; k += 64) buf[k] = file4[(base >> 2) + k];
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t get32(uint32_t pos)
    {
        const int64_t a = off + pos;
        stage(a);
        const uint32_t i = (uint32_t)(a - base), w = i >> 2, sh = (i & 3u) * 8u;
        const uint32_t lo = buf[w];
        return sh ? (lo >> sh) | (buf[w + 1] << (32u - sh)) : lo;
    }
    __device__ __forceinline__ uint32_t get8(uint32_t pos)
    {
        const int64_t a = off + pos;
        stage(a);
        const uint32_t i = (uint32_t)(a - base);
        return (buf[i >> 2] >> ((i & 3u) * 8u)) & 0xffu;
    }
};
// All 64 lanes run the symbol loop in step (same bits, same tables, same positions): a literal is stored by every lane (same byte, same
// address), a copy is shared out over the lanes and fenced by a barrier before the next symbol may read it.
struct BgzfSink {
    uint8_t *win;               // LDS [65536]
    const uint8_t *in;          // the member's deflate bytes in the file
    __device__ __forceinline__ void lit(uint32_t pos, uint8_t b) { win[pos] = b; }
    __device__ __forceinline__ void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        // every source byte lies before pos: it exists; distance < length repeats the last `dist` bytes
        for (uint32_t i = threadIdx.x; i < len; i += 64) win[pos + i] = win[pos - dist + (dist >= len ? i : i % dist)];
        __syncthreads();
    }
    __device__ __forceinline__ void stored(uint32_t pos, uint32_t ipos, uint32_t len)
    {
        for (uint32_t i = threadIdx.x; i < len; i += 64) win[pos + i] = in[ipos + i];
        __syncthreads();
    }
};

// one workgroup of one wave per member.  status[m] = INFL_*; the member's bytes reach `out` only when it is INFL_OK.
__global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t *__restrict__ file, const BgzfMember *__restrict__ mem, const int64_t *__restrict__ out_off,
                                                     const CrcTabs *__restrict__ CT, uint8_t *__restrict__ out, int32_t *__restrict__ status)
{
    __shared__ uint32_t win4[65536 / 4];
    __shared__ uint32_t inbuf[BGZF_INCH / 4];
    __shared__ InflTables T;
    __shared__ uint32_t tab[256];
    const int lane = threadIdx.x;
    const BgzfMember M = mem[blockIdx.x];
    uint8_t *win = (uint8_t*)win4;
    for (int k = lane; k < 256; k += 64) tab[k] = CT->byte_tab[k];
    BgzfSrc S; S.file4 = (const uint32_t*)file; S.off = M.off; S.buf = inbuf; S.base = -1;
    BgzfSink W; W.win = win; W.in = file + M.off;
    int st = M.isize <= 65536u ? infl_member(S, M.clen, M.isize, &T, W) : INFL_E_LONG;
    __syncthreads();
    if (st == INFL_OK) {
        uint32_t c = infl_crc_lane(win, M.isize, lane, tab, CT->xpow64);
        for (int o = 32; o >= 1; o >>= 1) c ^= (uint32_t)__shfl_xor((int)c, o);
        if ((M.isize ? ~c : 0u) != M.crc) st = INFL_E_CRC;
    }
    if (lane == 0) status[blockIdx.x] = st;
    if (st != INFL_OK) return;
    // window -> stream: bytes up to the first aligned dword, dwords, bytes
    uint8_t *d = out + out_off[blockIdx.x];
    const uint32_t n = M.isize;
    uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    if (head > n) head = n;
    if ((uint32_t)lane < head) d[lane] = win[lane];
    const uint32_t nd = (n - head) >> 2;
    uint32_t *d4 = (uint32_t*)(d + head);
    for (uint32_t k = lane; k < nd; k += 64) {
        const uint8_t *s = win + head + 4 * k;
        d4[k] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
    }
    const uint32_t t0 = head + 4 * nd;
    if (t0 + lane < n) d[t0 + lane] = win[t0 + lane];
}

// ---- records ----------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint32_t bi_ld32(const uint8_t *__restrict__ s, int64_t p)
{
    return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8 | (uint32_t)s[p + 2] << 16 | (uint32_t)s[p + 3] << 24;
}
static __device__ __forceinline__ uint32_t bi_ld16(const uint8_t *__restrict__ s, int64_t p) { return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8; }

// res[0] = records, res[1] = 0 | 1 (record res[0] runs past the buffer) | 2 (its block_size is below 32) | 3 (more records than `cap`),
// res[2] = where the walk ended -- behind the last complete record: the next chunk's carry starts there
__global__ void __launch_bounds__(64) k_bam_chain(const uint8_t *__restrict__ stream, int64_t total, int64_t start, int64_t *__restrict__ offs, int64_t cap,
                                                  int64_t *__restrict__ res)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t p = start, n = 0, st = 0;
    while (p < total) {
        if (p + 4 > total) { st = 1; break; }
        const int32_t bs = (int32_t)bi_ld32(stream, p);
        if (bs < 32) { st = 2; break; }
        if (p + 4 + (int64_t)bs > total) { st = 1; break; }
        if (n >= cap) { st = 3; break; }
        offs[n++] = p;
        p += 4 + (int64_t)bs;
    }
    res[0] = n; res[1] = st; res[2] = p;
}

enum { BREC_OK = 0, BREC_FIELDS = 1, BREC_TAGS = 2, BREC_REF = 3, BREC_CLIP = 4, BREC_OP = 5, BREC_RANGE = 6 };
struct BamRec {
    int64_t seq_off, cig_src;          // stream offsets of SEQ and of the CIGAR words in force (the record's own or the CG array)
    int32_t n_raw;                     // their number
    int32_t refid, pos, flag, mapq, lseq, name_len, status;
    int32_t clip5, clip3, sm, si, sd, n_norm;
    int32_t has_nm, nm, as, cm, s1, s2;
    int32_t qual0, pad;
};

struct CigWalk { int32_t status; int64_t clip5, clip3, sm, si, sd; int32_t n_norm; };

// The CIGAR rules over n raw words at stream offset c0 (any byte alignment), one wave, 64 words per step.  EMIT: the normalised words go
// to out[0 .. n_norm); a run of equal ops is written once it ends -- by the lane of its first op inside a step, by lane 0 where it crossed
// the 64-word seam (the open run is carried: type, sum, slot).
template <bool EMIT>
static __device__ __forceinline__ CigWalk bam_cigar_walk(const uint8_t *__restrict__ s, int64_t c0, int32_t n, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    CigWalk R; R.status = BREC_OK; R.clip5 = R.clip3 = R.sm = R.si = R.sd = 0; R.n_norm = 0;
    int32_t i = 0, j = n;
    if (i < j) { const uint32_t w = bi_ld32(s, c0 + 4 * (int64_t)i); if ((w & 15u) == 5u) { R.clip5 += w >> 4; ++i; } }
    if (i < j) { const uint32_t w = bi_ld32(s, c0 + 4 * (int64_t)i); if ((w & 15u) == 4u) { R.clip5 += w >> 4; ++i; } }
    if (j > i) { const uint32_t w = bi_ld32(s, c0 + 4 * (int64_t)(j - 1)); if ((w & 15u) == 5u) { R.clip3 += w >> 4; --j; } }
    if (j > i) { const uint32_t w = bi_ld32(s, c0 + 4 * (int64_t)(j - 1)); if ((w & 15u) == 4u) { R.clip3 += w >> 4; --j; } }
    int carry_type = -1; int64_t carry_sum = 0; int32_t carry_slot = 0, n_out = 0;
    int64_t acc0 = 0, acc1 = 0, acc2 = 0;
    bool range = false;
    for (int32_t base = i; base < j; base += 64) {
        const int32_t k = base + lane;
        const bool valid = k < j;
        const uint32_t w = valid ? bi_ld32(s, c0 + 4 * (int64_t)k) : 0u;
        const uint32_t op = w & 15u, len = w >> 4;
        int m = -1, e = 0;
        if (valid) {
            if (op > 8u) e = BREC_OP;
            else if (op == 4u || op == 5u) e = BREC_CLIP;
            else if (op != 6u && len != 0u) m = (op == 1u) ? 1 : (op == 2u || op == 3u) ? 2 : 0;
        }
        const uint64_t bad = __ballot(e != 0);
        if (bad) { R.status = __shfl(e, __ffsll((long long)bad) - 1); return R; }          // the first offending op, as the serial walk meets it
        const uint64_t surv = __ballot(m >= 0), t0 = __ballot(m == 0), t1 = __ballot(m == 1);
        const uint64_t below = surv & ((1ull << lane) - 1ull);
        int prev = carry_type;
        if (below) { const int pl = 63 - __clzll((long long)below); prev = (t0 >> pl & 1ull) ? 0 : (t1 >> pl & 1ull) ? 1 : 2; }
        const bool head = m >= 0 && prev != m;
        const uint64_t heads = __ballot(head);
        const int64_t L = m >= 0 ? (int64_t)len : 0;
        if (m == 0) acc0 += L; else if (m == 1) acc1 += L; else if (m == 2) acc2 += L;
        const int64_t P = d_wave_incl<int64_t>(L, lane);
        const int64_t tot = __shfl(P, 63);
        if (!heads) { carry_sum += tot; continue; }
        const int fh = __ffsll((long long)heads) - 1;
        const int64_t before = fh > 0 ? __shfl(P, fh - 1) : 0;   // survivors before the first head continue the carried run
        if (carry_type >= 0) {
            const int64_t v = carry_sum + before;
            if (v >= (1ll << 28)) range = true;
            else if (EMIT && lane == 0) out[carry_slot] = (uint32_t)v << 4 | (uint32_t)carry_type;
        }
        // runs that start in this step
        const uint64_t above = heads & ~((2ull << lane) - 1ull);          // (lane 63: 2 << 63 wraps to 0, minus 1 = all ones: no head above)
        const int h2 = above ? __ffsll((long long)above) - 1 : 64;
        const int64_t pm1 = __shfl_up(P, 1);
        const int64_t endv = __shfl(P, h2 < 64 ? h2 - 1 : 63);
        const int64_t mine = endv - (lane > 0 ? pm1 : 0);
        const int32_t slot = n_out + __popcll(heads & ((1ull << lane) - 1ull));
        if (head && h2 < 64) {
            if (mine >= (1ll << 28)) range = true;
            else if (EMIT) out[slot] = (uint32_t)mine << 4 | (uint32_t)m;
        }
        range = __ballot(range) != 0;
        const int lh = 63 - __clzll((long long)heads);
        carry_type = __shfl(m, lh); carry_sum = __shfl(mine, lh); carry_slot = __shfl(slot, lh);
        n_out += __popcll(heads);
    }
    if (carry_type >= 0) {
        if (carry_sum >= (1ll << 28)) range = true;
        else if (EMIT && lane == 0) out[carry_slot] = (uint32_t)carry_sum << 4 | (uint32_t)carry_type;
    }
    for (int o = 32; o >= 1; o >>= 1) { acc0 += __shfl_xor(acc0, o); acc1 += __shfl_xor(acc1, o); acc2 += __shfl_xor(acc2, o); }
    R.sm = acc0; R.si = acc1; R.sd = acc2; R.n_norm = n_out;
    if (range || R.sm + R.si + R.sd + R.clip5 + R.clip3 >= (1ll << 31)) R.status = BREC_RANGE;
    return R;
}

// first NUL in s[p .. p + n), or n: 64 bytes per step
static __device__ __forceinline__ int64_t bi_find_nul(const uint8_t *__restrict__ s, int64_t p, int64_t n)
{
    const int lane = threadIdx.x & 63;
    for (int64_t b = 0; b < n; b += 64) {
        const uint64_t z = __ballot(b + lane < n && s[p + b + lane] == 0);
        if (z) return b + __ffsll((long long)z) - 1;
    }
    return n;
}

// one wave per record
__global__ void __launch_bounds__(256) k_bam_rec(const uint8_t *__restrict__ stream, const int64_t *__restrict__ offs, int64_t nrec, int32_t n_ref,
                                                 BamRec *__restrict__ recs, int32_t *__restrict__ name_len)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (r >= nrec) return;
    const int64_t p = offs[r];
    const int64_t bs = (int32_t)bi_ld32(stream, p), end = p + 4 + bs;          // the chain held it to >= 32 and to the stream
    BamRec B;
    B.refid = (int32_t)bi_ld32(stream, p + 4); B.pos = (int32_t)bi_ld32(stream, p + 8);
    const int32_t lrn = stream[p + 12]; B.mapq = stream[p + 13];
    const int32_t ncig = (int32_t)bi_ld16(stream, p + 16); B.flag = (int32_t)bi_ld16(stream, p + 18);
    B.lseq = (int32_t)bi_ld32(stream, p + 20);
    B.status = BREC_OK; B.name_len = 0; B.seq_off = 0; B.cig_src = 0; B.n_raw = 0; B.clip5 = B.clip3 = B.sm = B.si = B.sd = B.n_norm = 0;
    B.has_nm = B.nm = B.as = B.cm = B.s1 = B.s2 = 0; B.qual0 = 0xff; B.pad = 0;
    const int64_t lseq = B.lseq;
    if (lrn < 1 || lseq < 0 || 36 + (int64_t)lrn + 4 * (int64_t)ncig + (lseq + 1) / 2 + lseq > 4 + bs) B.status = BREC_FIELDS;
    if (B.status == BREC_OK) {
        const int64_t cig_off = p + 36 + lrn, seq_off = cig_off + 4 * (int64_t)ncig, qual_off = seq_off + (lseq + 1) / 2;
        B.name_len = (int32_t)bi_find_nul(stream, p + 36, lrn - 1);
        B.seq_off = seq_off;
        if (lseq > 0) B.qual0 = stream[qual_off];
        // the tags, one after the other (every lane walks them in step)
        int64_t t = qual_off + lseq, cg_off = -1; int32_t cg_n = 0;
        while (t < end) {
            if (t + 3 > end) { B.status = BREC_TAGS; break; }
            const uint32_t t0 = stream[t], t1 = stream[t + 1], ty = stream[t + 2];
            t += 3;
            int sz = 0; bool isint = false; int64_t v = 0;
            switch (ty) {
                case 'A': sz = 1; break;
                case 'c': sz = 1; isint = true; break; case 'C': sz = 1; isint = true; break;
                case 's': sz = 2; isint = true; break; case 'S': sz = 2; isint = true; break;
                case 'i': sz = 4; isint = true; break; case 'I': sz = 4; isint = true; break;
                case 'f': sz = 4; break;
                default: break;
            }
            if (sz) {
                if (t + sz > end) { B.status = BREC_TAGS; break; }
                if (isint) {
                    if (ty == 'c') v = (int8_t)stream[t]; else if (ty == 'C') v = stream[t];
                    else if (ty == 's') v = (int16_t)bi_ld16(stream, t); else if (ty == 'S') v = bi_ld16(stream, t);
                    else v = (int32_t)bi_ld32(stream, t);          // 'I' above 2^31 - 1 wraps: a tag is truncated to 32 bits
                    const int32_t x = (int32_t)v;
                    if (t0 == 'N' && t1 == 'M') { B.has_nm = 1; B.nm = x; }
                    else if (t0 == 'A' && t1 == 'S') B.as = x;
                    else if (t0 == 'c' && t1 == 'm') B.cm = x;
                    else if (t0 == 's' && t1 == '1') B.s1 = x;
                    else if (t0 == 's' && t1 == '2') B.s2 = x;
                }
                t += sz;
            } else if (ty == 'Z' || ty == 'H') {
                const int64_t z = bi_find_nul(stream, t, end - t);
                if (z == end - t) { B.status = BREC_TAGS; break; }
                t += z + 1;
            } else if (ty == 'B') {
                if (t + 5 > end) { B.status = BREC_TAGS; break; }
                const uint32_t sub = stream[t]; const int64_t cnt = bi_ld32(stream, t + 1);
                const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                if (!es || t + 5 + cnt * es > end) { B.status = BREC_TAGS; break; }
                if (t0 == 'C' && t1 == 'G' && sub == 'I') { cg_off = t + 5; cg_n = (int32_t)cnt; }          // (cnt * 4 fits the record: below 2^29)
                t += 5 + cnt * es;
            } else { B.status = BREC_TAGS; break; }
        }
        const bool mapped = !(B.flag & 4) && B.refid >= 0;
        if (B.status == BREC_OK && mapped) {
            if (B.refid >= n_ref || B.pos < 0) B.status = BREC_REF;
            else {
                B.cig_src = cig_off; B.n_raw = ncig;
                if (ncig == 2 && cg_off >= 0) {
                    const uint32_t w0 = bi_ld32(stream, cig_off), w1 = bi_ld32(stream, cig_off + 4);
                    if ((uint64_t)w0 == ((uint64_t)lseq << 4 | 4u) && (w1 & 15u) == 3u) { B.cig_src = cg_off; B.n_raw = cg_n; }
                }
                const CigWalk Wk = bam_cigar_walk<false>(stream, B.cig_src, B.n_raw, nullptr);
                B.status = Wk.status;
                if (B.status == BREC_OK && (int64_t)B.pos + Wk.sm + Wk.sd >= (1ll << 31)) B.status = BREC_RANGE;
                if (B.status == BREC_OK) {
                    B.clip5 = (int32_t)Wk.clip5; B.clip3 = (int32_t)Wk.clip3; B.sm = (int32_t)Wk.sm; B.si = (int32_t)Wk.si; B.sd = (int32_t)Wk.sd;
                    B.n_norm = Wk.n_norm;
                }
            }
        }
    }
    if (lane == 0) { recs[r] = B; name_len[r] = B.status == BREC_FIELDS ? 0 : B.name_len; }
}

__global__ void __launch_bounds__(256) k_bam_names(const uint8_t *__restrict__ stream, const int64_t *__restrict__ offs, int64_t nrec,
                                                   const int32_t *__restrict__ name_len, const int64_t *__restrict__ name_off, uint8_t *__restrict__ names)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (r >= nrec) return;
    const int32_t n = name_len[r];
    const int64_t src = offs[r] + 36, dst = name_off[r];
    for (int32_t k = lane; k < n; k += 64) names[dst + k] = stream[src + k];
}

// emit pass: the kept records' normalised words at the offsets the host's scan gave them.  kept[k] = record, cig_off[k] = its first word
__global__ void __launch_bounds__(256) k_bam_cig(const uint8_t *__restrict__ stream, const BamRec *__restrict__ recs, const int32_t *__restrict__ kept,
                                                 const int64_t *__restrict__ cig_off, int64_t nkept, uint32_t *__restrict__ cig)
{
    const int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (k >= nkept) return;
    const BamRec B = recs[kept[k]];
    (void)bam_cigar_walk<true>(stream, B.cig_src, B.n_raw, cig + cig_off[k]);
}

// ---- reads ------------------------------------------------------------------------------------------------------------------------
struct BamRead { int64_t seq_off, qual_off; int32_t len, rev; };

// base j of the read as the set holds it: 2-bit code, or 4 for N.  SEQ: two bases per byte, the first in the high nibble
static __device__ __forceinline__ uint32_t bam_base(const uint8_t *__restrict__ stream, const BamRead R, int32_t j)
{
    const int32_t x = R.rev ? R.len - 1 - j : j;
    const uint32_t b = stream[R.seq_off + (x >> 1)];
    const uint32_t nib = (x & 1) ? b & 15u : b >> 4;
    const uint32_t c = nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u;
    return (R.rev && c < 4u) ? 3u - c : c;
}
static __device__ __forceinline__ int32_t bam_read_of(const int64_t *__restrict__ boff, int32_t n, int64_t b0)
{
    int32_t lo = 0, hi = n;                                   // first read with boff > b0
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (boff[mid] <= b0) lo = mid + 1; else hi = mid; }
    return lo - 1;
}
// one lane per 2-bit word (16 bases) of the set's layout; the mask words from lane pairs (nw is even: reads are padded to 64 bases)
static __device__ __forceinline__ void bam_seq_word(const uint8_t *__restrict__ stream, const BamRead *__restrict__ reads, const int64_t *__restrict__ boff, int32_t n,
                                                    int64_t w, uint32_t *__restrict__ out2, uint32_t *__restrict__ outn)
{
    const int64_t b0 = w * 16;
    const int32_t q = bam_read_of(boff, n, b0);
    const BamRead R = reads[q];
    const int64_t j0 = b0 - boff[q];
    uint32_t code = 0, m16 = 0;
    for (int b = 0; b < 16; ++b) {
        if (j0 + b >= R.len) break;
        const uint32_t c = bam_base(stream, R, (int32_t)(j0 + b));
        if (c == 4u) m16 |= 1u << b; else code |= c << (2 * b);
    }
    out2[w] = code;
    const uint32_t other = __shfl_xor(m16, 1);
    if (!(w & 1)) outn[w >> 1] = m16 | (other << 16);
}
// words [w0, w1) of the set's layout, both multiples of 4: the reads first met in one chunk; reads / boff start at the chunk's first read
__global__ void __launch_bounds__(256) k_bam_seq(const uint8_t *__restrict__ stream, const BamRead *__restrict__ reads, const int64_t *__restrict__ boff, int32_t n,
                                                 int64_t w0, int64_t w1, uint32_t *__restrict__ out2, uint32_t *__restrict__ outn)
{
    const int64_t w = w0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= w1) return;
    bam_seq_word(stream, reads, boff, n, w, out2, outn);
}
// one lane per 4 Phred bytes of the set's base layout (zero behind a read's end); over[q] = 1 for a read with a value above 93 (the same 1 from whichever lane meets one)
static __device__ __forceinline__ void bam_qual_word(const uint8_t *__restrict__ stream, const BamRead *__restrict__ reads, const int64_t *__restrict__ boff, int32_t n,
                                                     int64_t w, uint32_t *__restrict__ out4, int32_t *__restrict__ over)
{
    const int64_t b0 = w * 4;
    const int32_t q = bam_read_of(boff, n, b0);
    const BamRead R = reads[q];
    const int64_t j0 = b0 - boff[q];
    uint32_t v = 0; bool big = false;
    for (int b = 0; b < 4; ++b) {
        if (j0 + b >= R.len) break;
        const int32_t x = R.rev ? R.len - 1 - (int32_t)(j0 + b) : (int32_t)(j0 + b);
        const uint32_t ph = stream[R.qual_off + x];
        big |= ph > 93u;
        v |= ph << (8 * b);
    }
    out4[w] = v;
    if (big) over[q] = 1;
}
__global__ void __launch_bounds__(256) k_bam_qual(const uint8_t *__restrict__ stream, const BamRead *__restrict__ reads, const int64_t *__restrict__ boff, int32_t n,
                                                  int64_t w0, int64_t w1, uint32_t *__restrict__ out4, int32_t *__restrict__ over)
{
    const int64_t w = w0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= w1) return;
    bam_qual_word(stream, reads, boff, n, w, out4, over);
}
// the set as text: one lane per 4 bases of the padded layout, stored where the compact text has them (coff[q] = bases before read q)
__global__ void __launch_bounds__(256) k_bam_ascii(const uint32_t *__restrict__ seq2, const uint32_t *__restrict__ nmask, const int64_t *__restrict__ boff,
                                                   const int32_t *__restrict__ len, const int64_t *__restrict__ coff, int32_t n, int64_t nq4, uint8_t *__restrict__ text)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nq4) return;
    const int64_t b0 = w * 4;
    const int32_t q = bam_read_of(boff, n, b0);
    const int64_t j0 = b0 - boff[q];
    const int32_t L = len[q];
    if (j0 >= L) return;
    const uint32_t c8 = (seq2[b0 >> 4] >> (2 * (b0 & 15))) & 0xffu, m4 = (nmask[b0 >> 5] >> (b0 & 31)) & 0xfu;
    uint8_t *d = text + coff[q] + j0;
    for (int b = 0; b < 4 && j0 + b < L; ++b) d[b] = (m4 >> b & 1u) ? 'N' : "ACGT"[(c8 >> (2 * b)) & 3u];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <unordered_map>

enum { BIN_HOP, BIN_UPLOAD, BIN_INFLATE, BIN_CHAIN, BIN_PARSE, BIN_NAMES_HOST, BIN_SEQ, BIN_TOTAL, BIN_NPHASE };
struct telr_bam_in {
    telr_ctx *ctx = nullptr;
    std::vector<std::string> tnames, qnames;
    std::vector<const char*> tname_ptr, qname_ptr;
    std::vector<int32_t> tlens;
    telr_seqset *set = nullptr; telr_result *res = nullptr;
    bool set_owned = true, res_owned = true;
    int64_t counters[9] = {0};
    float phase_ms[BIN_NPHASE] = {0};
    int64_t chunk_info[4] = {0};       // telr_bam_load_chunked: chunks, passes, largest chunk buffer, largest carry (telr_bam_load leaves them 0)
    int64_t region_info[6] = {0};      // telr_bam_load_regions: merged regions, intervals, their members, header members, records walked, selected
    int64_t region_bytes = 0;          // ... and the file bytes it uploaded, both passes
};
struct BamInClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    float lap() { const auto n = std::chrono::steady_clock::now(); const float ms = std::chrono::duration<float, std::milli>(n - t).count(); t = n; return ms; }
};
struct BamInFile {
    int fd = -1; const uint8_t *p = nullptr; size_t n = 0;
    ~BamInFile() { if (p && n) munmap((void*)p, n); if (fd >= 0) close(fd); }
};
static const char *const BGZF_EOF28 = "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00";
static const char *infl_text(int st)
{
    static const char *const T[] = { "ok", "the deflate stream reads past its member", "deflate block type 3", "stored block: LEN / NLEN disagree",
                                     "invalid code-length set", "invalid code or symbol", "distance before the member's start", "more output than ISIZE",
                                     "less output than ISIZE", "CRC-32 mismatch" };
    return st >= 0 && st <= 9 ? T[st] : "?";
}

// the mapped file and its member table (host only): what a load starts from
struct BamInHop {
    BamInFile F;
    std::vector<BgzfMember> mem; std::vector<int32_t> isz;      // mem[k].off: file offset of member k's deflate bytes
    int64_t total = 0, no_eof = 0;                              // sum of ISIZE; 1 without the EOF marker
    float ms = 0;
};
// one member's header at file offset p of the mapped file: nullptr and M, bsize (the member's whole length), or why it is none
static const char *bgzf_member_at(const uint8_t *d, size_t size, size_t p, BgzfMember &M, size_t &bsize)
{
    if (p + 12 > size) return "truncated member";
    if (d[p] != 0x1f || d[p + 1] != 0x8b || d[p + 2] != 8 || d[p + 3] != 4) return "not a BGZF member (wrong magic, or bytes after the last member)";
    const size_t xlen = (size_t)d[p + 10] | (size_t)d[p + 11] << 8;
    if (p + 12 + xlen > size) return "truncated member";
    size_t q = p + 12; bsize = 0;
    while (q + 4 <= p + 12 + xlen) {
        const size_t slen = (size_t)d[q + 2] | (size_t)d[q + 3] << 8;
        if (d[q] == 'B' && d[q + 1] == 'C' && slen == 2 && q + 6 <= p + 12 + xlen) { bsize = ((size_t)d[q + 4] | (size_t)d[q + 5] << 8) + 1; break; }
        q += 4 + slen;
    }
    if (!bsize) return "no BC subfield";
    if (bsize < 12 + xlen + 8) return "BSIZE smaller than the member's own fields";
    if (p + bsize > size) return "truncated member";
    const uint8_t *t = d + p + bsize - 8;
    M.off = (int64_t)(p + 12 + xlen); M.clen = (uint32_t)(bsize - 12 - xlen - 8); M.pad = 0;
    M.crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    M.isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    if (M.isize > 65536u) return "ISIZE above 65,536";
    return nullptr;
}
// the file, mapped; H.no_eof
static int bam_in_open(telr_ctx *ctx, const char *what, const char *path, BamInHop &H)
{
    BamInFile &F = H.F;
    F.fd = open(path, O_RDONLY);
    struct stat sb;
    if (F.fd < 0 || fstat(F.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { ctx->err = std::string(what) + ": cannot open " + path; return TELR_E_IO; }
    F.n = (size_t)sb.st_size;
    if (F.n) { void *m = mmap(nullptr, F.n, PROT_READ, MAP_PRIVATE, F.fd, 0); if (m == MAP_FAILED) { F.n = 0; ctx->err = std::string(what) + ": cannot map " + path; return TELR_E_IO; } F.p = (const uint8_t*)m; }
    H.no_eof = (F.n >= 28 && !memcmp(F.p + F.n - 28, BGZF_EOF28, 28)) ? 0 : 1;
    return TELR_OK;
}
static int bam_in_hop(telr_ctx *ctx, const char *what, const char *path, BamInHop &H)
{
    BamInClock clk;
    TRY(bam_in_open(ctx, what, path, H));
    const uint8_t *d = H.F.p; const size_t size = H.F.n;
    // hop the member headers
    std::vector<BgzfMember> &mem = H.mem; std::vector<int32_t> &isz = H.isz;
    size_t p = 0;
    while (p < size) {
        BgzfMember M; size_t bsize = 0;
        if (const char *why = bgzf_member_at(d, size, p, M, bsize)) { ctx->err = std::string(what) + ": block " + std::to_string(mem.size()) + ": " + why; return TELR_E_ARG; }
        mem.push_back(M); isz.push_back((int32_t)M.isize);
        p += bsize;
    }
    const size_t nm = mem.size();
    if (nm >= 0x7ffffff0u) { ctx->err = std::string(what) + ": too many BGZF members"; return TELR_E_RANGE; }
    H.total = 0;
    for (size_t k = 0; k < nm; ++k) H.total += mem[k].isize;
    H.ms = clk.lap();
    return TELR_OK;
}

// test tap: the Phred bytes of a set in its base layout (padded_bases of them) -> out; returns their number, -1 without qualities
extern "C" int64_t telr_debug_seqset_qual(const telr_seqset *s, uint8_t *out, int64_t cap)
{
    if (!s || !s->d_qual || !out || cap < s->padded_bases) return -1;
    if (s->padded_bases && hipMemcpy(out, s->d_qual, (size_t)s->padded_bases, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return s->padded_bases;
}

// the BAM header in the first `have` bytes of the stream: TELR_OK (start = first record), 1 = needs `*need` bytes, or an error
static int bam_in_header(telr_ctx *ctx, const uint8_t *h, int64_t have, int64_t total, telr_bam_in *B, int64_t *start, int64_t *need)
{
    auto bad = [&](const char *why) { ctx->err = std::string("telr_bam_load: header: ") + why; return TELR_E_ARG; };
    auto rd = [&](int64_t p) { return (int32_t)((uint32_t)h[p] | (uint32_t)h[p + 1] << 8 | (uint32_t)h[p + 2] << 16 | (uint32_t)h[p + 3] << 24); };
#define BIN_NEED(p_, n_, what_) do { if ((p_) + (n_) > total) return bad(what_ " runs past the stream"); if ((p_) + (n_) > have) { *need = (p_) + (n_); return 1; } } while (0)
    BIN_NEED(0, 12, "magic");
    if (memcmp(h, "BAM\1", 4)) return bad("no BAM magic");
    const int64_t l_text = rd(4);
    if (l_text < 0) return bad("negative text length");
    BIN_NEED(8, l_text + 4, "text");
    int64_t p = 8 + l_text;
    const int64_t n_ref = rd(p); p += 4;
    if (n_ref < 0) return bad("negative reference count");
    B->tnames.clear(); B->tlens.clear();
    for (int64_t i = 0; i < n_ref; ++i) {
        BIN_NEED(p, 4, "reference");
        const int64_t ln = rd(p);
        if (ln < 1) return bad("reference name length");
        BIN_NEED(p + 4, ln + 4, "reference");
        const char *nmp = (const char*)h + p + 4;
        B->tnames.emplace_back(nmp, strnlen(nmp, (size_t)ln - 1)); B->tlens.push_back(rd(p + 4 + ln));
        p += 8 + ln;
    }
#undef BIN_NEED
    *start = p;
    return TELR_OK;
}

extern "C" void telr_bam_in_free(telr_bam_in *in)
{
    if (!in) return;
    if (in->set && in->set_owned) telr_seqset_free(in->set);
    if (in->res && in->res_owned) telr_result_free(in->res);
    delete in;
}

// ---- what the host decides from the records' fields and names (the whole file's records, in file order) ----
// the first of recs[0 .. n) that breaks a rule; recs[k] is the load's record base + k, and who(base + k) is how the text names it
template <class Who>
static int bam_in_rec_fault(telr_ctx *ctx, const BamRec *recs, int64_t n, int64_t base, Who who)
{
    for (int64_t k = 0; k < n; ++k) {
        const int s = recs[k].status;
        if (s == BREC_OK) continue;
        static const char *const why[] = { "", "fields run past the record", "malformed tags", "refID or pos outside the header's references",
                                           "a clip inside the CIGAR", "CIGAR op code above 8", "CIGAR lengths beyond the record's coordinate bits" };
        ctx->err = "telr_bam_load: record " + who(base + k) + ": " + why[s >= 1 && s <= 6 ? s : 0];
        return s == BREC_RANGE ? TELR_E_RANGE : TELR_E_ARG;
    }
    return TELR_OK;
}
struct BamInDecided {
    std::vector<BamRead> reads; std::vector<int32_t> rlen, first_rec;      // read q: where its bases are, its length, its record
    bool any_ff = false;                                                   // a sequence-bearing record without QUAL
    std::vector<int32_t> kept_rec; std::vector<int64_t> kept_off;          // the kept records in the result's order; their first CIGAR word
    int64_t ncig = 0;
    std::unique_ptr<telr_result> R;                                        // alns filled in, no CIGAR array yet
};
// names -> read numbers (first name wins), which records are kept, their order, their result records; B: qnames and counters 1 .. 7
static int bam_in_decide(telr_ctx *ctx, telr_bam_in *B, const std::vector<BamRec> &recs, const std::vector<char> &names, const std::vector<int64_t> &noff, BamInDecided &D)
{
    const int64_t nrec = (int64_t)recs.size();
    std::unordered_map<std::string, int32_t> qid_of;
    std::vector<BamRead> &reads = D.reads; std::vector<int32_t> &rlen = D.rlen, &first_rec = D.first_rec;
    int64_t n_mapped = 0, n_nocig = 0;
    auto name_of = [&](int64_t k) { return std::string(names.data() + noff[(size_t)k], (size_t)(noff[(size_t)k + 1] - noff[(size_t)k])); };
    auto mapped_of = [](const BamRec &r) { return !(r.flag & 4) && r.refid >= 0; };
    for (int64_t k = 0; k < nrec; ++k) {
        const BamRec &r = recs[(size_t)k];
        const bool mapped = mapped_of(r);
        if (mapped) { ++n_mapped; if (r.n_norm == 0) ++n_nocig; }
        const int64_t qlen = (int64_t)r.clip5 + r.sm + r.si + r.clip3;
        if ((r.flag & 0x900) || r.lseq <= 0 || (mapped && r.lseq != qlen)) continue;
        if (r.qual0 == 0xff) D.any_ff = true;
        auto ins = qid_of.emplace(name_of(k), (int32_t)reads.size());
        if (!ins.second) continue;
        if (reads.size() >= 0x7ffffff0u) { ctx->err = "telr_bam_load: too many reads"; return TELR_E_RANGE; }
        BamRead R; R.seq_off = r.seq_off; R.qual_off = r.seq_off + ((int64_t)r.lseq + 1) / 2; R.len = r.lseq; R.rev = (r.flag & 0x10) ? 1 : 0;
        reads.push_back(R); rlen.push_back(r.lseq); first_rec.push_back((int32_t)k);
        B->qnames.push_back(ins.first->first);
    }
    const int32_t nq = (int32_t)reads.size();
    struct Kept { int32_t qid, cls, rec; };
    std::vector<Kept> kept;
    int64_t n_orphan = 0, n_lenmis = 0;
    for (int64_t k = 0; k < nrec; ++k) {
        const BamRec &r = recs[(size_t)k];
        if (!mapped_of(r) || r.n_norm == 0) continue;
        auto it = qid_of.find(name_of(k));
        if (it == qid_of.end()) { ++n_orphan; continue; }
        if ((int64_t)r.clip5 + r.sm + r.si + r.clip3 != rlen[(size_t)it->second]) { ++n_lenmis; continue; }
        Kept x; x.qid = it->second; x.cls = (r.flag & 0x100) ? 2 : (r.flag & 0x800) ? 1 : 0; x.rec = (int32_t)k;
        kept.push_back(x);
    }
    std::sort(kept.begin(), kept.end(), [](const Kept &a, const Kept &b) { return a.qid != b.qid ? a.qid < b.qid : a.cls != b.cls ? a.cls < b.cls : a.rec < b.rec; });
    const size_t nk = kept.size();
    D.R.reset(new telr_result());
    telr_result *R = D.R.get();
    R->ctx = ctx;
    R->alns.resize(nk);
    D.kept_rec.resize(nk); D.kept_off.resize(nk);
    int64_t ncig = 0; int32_t within = 0;
    for (size_t i = 0; i < nk; ++i) {
        const BamRec &r = recs[(size_t)kept[i].rec];
        within = (i > 0 && kept[i - 1].qid == kept[i].qid) ? within + 1 : 0;
        telr_aln &a = R->alns[i];
        const bool rev = (r.flag & 0x10) != 0;
        const int32_t qlen = r.clip5 + r.sm + r.si + r.clip3, blen = r.sm + r.si + r.sd;
        a.qid = kept[i].qid; a.tid = r.refid; a.qlen = qlen; a.tlen = B->tlens[(size_t)r.refid];
        a.qs = rev ? r.clip3 : r.clip5; a.qe = rev ? qlen - r.clip5 : qlen - r.clip3;
        a.ts = r.pos; a.te = r.pos + r.sm + r.sd;
        a.blen = blen;
        if (r.has_nm) { const int32_t m = (int32_t)((uint32_t)blen - (uint32_t)r.nm); a.mlen = m > 0 ? m : 0; } else a.mlen = r.sm;
        a.score = r.s1; a.subsc = r.s2; a.dp_score = r.as; a.cnt = r.cm; a.n_sub = 0; a.n_ambi = 0;
        a.parent = kept[i].cls == 2 ? 0 : within;
        a.n_cigar = r.n_norm; a.cigar_off = ncig;
        a.flags = (kept[i].cls == 2 ? TELR_F_SECONDARY : kept[i].cls == 1 ? TELR_F_SUPPL : TELR_F_PRIMARY) | (rev ? TELR_F_REV : 0);
        a.mapq = r.mapq;
        D.kept_rec[i] = kept[i].rec; D.kept_off[i] = ncig;
        ncig += r.n_norm;
    }
    D.ncig = ncig;
    B->counters[1] = nrec; B->counters[2] = n_mapped; B->counters[3] = (int64_t)nk; B->counters[4] = nq;
    B->counters[5] = n_orphan; B->counters[6] = n_lenmis; B->counters[7] = n_nocig;
    return TELR_OK;
}
// the result's CIGAR arrays for ncig words: the host mirror and the device array the emit pass writes
static int bam_in_result_arrays(telr_ctx *ctx, telr_result *R, int64_t ncig)
{
    R->cig = cig_alloc((size_t)ncig + 1);
    if (!R->cig) { ctx->err = "telr_bam_load: host CIGAR array"; return TELR_E_NOMEM; }
    R->cap = (size_t)ncig + 1; R->ncig = (size_t)ncig;
    if (hipMalloc(&R->d_cig, ((size_t)ncig + 1) * 4) != hipSuccess) { (void)hipGetLastError(); R->d_cig = nullptr; ctx->err = "telr_bam_load: device CIGAR array"; return TELR_E_NOMEM; }
    R->d_cap = (size_t)ncig + 1;
    return TELR_OK;
}

// a finished load: the handle takes the set and the result, and its name tables are made
static void bam_in_finish(telr_bam_in *B, telr_seqset *S, telr_result *R)
{
    for (auto &s : B->tnames) B->tname_ptr.push_back(s.c_str());
    for (auto &s : B->qnames) B->qname_ptr.push_back(s.c_str());
    B->tname_ptr.push_back(nullptr); B->qname_ptr.push_back(nullptr);
    B->set = S; B->res = R;
}

extern "C" int32_t telr_bam_in_target_count(const telr_bam_in *in) { return in ? (int32_t)in->tnames.size() : 0; }
extern "C" const char *const *telr_bam_in_target_names(const telr_bam_in *in) { return in ? in->tname_ptr.data() : nullptr; }
extern "C" const int32_t *telr_bam_in_target_lens(const telr_bam_in *in) { return in ? in->tlens.data() : nullptr; }
extern "C" int32_t telr_bam_in_read_count(const telr_bam_in *in) { return in ? (int32_t)in->qnames.size() : 0; }
extern "C" const char *const *telr_bam_in_read_names(const telr_bam_in *in) { return in ? in->qname_ptr.data() : nullptr; }
extern "C" const int32_t *telr_bam_in_read_lens(const telr_bam_in *in) { return in && in->set ? in->set->len.data() : nullptr; }
extern "C" telr_seqset *telr_bam_in_seqset(const telr_bam_in *in) { return in ? in->set : nullptr; }
extern "C" telr_result *telr_bam_in_result(const telr_bam_in *in) { return in ? in->res : nullptr; }
extern "C" telr_seqset *telr_bam_in_detach_seqset(telr_bam_in *in) { if (!in || !in->set_owned) return nullptr; in->set_owned = false; return in->set; }
extern "C" telr_result *telr_bam_in_detach_result(telr_bam_in *in) { if (!in || !in->res_owned) return nullptr; in->res_owned = false; return in->res; }
extern "C" int telr_bam_in_counters(const telr_bam_in *in, int64_t *out) { if (!in || !out) return TELR_E_ARG; memcpy(out, in->counters, sizeof(in->counters)); return TELR_OK; }
extern "C" int telr_bam_in_chunk_info(const telr_bam_in *in, int64_t *out) { if (!in || !out) return TELR_E_ARG; memcpy(out, in->chunk_info, sizeof(in->chunk_info)); return TELR_OK; }
extern "C" int telr_bam_in_phase_ms(const telr_bam_in *in, float *out) { if (!in || !out) return TELR_E_ARG; memcpy(out, in->phase_ms, sizeof(in->phase_ms)); return TELR_OK; }
// the reads as text: buf[off[q] .. off[q] + len[q]) = read q (A C G T N), off[q] = the bases before it; decoded on the device from the set
extern "C" int telr_bam_in_ascii(const telr_bam_in *in, char *buf, int64_t *off)
{
    (void)hipGetLastError();
    if (!in || !in->set || !in->ctx) return TELR_E_ARG;
    telr_ctx *ctx = in->ctx; const telr_seqset *S = in->set;
    if (!off || (S->total_bases > 0 && !buf)) { ctx->err = "telr_bam_in_ascii: null buffer"; return TELR_E_ARG; }
    std::vector<int64_t> coff((size_t)S->n + 1, 0);
    for (int32_t q = 0; q < S->n; ++q) { off[q] = coff[(size_t)q]; coff[(size_t)q + 1] = coff[(size_t)q] + S->len[(size_t)q]; }
    if (S->total_bases == 0) return TELR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint8_t *d_text; int64_t *d_coff;
    TRY(ctx_buf_t(ctx, "bamin_text", (size_t)S->total_bases, &d_text));
    TRY(ctx_buf_t(ctx, "bamin_coff", (size_t)S->n + 1, &d_coff));
    HIPCHK(hipMemcpyAsync(d_coff, coff.data(), ((size_t)S->n + 1) * 8, hipMemcpyHostToDevice, st));
    const int64_t nq4 = S->padded_bases / 4;
    hipLaunchKernelGGL(k_bam_ascii, grid256(nq4), dim3(256), 0, st, S->d_seq2, S->d_nmask, S->d_boff, S->d_len, d_coff, S->n, nq4, d_text);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(buf, d_text, (size_t)S->total_bases, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return TELR_OK;
}
