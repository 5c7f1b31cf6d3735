/*
 * telr_hip.h — C ABI of libtelrhip.so, the MI355X (gfx950) alignment engine that
 * replaces the seven aligner subprocess call sites of bergmanlab/TELR.
 *
 * The reference has no FFI: its boundary is `subprocess` argv + a SAM/PAF text
 * file.  Each entry point below cites the reference call site(s) it stands in
 * for (paths relative to the reference checkout):
 *
 *   S1  ngmlr -r R -q Q -x {ont,pacbio} ...            src/telr/TELR_alignment.py:31-51
 *   S2  minimap2 --cs --MD -Y -L -ax P R Q             src/telr/TELR_alignment.py:69-82
 *   S3  minimap2 -t N -ax P -r2k CNS READS             src/telr/TELR_assembly.py:199-212
 *   S4  minimap2 -cx P --secondary=no -v 0 SUBJ QRY    src/telr/TELR_te.py:68-78
 *   S5  minimap2 -cx P CONTIG LIB -v 0 -t T            src/telr/TELR_te.py:119-132
 *   S6  minimap2 -a -x P -v 0 SUBJ QRY                 src/telr/TELR_te.py:504-506
 *   S7  minimap2 -cx asm10 -v 0 -N 10 REF FLANK        src/telr/TELR_liftover.py:253-266
 *   D   samtools depth -aa -r chr:S-E  -> median       src/telr/TELR_te.py:870-884
 *
 * Conventions: every function returns 0 on success and a negative TELR_E_* code
 * on failure (telr_strerror() gives the text).  An empty result is NOT an
 * error (the reference treats an empty PAF as "locus not passed",
 * TELR_te.py:79-81).  The caller owns every input buffer (host pointers, may be
 * freed after the call returns); the library owns outputs until the matching
 * telr_*_free().  Device buffers never escape.  No torch types, no C++ types.
 */
#ifndef TELR_HIP_H
#define TELR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TELR_OK            0
#define TELR_E_NODEVICE   -1   /* no HIP device / HIP runtime error at init  */
#define TELR_E_HIP        -2   /* HIP runtime error (see telr_last_error)    */
#define TELR_E_ARG        -3   /* invalid argument                           */
#define TELR_E_RANGE      -4   /* input exceeds the engine's coordinate bits */
#define TELR_E_NOMEM      -5
#define TELR_E_IO         -6   /* a file could not be opened / mapped / written (telr_fasta_load: errno is the caller's to read) */

/* ---- alignment record flags -------------------------------------------- */
#define TELR_F_PRIMARY     0x1   /* parent == self                                  */
#define TELR_F_SECONDARY   0x2   /* overlaps a better chain on the query (SAM 0x100) */
#define TELR_F_SUPPL       0x4   /* primary chain that is not the best (SAM 0x800)   */
#define TELR_F_REV         0x8   /* query aligned on the reverse strand              */

/* ---- index options (minimap2 -k/-w/-H) ---------------------------------- */
typedef struct telr_idx_opt {
    int32_t k;            /* k-mer length, 4..28                                  */
    int32_t w;            /* minimizer window, 1..255                             */
    int32_t is_hpc;       /* homopolymer-compressed k-mers (map-pb)               */
    int32_t bucket_bits;  /* reserved (ignored): seeding probes an open-addressing table */
} telr_idx_opt;

/* ---- mapping options (one struct for all seven call sites) --------------- */
typedef struct telr_map_opt {
    /* seeding */
    float   mid_occ_frac;     /* -f   : fraction of most frequent minimizers ignored  */
    int32_t min_mid_occ;      /* -U lo                                                 */
    int32_t max_mid_occ;      /* -U hi                                                 */
    /* chaining */
    int32_t max_gap;          /* -g   : max reference/query distance between anchors   */
    int32_t bw;               /* -r   : max diagonal difference between anchors        */
    int32_t chain_lookback;   /* predecessors examined per anchor (multiple of 64)     */
    int32_t min_cnt;          /* -n   : min anchors per chain                          */
    int32_t min_chain_score;  /* -m                                                    */
    int32_t chain_gap_q8;     /* gap penalty per diagonal-difference base, Q8 fixed    */
    int32_t chain_skip_q8;    /* penalty per skipped base, Q8 fixed                    */
    /* chain selection */
    float   mask_level;       /* -M                                                    */
    float   pri_ratio;        /* -p                                                    */
    int32_t best_n;           /* -N                                                    */
    int32_t secondary;        /* --secondary=yes|no                                    */
    /* base-level alignment */
    int32_t a, b;             /* -A -B                                                 */
    int32_t q, e, q2, e2;     /* -O q,q2  -E e,e2                                      */
    int32_t sc_ambi;          /* penalty against an ambiguous base                     */
    int32_t zdrop;            /* -z                                                    */
    int32_t min_dp_max;       /* -s                                                    */
    int32_t min_ksw_len;      /* min gap-fill segment length                           */
    int32_t ext_max;          /* max bases an end extension may consume on the query   */
    int32_t ext_band;         /* half band width of end extensions (<= 31 with bw_long; presets: 31, ngmlr-ont 63) */
    int32_t flags;            /* TELR_MF_*                                             */
    int32_t fill_band_q4;     /* first-pass half band of a gap fill: 2 + q4*floor(sqrt(min(m,n)))/16;
                                 0 = 8.  Paths that come close to a band edge are re-aligned with the wide band. */
    int32_t fill_margin;      /* "close" = within this many diagonals of a band edge (0 = touching it)        */
    /* sub-read voting (NGMLR's candidate search, Sedlazeck 2018: the read is cut into sub-reads, the k-mer hits of a sub-read
     * vote for reference regions, only the best-voted regions are kept).  Applies to all-vs-all calls (qtarget == NULL, no
     * TELR_MF_PER_TARGET); 0 = off.  The hits of the minimizers whose last base lies in query bases [s*vote_len, (s+1)*vote_len)
     * vote into diagonal bins of 2^vote_bin_shift bases (per strand; 1024 bins, folded); a hit stays an anchor iff its bin and
     * the two next to it hold >= max(vote_min, ceil(vote_frac_q8 / 256 * votes of the sub-read's fullest bin)) hits. */
    int32_t vote_len;
    int32_t vote_bin_shift;
    int32_t vote_min;
    int32_t vote_frac_q8;
    /* long join (minimap2 -r500,20000: the second number): anchors are chained within max(bw, bw_long) diagonals, so that a
     * read across a multi-kb insertion or deletion is ONE chain; `bw` still bounds the gap fills.  A fill whose two lengths
     * differ by more than `bw` is aligned as two banded halves joined by one long gap at its best position.
     * 0 = off (asm10, ngmlr-*: NGMLR splits reads at SV breakpoints). */
    int32_t bw_long;
    /* convex gap cost (NGMLR, Sedlazeck 2018 Methods; `ngmlr -x ont`, TELR_alignment.py:28-51): cx_scale > 0 replaces the
     * two-piece affine cost (q, e, q2, e2 are then unused by the base-level DP) by: a gap pays cx_open once, and the gap base that
     * makes a gap of length i one longer pays ext(i) = max(cx_ext_min, cx_ext_max - cx_decay * i) -- NGMLR keeps the current
     * length with every gap cell, so this is the affine recurrence with a length-dependent extension.  All four numbers, and
     * every score inside the DP (a, b, sc_ambi, zdrop times cx_scale), are in 1/cx_scale of the unit of a / b / dp_score; a
     * record's dp_score is the sum of its segments' scores divided by cx_scale, rounded half up.  ngmlr-ont (NGMLR: match 1,
     * mismatch 1, open 1, extension 1 -> 0.5, decay 0.15; the preset's unit is half of NGMLR's): cx_scale 10, open 20,
     * ext 20 -> 10, decay 3.  ngmlr-pacbio (match 2, mismatch 5, open 5, extension 5 -> 1): cx_scale 20, open 100, ext 100 -> 20,
     * decay 3.  cx_scale = 0 over either preset gives the two-piece envelope q / e / q2 / e2 of round 3. */
    int32_t cx_scale, cx_open, cx_ext_max, cx_ext_min, cx_decay;
} telr_map_opt;

#define TELR_MF_CIGAR      0x1   /* -c / -a : run base-level alignment               */
#define TELR_MF_PER_TARGET 0x2   /* select/rank chains separately for every target:
                                    one call answers "QRY vs each of N subjects"
                                    (S5: the TE library against every contig)        */
#define TELR_MF_FAITHFUL   0x4   /* CPU oracle only (telr_map rejects it): drop the speed-motivated bounds of the spec --
                                    gap fills over the whole -r band, end extensions over the whole remaining read in a
                                    band of -r diagonals, chaining look-back 5000.  The reference point against which
                                    the tuned presets are gated (tests/test_faithful_gate.py).                          */

#define TELR_MF_KEEP_CIGARS 0x8  /* engine only (the oracle ignores it): the result keeps its CIGAR array on the device as well
                                    (same offsets; ~1.2 bytes per query base reserved), so that telr_write_bam_dev on the same
                                    context need not upload it again.  Records and CIGARs on the host are what they are without it. */
#define TELR_MF_CHAIN_SKIP 0x1000 /* minimap2's chaining scan (lchain.c: mg_lchain_dp, max_chain_iter 5000 / max_chain_skip 25):
                                    the predecessors of an anchor are scanned from the nearest down to the first one on its strand
                                    within max_gap reference bases, at most 5,000 back; a predecessor is taken only on a strictly
                                    larger score, and the scan stops once more than 25 predecessors that already lie on a chain
                                    through the anchor failed to improve it (the oracle's 0x1000: same f, p, chains and records).
                                    Overrides chain_lookback (which must still be valid).  Applies to every preset and to the
                                    per-target and per-query-target calls alike.  Off: the fixed look-back of the spec. */
#define TELR_MF_SEED_RESCUE 0x2000 /* minimap2's high-occurrence seed rescue (seed.c: mm_seed_select, occ_dist 500, max_max_occ 4095): in a
                                    maximal run of query minimizers with more than mid_occ occurrences (an absent minimizer ends a run
                                    like a rare one), bounded by the query positions ps and pe of the minimizers around it (0 and the
                                    query length at the ends), the (int)((pe - ps) / 500.0 + .499) least frequent ones with fewer than
                                    4,095 occurrences are seeded after all, each with all its occurrences, the earlier one on a tie
                                    (the oracle's 0x2000: same anchors, chains and records).  In the voting presets their hits vote
                                    like any other.  Applies to queries mapped against the whole index with the pooled cut-off; on
                                    a TELR_MF_PER_TARGET call and for a query with a target of its own (qtarget[i] >= 0) it is
                                    accepted and changes nothing.  Record fields such as n_ambi and the counters' meaning are unaffected. */
#define TELR_MF_MM2_MAPQ   0x20000 /* minimap2's MAPQ (map.c: mm_set_mapq) WITHOUT the second-best DP score (dp_max2 is not computed):
                                    (int)(identity * min(pen_s1, pen_cm) * 40 * (1 - subsc / score) * ln(dp_score / a))
                                    - (int)(4.343 * ln(n_sub + 1) + .499), clamped to 0..60, with identity = mlen / blen,
                                    pen_s1 = min(1, score / 100), pen_cm = min(1, cnt / 10), subsc floored at min_chain_score
                                    (the oracle's 0x20000: same mapq).  Every other field is what it is without it.  Applies to
                                    every call.  Off: the formula of Li 2018. */

/* ---- one alignment (PAF line / SAM record worth of numbers), 88 bytes ---- */
typedef struct telr_aln {
    int32_t  qid;        /* query index in the query set                          */
    int32_t  tid;        /* target index in the index                             */
    int32_t  qlen;
    int32_t  qs, qe;     /* query interval on the FORWARD query strand, [qs,qe)   */
    int32_t  tlen;
    int32_t  ts, te;     /* target interval, [ts,te)                              */
    int32_t  mlen;       /* matching bases (PAF col 10)                           */
    int32_t  blen;       /* alignment block length (PAF col 11)                   */
    int32_t  score;      /* chaining score   (s1)                                 */
    int32_t  subsc;      /* best secondary chaining score (s2)                    */
    int32_t  dp_score;   /* DP alignment score (AS)                               */
    int32_t  cnt;        /* anchors on the chain (cm)                             */
    int32_t  n_sub;      /* number of suboptimal chains                           */
    int32_t  parent;     /* index (within this query's records) of the parent     */
    int32_t  n_cigar;    /* number of CIGAR ops                                   */
    int32_t  flags;      /* TELR_F_*                                              */
    int64_t  cigar_off;  /* offset of the first op in the result's cigar array    */
    int32_t  mapq;
    int32_t  n_ambi;     /* reserved (0): ambiguous columns count as mismatches   */
} telr_aln;

/* CIGAR op encoding: len<<4 | op, op 0=M 1=I 2=D (BAM numbering) */

typedef struct telr_ctx    telr_ctx;     /* one per process per device            */
typedef struct telr_seqset telr_seqset;  /* 2-bit packed sequences resident in HBM */
typedef struct telr_index  telr_index;   /* minimizer index resident in HBM        */
typedef struct telr_result telr_result;  /* host-side alignment records + CIGARs   */

/* ---- context ------------------------------------------------------------- */
int  telr_init(int device, telr_ctx **out);
/* A second context for a host thread of its own: contexts are not re-entrant, different contexts are independent, sequence sets
 * and indexes may be used from either.  Its streams have the device's lowest priority: the kernels of the process' other
 * context are dispatched first (the loci leg runs its one large realignment, S6, behind the small S4 / S5 / S7 calls). */
int  telr_init_background(int device, telr_ctx **out);
/* Scratch is grow-only per context (a 30x read set leaves 150-250 GB behind): give all of it back -- the next call sizes it
 * again, ~2 ms per GB -- and the device's free / total memory, for a process whose contexts share one device. */
int  telr_release_scratch(telr_ctx *ctx);
int  telr_device_mem(telr_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
void telr_destroy(telr_ctx *ctx);
const char *telr_strerror(int code);
const char *telr_last_error(const telr_ctx *ctx);   /* text of the last HIP error   */
int  telr_device_name(const telr_ctx *ctx, char *buf, int buflen);

/* ---- presets: the -x values the reference passes -------------------------- */
/* name in {"map-ont","map-pb","asm10","ngmlr-ont","ngmlr-pacbio"}; returns TELR_E_ARG otherwise.
 * ngmlr-*: the stage-1 default of the reference (`ngmlr -x ont|pacbio`, TELR_alignment.py:28-51): (w,k) = (5,13)
 * minimizers (NGMLR's 13-mers at every third position), sub-read voting, NGMLR's convex gap cost in exact form (cx_*). */
int  telr_preset(const char *name, telr_idx_opt *io, telr_map_opt *mo);

/* ---- sequence sets --------------------------------------------------------- */
/* n sequences given as one concatenated ASCII buffer; seq i = ascii[off[i] .. off[i]+len[i]).
 * Packs to 2 bits/base + an ambiguity bitmask (host threads, 32 bases per AVX2 step where available; pinned grow-only
 * staging in the context) and uploads to HBM, chunk by chunk while the next chunks are packed. */
int  telr_seqset_create(telr_ctx *ctx, int32_t n, const char *ascii,
                        const int64_t *off, const int32_t *len, telr_seqset **out);
void telr_seqset_free(telr_seqset *s);
/* a new set holding copies of sequences idx[0..n) of `parent` (repeats allowed), made on the device from the packed
 * form: no host packing, no upload.  Replaces `seqtk subseq` of window reads out of the read file
 * (TELR_assembly.py:419-456) when the reads are already resident for stage 1. */
int  telr_seqset_subset(telr_ctx *ctx, const telr_seqset *parent, int32_t n, const int32_t *idx, telr_seqset **out);
/* the same with an orientation per copy: sequence i of the new set is the REVERSE COMPLEMENT of parent[idx[i]] when rc[i] != 0
 * (rc NULL = telr_seqset_subset).  Replaces the reverse-complemented contig FASTA of the per-locus realignment
 * (`realignment()` maps the window reads to the contig and to its reverse complement, TELR_te.py:495-515, 644-646): the
 * contigs are turned on the device, from the packed form they already have there. */
int  telr_seqset_subset_rc(telr_ctx *ctx, const telr_seqset *parent, int32_t n, const int32_t *idx, const uint8_t *rc, telr_seqset **out);
int64_t telr_seqset_bases(const telr_seqset *s);
int32_t telr_seqset_count(const telr_seqset *s);
/* The packed form itself, for moving sequences between the GPUs of a node without ever unpacking them (the N > 1 hand-offs of
 * window reads to the owner of their locus -- TELR_assembly.py:384-462 does this through the shared file system --
 * and the reads of a coordinate slice to the rank that writes that slice of the BAM, TELR_alignment.py:103-114).  The layout is
 * a pure function of the lengths: sequence i starts at base offset B(i) = sum over j < i of ceil(len[j] / 64) * 64; 2-bit
 * codes, 16 bases per 32-bit word (base b of the set in bits 2(b % 16).. of word b / 16), ambiguity mask 32 bases per word.
 * Two sets placed end to end are therefore the set of the concatenated lengths.
 * telr_seqset_packed: DEVICE pointers to the two word arrays of `s` (valid until it is freed) and their lengths in words
 * (padded_bases / 16 and padded_bases / 32).  telr_seqset_from_packed: a new set of n sequences with the given lengths (host
 * array) whose word arrays are copied device-to-device from d_seq2 / d_nmask (device pointers, e.g. the receive buffer of an
 * all-to-all; nwords2 / nwordsn must equal the layout's sizes). */
int  telr_seqset_packed(const telr_seqset *s, const void **d_seq2, const void **d_nmask, int64_t *nwords2, int64_t *nwordsn);
int  telr_seqset_from_packed(telr_ctx *ctx, int32_t n, const int32_t *len, const void *d_seq2, int64_t nwords2,
                             const void *d_nmask, int64_t nwordsn, telr_seqset **out);
/* Base qualities (FASTQ) for the QUAL field of the device BAM writer; optional.  qual_ascii[qual_off[i] .. qual_off[i] + len[i])
 * are the quality characters of sequence i of `s`; what is kept on the device is one byte per base, the Phred value (character
 * minus phred_offset; callers pass 33), in the set's own base layout: sequence i at byte B(i) of the array (see above).  Costs
 * 1 byte of HBM per (padded) base -- about 4 GB for a 30x read set -- and the upload (32-MB chunks through pinned staging),
 * taken only when called.  A character outside phred_offset .. phred_offset + 93 is TELR_E_ARG and leaves the set without
 * qualities; attaching again replaces the values.  telr_seqset_free frees the array.  Sets made by telr_seqset_subset,
 * telr_seqset_subset_rc and telr_seqset_from_packed carry NO qualities, whatever their source held (so the N-rank writer of
 * telr_amd/shard.py, which moves packed reads between ranks, writes 0xff). */
int  telr_seqset_attach_qual(telr_ctx *ctx, telr_seqset *s, const char *qual_ascii, const int64_t *qual_off, int32_t phred_offset);
int  telr_seqset_has_qual(const telr_seqset *s);
/* Pieces of a resident set as text (tests/seq_extract_ref.py states the definition in plain Python).  Piece k is
 * bases [start[k], start[k] + len[k]) of sequence idx[k]: the letters A C G T, N for a base whose mask bit is set; with rc[k] != 0
 * (rc NULL = all forward) the piece is reverse-complemented, the complement of N being N.  Pieces may repeat, overlap and come in
 * any order; len[k] == 0 writes nothing; no terminator is written.  The caller's `out` is dense: piece k at out[out_off[k] ..
 * out_off[k + 1]), out_off[n + 1] with out_off[0] >= 0 and out_off[k + 1] - out_off[k] == len[k].  n == 0 returns TELR_OK and
 * touches nothing.  The letters are made on the device from the packed words (one lane per 16 letters, each piece in a 16-byte
 * aligned slot of the device text); only the pieces travel to the host, the set is not copied; the bytes are the same on every run.
 * Everything is checked on the host before a kernel is launched, and a refused call leaves `out` untouched.  TELR_E_ARG (text in
 * telr_last_error): a negative n, an idx outside the set, a negative start or len, start + len beyond the sequence, out_off not
 * matching len, a null pointer where n > 0.  TELR_E_RANGE: 2^31 - 16 pieces or more, or slots (len rounded up to 16 bytes,
 * summed) of 2^35 bytes or more in one call. */
int  telr_seqset_extract(telr_ctx *ctx, const telr_seqset *s, int64_t n, const int32_t *idx, const int32_t *start, const int32_t *len,
                         const uint8_t *rc /* NULL = all forward */, char *out, const int64_t *out_off /* [n + 1] */);
/* The same pieces as a NEW SET: sequence k of *out is bases [start[k], start[k] + len[k]) of parent[idx[k]],
 * reverse-complemented when rc[k] != 0 (rc NULL = all forward); the mask bits are carried (an N stays an N), len[k] == 0 gives an empty
 * sequence.  The set has the layout of any other set (64-base-aligned offsets) and is made on the device from the packed words of
 * `parent` (the kernel telr_draft_contigs cuts its drafts with); no qualities are carried (as telr_seqset_subset).  n == 0 gives an
 * empty set.  The set is the caller's (telr_seqset_free).  Checked on the host before any launch, with the codes of
 * telr_seqset_extract: TELR_E_ARG for a negative n, an idx outside the set, a negative start or len, start + len beyond the sequence, a
 * null pointer where n > 0; TELR_E_RANGE from 2^31 - 16 pieces on. */
int  telr_seqset_pieces(telr_ctx *ctx, const telr_seqset *parent, int32_t n, const int32_t *idx, const int32_t *start, const int32_t *len,
                        const uint8_t *rc /* NULL = all forward */, telr_seqset **out);
/* Pieces CONCATENATED into a new set (tests/bridge_ref.py: join states the definition in plain Python): sequence o of
 * *out is pieces piece_off[o] .. piece_off[o + 1] one after the other, in order; a piece is what telr_seqset_pieces defines (bases
 * [start, start + len) of parent[idx], reverse-complemented when rc != 0, mask bits carried).  A sequence may have no pieces or pieces
 * of length 0 (both give what they hold: nothing); pieces may repeat and overlap.  The set has the normal layout (64-base-aligned
 * offsets, zero padding in both word arrays, an N has code 0) and carries no qualities.  n_out == 0 gives an empty set.  Made on the
 * device from the packed words of `parent`, one lane per 2-bit output word; the bytes are the same on every run.  The set is the
 * caller's (telr_seqset_free).  Checked on the host before any launch with the codes of telr_seqset_pieces (TELR_E_ARG: a negative
 * n_out, an idx outside the set, a negative start or len, start + len beyond the sequence, a null pointer where one is read), and
 * TELR_E_ARG for a piece_off that does not start at 0 or decreases; TELR_E_RANGE from 2^31 - 16 sequences or pieces on and for a
 * joined length above INT32_MAX.  A refused call leaves no set behind. */
int  telr_seqset_join(telr_ctx *ctx, const telr_seqset *parent, int32_t n_out, const int64_t *piece_off /* [n_out + 1] */,
                      const int32_t *idx, const int32_t *start, const int32_t *len, const uint8_t *rc /* NULL = all forward */,
                      telr_seqset **out);

/* ---- FASTA / FASTQ text -> the arrays above (host code; plain files, not gzip).  Replaces handing the file names to
 *      ngmlr / minimap2 (src/telr/TELR_alignment.py:31-51, 69-82).  Names end at the first white space. */
typedef struct telr_fasta telr_fasta;
int  telr_fasta_load(const char *path, telr_fasta **out);
int32_t telr_fasta_count(const telr_fasta *f);
int64_t telr_fasta_bases(const telr_fasta *f);                  /* sum of the lengths */
int64_t telr_fasta_extent(const telr_fasta *f);                 /* bytes behind telr_fasta_seq that the offsets may point into */
const char *telr_fasta_seq(const telr_fasta *f);                 /* base buffer: sequence i = [off[i], off[i] + len[i]); the sequences are
                                                                    packed end to end, or -- when every sequence of the file sits on one line --
                                                                    the buffer is the mapped file itself and nothing was copied */
const int64_t *telr_fasta_off(const telr_fasta *f);
const int32_t *telr_fasta_len(const telr_fasta *f);
const char *const *telr_fasta_names(const telr_fasta *f);
/* FASTQ: the quality characters of record i are qual[qual_off[i] .. qual_off[i] + len[i]) -- in the mapped file itself when
 * the bases are used in place, else copied next to the bases (CR dropped).  Both NULL for a FASTA file and for an empty file.
 * A record whose quality line is not as long as its sequence line makes telr_fasta_load return TELR_E_ARG. */
const char *telr_fasta_qual(const telr_fasta *f);
const int64_t *telr_fasta_qual_off(const telr_fasta *f);
void telr_fasta_free(telr_fasta *f);

/* ---- index (replaces "minimap2 ... REF" re-indexing REF on every call) ----- */
int  telr_index_build(telr_ctx *ctx, const telr_seqset *targets, const telr_idx_opt *io,
                      telr_index **out);
void telr_index_free(telr_index *idx);
/* number of minimizers / distinct minimizers, for reports */
int  telr_index_stats(const telr_index *idx, int64_t *n_minimizers, int64_t *n_distinct);

/* ---- references of any size: a multi-part index, merged on the device (opt-in).  An index holds its targets in one
 *      31-bit coordinate space, so telr_index_build refuses a target set whose padded extent reaches 2^31 bases.  The way round it is
 *      minimap2's own (`-I` / `--split-prefix`): cut the targets into parts that each fit, map the reads against every part, and run the
 *      final selection again over each read's pooled records.  tests/part_merge_ref.py states the merge in plain Python integers.
 * Parts (telr_part_plan; host only, no device needed).  Contiguous runs of targets in target order, chosen greedily: a part's extent
 *      starts at 0 and advances target by target as telr_index_build lays targets out, g -> (g + len + 16384 + 63) & ~63; a target with
 *      which the extent would REACH max_bases starts the next part.  max_bases 0 = the engine's own limit, 2^31 (a larger value is that
 *      limit too).  part_of[t] = the part of target t, *n_parts their number; n_targets == 0 gives 0 parts.  Every part is accepted by
 *      telr_index_build; no part would be with its successor's first target added.  TELR_E_RANGE: a target that alone reaches the limit
 *      (telr_part_plan_error names it; the text of the calling thread's last telr_part_plan).  TELR_E_ARG: a negative length or
 *      max_bases, a null pointer where it is needed.
 * Merge (telr_merge_parts).  parts[p] = the result of mapping the SAME n_queries queries against the index of part p, with the same
 *      options `mo`; tid_map[p][0 .. n_part_targets[p]) = the global id of every target of part p.
 *   1. Pool.   For each query, its records from all parts; a record is (part, rank), rank = its index within that part's records
 *              of the query.
 *   2. Order.  The pool sorted by (dp_score descending, part ascending, rank ascending).
 *   3. State.  Every record starts as its own parent.  A record that was PRIMARY or SUPPL in its part keeps its subsc and n_sub, one
 *              that was SECONDARY starts with 0 for both.
 *   4. Mask.   For i in order: the first earlier j that is still its own parent and for which
 *              (float)overlap(qs, qe) > mask_level * (float)min(len_i, len_j) (float32, as the engine's selection) becomes i's parent;
 *              then subsc[j] = max(subsc[j], score_i) and n_sub[j] += 1 -- unless i was j's secondary in the same part already (same
 *              part, i was SECONDARY, i's part-level parent == j's rank): j counted it there.
 *   5. Keep.   Own parents always.  A secondary iff mo->secondary, (float)dp_i >= (float)dp_parent * pri_ratio, and fewer than
 *              best_n kept secondaries precede it.
 *   6. Fields of a kept record: parent = the parent's index among the query's kept records; the first kept own parent is PRIMARY,
 *              the others SUPPL, the rest SECONDARY, TELR_F_REV (and any other bit) carried; subsc = n_sub = 0 on secondaries; tid =
 *              the global id; mapq by the formula telr_map uses (TELR_MF_MM2_MAPQ or not), computed on the host; cigar_off dense in
 *              output order; every other field carried.
 *   7. Output. Ordered by (qid, kept order).  An ordinary result: records on the host, the CIGAR words gathered on the device from
 *              the parts' arrays (a part's resident copy, TELR_MF_KEEP_CIGARS, or one upload) into a resident array of its own --
 *              complete, as after TELR_MF_KEEP_CIGARS -- and mirrored to the host once.  The bytes are the same on every run.
 *      With one part the merge is the identity.  TELR_MF_PER_TARGET is TELR_E_ARG (per-target calls never compete across targets);
 *      every other flag passes through.  Checked on the host before any launch, TELR_E_ARG with a text in telr_last_error and `out`
 *      untouched: a part not ordered by qid, a qid outside [0, n_queries), a tid outside its map, cigar_off + n_cigar outside the
 *      part's words, a parent outside the query's records in the part, flags without exactly one class bit, a null pointer where
 *      it is needed.  TELR_E_RANGE from 2^31 - 16 pooled records on.  An empty part, zero parts, zero queries, zero records: valid.
 * Caveats. The occurrence cut-off (mid_occ) is per part, as in minimap2: a repeat below it in a part but above it in the whole set is
 *      seeded in the parts, so the merged result can hold secondaries the unsplit index would not.  All part indexes, the P part
 *      results and the merged one live side by side: a read set for which that does not fit gets TELR_E_NOMEM. */
int  telr_part_plan(int32_t n_targets, const int32_t *target_len, int64_t max_bases, int32_t *part_of /* [n_targets] */, int32_t *n_parts);
const char *telr_part_plan_error(void);
int  telr_merge_parts(telr_ctx *ctx, int32_t n_parts, const telr_result *const *parts,
                      const int32_t *const *tid_map /* part-local tid -> global tid */, const int32_t *n_part_targets,
                      int32_t n_queries, const telr_map_opt *mo, telr_result **out);

/* ---- mapping (S1,S2,S7: all queries vs all targets; S3,S4,S6: query i vs the
 *      single target qtarget[i]; S5: TELR_MF_PER_TARGET) ------------------------
 * qtarget may be NULL (every query sees every target) or hold one target id
 * per query (-1 = all).  Blocking; internally stream-asynchronous.
 * A query set of any size is accepted: up to 1.6 Gbp is one range; a larger one streams through in an even number of equal
 * ranges of at most 1.4 Gbp, two of them in flight (each bounded by an anchor budget at the density the index has shown), and the records
 * come back in query order whatever the cut.  The scratch is grow-only per context (about 75 B per query base of the
 * largest range at 0.25 anchors per base); TELR_E_NOMEM with two ranges in flight makes the call run again one range at a
 * time before it is reported. */
int  telr_map(telr_ctx *ctx, const telr_index *idx, const telr_seqset *queries,
              const int32_t *qtarget, const telr_map_opt *mo, telr_result **out);

int64_t         telr_result_count(const telr_result *r);
const telr_aln *telr_result_alns(const telr_result *r);     /* sorted by (qid, rank) */
/* CIGAR ops (BAM encoding, len<<4|op) of all records in one array; a record owns ops
 * [cigar_off, cigar_off + n_cigar).  The array is filled by one DMA that starts before the final
 * chain selection, so it may also hold the ops of chains that selection dropped (unreferenced).
 * telr_map returns as soon as the RECORDS are complete; the DMA of the CIGAR array may still be in flight
 * (so that a caller streaming batches overlaps it with the next telr_map call).  telr_result_cigars,
 * the writers, telr_depth_medians and telr_result_free wait for it; telr_result_wait does so explicitly. */
/* A result made of records and CIGAR words the caller holds (copied; cigar_off must index `cigars`): for the writers and
 * telr_depth_medians on records that were mapped elsewhere -- at N > 1 ranks the stage-1 hand-off is ONE sorted BAM, written by
 * rank 0 from the records every rank mapped (telr_amd/shard.py: gather_stage1). */
int             telr_result_from_arrays(telr_ctx *ctx, const telr_aln *alns, int64_t n, const uint32_t *cigars, int64_t n_cigar,
                                        telr_result **out);
/* the same with the CIGAR words in DEVICE memory (e.g. the receive buffer of an all-to-all): copied device-to-device into the
 * result's device array -- which the device BAM writer reads in place -- and mirrored to the host array once */
int             telr_result_from_device_cigars(telr_ctx *ctx, const telr_aln *alns, int64_t n, const void *d_cigars, int64_t n_cigar,
                                               telr_result **out);
int             telr_result_wait(const telr_result *r);
int64_t         telr_result_cigar_count(const telr_result *r);
const uint32_t *telr_result_cigars(const telr_result *r);
void            telr_result_free(telr_result *r);

/* ---- text emitters at the reference's own boundary (PAF for S4,S5,S7; SAM for S1,S2,S3,S6) --------
 * qnames / tnames: arrays of C strings indexed by query / target id.  path NULL = stdout. */
int  telr_write_paf(const telr_result *r, const char *const *qnames, const char *const *tnames, int with_cigar,
                    const char *path, int append);
#define TELR_SAM_MD          0x1   /* --MD */
#define TELR_SAM_CS          0x2   /* --cs */
#define TELR_SAM_SOFTCLIP    0x4   /* -Y  */
#define TELR_SAM_NO_UNMAPPED 0x8
#define TELR_SAM_PRIMARY_ONLY 0x10 /* drop secondary and supplementary records: `samtools view -F0x900`          */
#define TELR_SAM_SORTED      0x20  /* coordinate order (target, position; unmapped last): `samtools sort`         */
#define TELR_SAM_NO_HEADER   0x40  /* records only, as `samtools view` without -h.  PRIMARY_ONLY|SORTED|NO_HEADER =
                                      the text `samtools view -F0x900 sorted.bam` pipes into wtpoa-cns at the
                                      polishing site (hand-off H3, src/telr/TELR_assembly.py:208,228)                */
/* sequences are needed for SEQ, NM, MD and cs: concatenated ASCII + offsets + lengths as in telr_seqset_create.
 * rg_id NULL = no @RG line / RG tag (minimap2 sites); NGMLR site passes --rg-id/--rg-sm/--rg-lb. */
int  telr_write_sam(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                    const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                    const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                    const char *pg_line, const char *path);
/* The same with the reads' base qualities in column 11: q_qual[q_qual_off[q] .. + q_len[q]) are read q's quality characters,
 * phred_offset what they are offset by (33 for FASTQ); printed as Phred + 33 for exactly the bases SEQ holds, in SEQ's
 * orientation (reversed on the reverse strand, cut like SEQ by hard clips), `*` where SEQ is `*` or empty.  q_qual NULL =
 * telr_write_sam.  A character outside phred_offset .. phred_offset + 93 is TELR_E_ARG (nothing is written). */
int  telr_write_sam_qual(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                         const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                         const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                         const char *pg_line, const char *path, const char *q_qual, const int64_t *q_qual_off, int32_t phred_offset);

/* Coordinate-sorted BAM (+ .bai when write_index != 0): replaces `samtools sort -o BAM SAM; samtools index BAM`
 * (src/telr/TELR_alignment.py:103-114).  Same arguments as telr_write_sam; level = zlib level (0 -> 1). */
int  telr_write_bam(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                    const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                    const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                    const char *pg_line, const char *bam_path, int32_t write_index, int32_t level);
/* The same with QUAL = the Phred values of SEQ's bases (arguments as telr_write_sam_qual; q_qual NULL = telr_write_bam: 0xff).
 * Its uncompressed stream equals the one telr_write_bam_dev writes for a read set with the same qualities attached. */
int  telr_write_bam_qual(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                         const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                         const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                         const char *pg_line, const char *bam_path, int32_t write_index, int32_t level,
                         const char *q_qual, const int64_t *q_qual_off, int32_t phred_offset);

/* The same file made on the DEVICE from what is already resident there (the reads, the reference, the CIGARs): NM / MD / cs /
 * SA, the 4-bit SEQ, the coordinate sort (refID, position, forward before reverse strand, then query order) and the BGZF
 * blocks (CRC-32 included) are computed by kernels, the host only moves the finished file image into `bam_path` and writes
 * the .bai.  `queries` = the set the result was mapped from, `idx` = the index it was mapped against (its targets supply the
 * reference bases).  No ASCII sequences are needed.  level 0 = stored BGZF blocks; level >= 1 = deflate blocks coded on
 * the device (Huffman tables per BAM field class, run-length matches).  Bases print as the engine sees them: A C G T, anything
 * else N (telr_write_bam / telr_write_sam print the same, so the uncompressed streams of the two writers are equal).
 * QUAL is 0xff (absent) unless `queries` has qualities attached (telr_seqset_attach_qual): then every record holds the Phred
 * values of the bases its SEQ holds, in SEQ's orientation -- reversed for a reverse-strand record, cut like SEQ on a
 * hard-clipped supplementary record, none for a secondary (l_seq 0), the whole read forward for an unmapped read -- and the
 * device deflate codes QUAL with a Huffman table of its own (a fourth field class).  telr_write_bam_slice honours attached
 * qualities the same way.  A file written without qualities is byte for byte what it was before the option existed. */
/* Optional, before telr_map: start creating `bam_path` in the background -- the file is created and mapped at once, then
 * est_bytes of it (a BAM with --cs --MD takes about 0.85 bytes per read base at level 1, 2.8 at level 0; attached qualities add
 * what their entropy asks for -- measured 0.81 -> 1.26 bytes per read base at level 1 with ONT-shaped qualities of 3.6 bits,
 * tools/bam_qual_ab.py; up to 0.82 more for qualities spread evenly over 0..93) are allocated and
 * pre-faulted into the mapping block by block, front to back -- so that telr_write_bam_dev(... the same path ...) copies the
 * finished file image into pages that exist and are mapped (80+ GB/s instead of the 6-15 GB/s of a fresh page-cache page),
 * and cuts the file to size.  Without it, or past the estimate, the writer streams through a pinned ring and one pwrite
 * thread.  The mapping is taken apart by a background thread after the file is complete; telr_bam_release_wait() waits for
 * that (only a process that prepares another file right away has a reason to).  A prepared file that is never written is
 * removed from the context by the next telr_bam_prepare / telr_destroy / telr_bam_discard (the file itself stays: a caller
 * whose mapping failed unlinks it -- the reference tests for the file's existence, TELR_alignment.py:110-114).  A writer call
 * that fails removes `bam_path` and its .bai itself.  One telr_write_bam_dev runs at a time per process. */
/* ---- ONE coordinate-sorted BAM written by N ranks (SURVEY 8e x TELR_alignment.py:103-114; TELR_sv.py:35-47 reads one file) ----
 * The records of the job are range-partitioned by (refID, position); rank k holds the reads that have a record in slice k with
 * ALL their records (`emit[i]` = record i of the result lies in this slice; the others are only there so that the SA tag of an
 * emitted record can name them) and makes the BGZF blocks of its slice on its device: telr_write_bam_slice (with_header: rank 0;
 * TELR_SAM_NO_UNMAPPED in flags on every rank but the last, which also holds the reads without a record).  The slice's size is
 * then known (telr_bam_segment_info: out[0] bytes in the file, [1] mapped records, [2] unmapped reads, [3] uncompressed
 * bytes); after an exclusive scan of the sizes over the ranks every rank puts its image at its place of the one file
 * (telr_bam_segment_write: `path` exists, is_last appends the BGZF EOF block) and hands what the index needs of its records
 * (telr_bam_segment_entries: arrays of [1] entries in file order, virtual offsets for the slice at file_off) to rank 0, which
 * writes the one .bai from the concatenated arrays (telr_bai_write).  The inflated stream of the N-rank file equals the
 * one-rank file's byte for byte (same records, same order -- ties by the job-level read number: the reads of a rank must be
 * in that order); the BGZF block boundaries differ.  The image lives in the context until its next writer call. */
typedef struct telr_bam_segment telr_bam_segment;
int  telr_write_bam_slice(telr_ctx *ctx, const telr_result *r, const telr_seqset *queries, const telr_index *idx,
                          const char *const *qnames, const char *const *tnames, int32_t flags,
                          const char *rg_id, const char *rg_sm, const char *rg_lb, const char *pg_line,
                          const uint8_t *emit, int32_t with_header, int32_t level, telr_bam_segment **out);
int  telr_bam_segment_info(const telr_bam_segment *s, int64_t *out);
int  telr_bam_segment_entries(const telr_bam_segment *s, int64_t file_off, int32_t *tid, int32_t *ts, int32_t *te, uint64_t *vb, uint64_t *v_end);
int  telr_bam_segment_write(telr_ctx *ctx, const telr_bam_segment *s, const char *path, int64_t file_off, int32_t is_last);
void telr_bam_segment_free(telr_bam_segment *s);
int  telr_bai_write(const char *bai_path, int64_t n, const int32_t *tid, const int32_t *ts, const int32_t *te, const uint64_t *vb, uint64_t v_end,
                    int64_t n_unmapped, int32_t n_targets, const int32_t *t_len);
int  telr_bam_prepare(telr_ctx *ctx, const char *bam_path, int64_t est_bytes);
int  telr_bam_release_wait(void);
int  telr_bam_discard(telr_ctx *ctx);
int  telr_write_bam_dev(telr_ctx *ctx, const telr_result *r, const telr_seqset *queries, const telr_index *idx,
                        const char *const *qnames, const char *const *tnames, int32_t flags, const char *rg_id, const char *rg_sm,
                        const char *rg_lb, const char *pg_line, const char *bam_path, int32_t write_index, int32_t level);
/* the same with the target set itself in the index's place (the writer reads nothing of an index but its targets): for a result
 * whose tids are those of a set no single index holds (telr_merge_parts).  telr_write_bam_dev is this call with the index's targets. */
int  telr_write_bam_dev_targets(telr_ctx *ctx, const telr_result *r, const telr_seqset *queries, const telr_seqset *targets,
                                const char *const *qnames, const char *const *tnames, int32_t flags, const char *rg_id, const char *rg_sm,
                                const char *rg_lb, const char *pg_line, const char *bam_path, int32_t write_index, int32_t level);

/* ---- pile-up consensus of the index's targets from the PRIMARY records of a result (neither secondary nor supplementary:
 *      `samtools view -F0x900`).  Stands where the reference pipes that view into `wtpoa-cns -d CNS -i -` to polish a locus'
 *      draft contig (src/telr/TELR_assembly.py:226-247) -- with a different algorithm: a majority vote per contig position
 *      (base / deletion / up to 8 inserted bases after it; D runs longer than 30 do not vote; positions covered by fewer than
 *      min_depth records keep the draft base), not wtpoa-cns's partial-order alignment.  Offered behind telr_assembly's polish="pileup".  DESIGN.md 3.12. */
typedef struct telr_consensus telr_consensus;
int  telr_consensus_build(telr_ctx *ctx, const telr_result *r, const telr_seqset *queries, const telr_index *idx, int32_t min_depth,
                          telr_consensus **out);
/* The same hand-off with a WINDOW PARTIAL-ORDER consensus (opt-in like the pile-up: wtpoa-cns's own source is
 * absent, this is the published scheme of window POA polishing): the draft is cut into 200-base windows, every primary record
 * that covers a window whole gives the piece of its read its CIGAR aligns there, the pieces are re-aligned one by one to a graph
 * that starts as the draft's window (sequence-to-graph DP, one wave per window) and merged into it, the window's consensus is
 * the heaviest-bundle path.  Unlike the pile-up vote it re-phases columns: it does not trust the pairwise CIGARs inside a window. */
int  telr_poa_build(telr_ctx *ctx, const telr_result *r, const telr_seqset *queries, const telr_index *idx, int32_t min_depth,
                    telr_consensus **out);
/* Both builds check every record of r before anything reaches the device and return TELR_E_ARG if one fails: 0 <= ts <= te <=
 * the target's length, 0 <= qs <= qe <= qlen == the query's length, CIGAR ops only M / I / D, M + D = te - ts, M + I = qe - qs
 * (a record without CIGAR ops votes nothing and passes).  Host-only debug entry of the same check on caller-held arrays:
 * TELR_OK, or TELR_E_ARG with *first_bad = the index of the first record that fails. */
int  telr_debug_check_records(const telr_aln *alns, int64_t n, const uint32_t *cigars, int64_t n_cigar, const int32_t *qlens, int32_t n_queries,
                              const int32_t *tlens, int32_t n_targets, int64_t *first_bad);
int32_t telr_consensus_count(const telr_consensus *c);              /* = number of targets */
const char *telr_consensus_seq(const telr_consensus *c);             /* concatenated consensus sequences (A C G T N) */
const int64_t *telr_consensus_off(const telr_consensus *c);
const int32_t *telr_consensus_len(const telr_consensus *c);
void telr_consensus_free(telr_consensus *c);

/* ---- fused "samtools depth -aa -r | median" (D) --------------------------------
 * For n_iv intervals (target id, 0-based start, 0-based INCLUSIVE end — the
 * reference feeds 0-based numbers into samtools' 1-based inclusive region
 * string, TELR_te.py:870-884, so E-S+1 positions are read starting one base
 * to the left; callers pass the positions they want counted) compute the
 * per-base depth of the result's primary+supplementary records (secondary
 * skipped, deletions not counted) and return the median as samtools+python
 * `statistics.median` would (mean of the two middle values for even counts).
 * A depth above 8,000 counts as 8,000; an interval is clamped to the target, an
 * empty one (start past the last base, end before the start) gives NaN.
 * Refused with TELR_E_ARG, before anything is launched, with the reason in
 * telr_last_error ("telr_depth_medians: ..."): a negative target_len; an interval
 * whose tid is no target; any record (secondary ones included) with a tid that is
 * no target, with qid / qlen / qs < 0, qe outside [qs, qlen], ts < 0 or te < ts, or
 * with a CIGAR range outside the result's array; a record that is not secondary
 * with te > target_len[tid].  A record whose te is inside its target but whose
 * CIGAR (M and D lengths from ts on) runs past the target's end is found on the
 * device: TELR_E_ARG, "record's CIGAR leaves its target".  median_out is written
 * only when the call returns TELR_OK. */
int  telr_depth_medians(telr_ctx *ctx, const telr_result *r, int32_t n_targets,
                        const int32_t *target_len, int32_t n_iv, const int32_t *iv_tid,
                        const int32_t *iv_start, const int32_t *iv_end, double *median_out);

/* ---- insertion candidates from a mapped read set (opt-in; stands where the reference shells out to Sniffles, `detect_sv`,
 *      src/telr/TELR_sv.py:49-51).  An OWN definition, not a restatement of Sniffles; parity with it is unpinned.
 * Eligible records: not TELR_F_SECONDARY, mapq >= min_mapq.  Strand coordinates of a record: qs' = qs, qe' = qe forward;
 * qs' = qlen - qe, qe' = qlen - qs on TELR_F_REV.
 * Signatures:  kind 0 (intra) every I op of >= min_len of an eligible record: pos = ts + the M and D lengths before it, len = its
 *              length (neighbouring I ops are not merged);
 *              kind 1 (split) every ordered pair (a, b) of distinct eligible records of one query with the same tid and strand,
 *              qgap = b.qs' - a.qe' >= 0, |tgap = b.ts - a.te| <= max_ref_gap, qgap - tgap >= min_len: pos = a.te,
 *              len = qgap - tgap, rec = a, mate = b (all pairs: adjacency is not tested);
 *              kind 2 (clip) qs' >= min_clip: pos = ts, len = qs'; qlen - qe' >= min_clip: pos = te, len = qlen - qe' (a lower bound).
 *              [seg_start, seg_start + seg_len) are the inserted / unaligned bases on the FORWARD read.  Sorted ascending by
 *              (tid, pos, rec, kind, len, mate).
 * Clusters:    single linkage over (tid, pos): a new one where tid changes or pos - previous pos > cluster_dist.  A cluster is a
 *              call when it has >= min_support distinct reads and >= min_sized distinct reads among its kind-0 / kind-1 signatures.
 * Call:        pos = lower median of its signatures' positions; len = lower median of the sized signatures' len; rep = index (in
 *              the signature array) of the sized signature holding it in the order (len, qid, rec, mate) (-1, len 0, without one);
 *              support / n_sized = distinct reads; its reads ascending at reads[read_off[i] .. read_off[i + 1]).
 * The CIGAR words are read on the device: the result's resident copy (TELR_MF_KEEP_CIGARS) or one upload.  The output is the
 * same on every run.  TELR_E_ARG (text in telr_last_error): a negative option, min_sized > min_support, a record's tid outside
 * [0, n_targets) or coordinates out of order.  No eligible record: zero calls, TELR_OK.  opt NULL = the defaults. */
typedef struct telr_ins_opt {
    int32_t min_len;       /* 50  */
    int32_t min_mapq;      /* 20  */
    int32_t min_clip;      /* 200 */
    int32_t max_ref_gap;   /* 200 */
    int32_t cluster_dist;  /* 50  */
    int32_t min_support;   /* 10  */
    int32_t min_sized;     /* 1   */
    int32_t reserved;      /* 0   */
} telr_ins_opt;
typedef struct telr_ins_sig  { int32_t tid, pos, len, qid, kind, rec, mate, seg_start, seg_len; } telr_ins_sig;
typedef struct telr_ins_call { int32_t tid, pos, len, support, n_sized, rep; } telr_ins_call;
typedef struct telr_ins_calls telr_ins_calls;
void telr_ins_opt_default(telr_ins_opt *o);
int  telr_call_insertions(telr_ctx *ctx, const telr_result *r, int32_t n_targets, const telr_ins_opt *opt, telr_ins_calls **out);
int64_t telr_ins_calls_count(const telr_ins_calls *c);
const telr_ins_call *telr_ins_calls_calls(const telr_ins_calls *c);
int64_t telr_ins_calls_sig_count(const telr_ins_calls *c);
const telr_ins_sig *telr_ins_calls_sigs(const telr_ins_calls *c);
const int64_t *telr_ins_calls_read_off(const telr_ins_calls *c);      /* count + 1 offsets into telr_ins_calls_reads */
const int32_t *telr_ins_calls_reads(const telr_ins_calls *c);
void telr_ins_calls_free(telr_ins_calls *c);

/* ---- the supporters of insertion sites the CALLER names (opt-in): another sample's calls, a cohort's merged list, a
 *      truth set.  telr_call_insertions can only discover clusters and threshold them; this entry assigns the same signatures to given
 *      positions and returns one call per site whatever its support, in the shape telr_genotype_insertions takes.  An OWN definition
 *      like 5.10 and 5.11: NOT Sniffles' --genotype-vcf, and its agreement with Sniffles is not pinned.
 * Signatures:  exactly those of telr_call_insertions under opt: same eligibility, same three kinds, and the same complete sort key
 *              (tid, pos, rec, kind, len, mate).  min_support, min_sized and cluster_dist of opt are not read.
 * Sites:       sites[n_sites], strictly ascending by (tid, pos); len = the expected insertion length, 0 = unknown.
 * Assignment:  a signature s is NEAR site c iff s.tid == c.tid and |s.pos - c.pos| <= reach.  A signature goes to the nearest site it
 *              is near; on equal distance to the site with the smaller index; a signature near no site is dropped.  (Because sites are
 *              strictly ascending, the nearest site is one of the two around the signature's key.)
 * Length test: only for sized signatures (kinds 0 and 1), and only when len_pct > 0 and the assigned site has len > 0: the signature
 *              is dropped iff 100 * |s.len - c.len| > len_pct * c.len, in 64-bit integer arithmetic.  A dropped signature is not offered
 *              to another site.  Clips are never length-tested.
 * Output:      a telr_ins_calls with ONE CALL PER SITE, IN SITE ORDER, whatever its support: tid and pos are the site's; support =
 *              the distinct qids of its kept signatures; n_sized = the distinct qids among the kept sized signatures; rep = the sized
 *              signature holding the lower median in the order (len, qid, rec, mate), len = that signature's len (without a sized
 *              signature rep = -1 and len = 0); the read list = the ascending distinct qids (a site with no kept signature has an
 *              empty list).  The signature array of the result holds ONLY THE KEPT signatures, in their sorted order; rep indexes it.
 *              Calls strictly ascending, each with a supporter list: what telr_genotype_insertions takes, unchanged.  (It returns
 *              gt = 2 for alt = ref = 0, since 0 >= 0; the layers above print such a site as ./. with AF nan.)
 * TELR_E_ARG (text in telr_last_error): everything telr_call_insertions refuses in a record or in the options this entry reads
 *              (a negative min_len, min_mapq, min_clip or max_ref_gap), sites not strictly ascending, a site's tid outside
 *              [0, n_targets), a negative pos or len, reach < 0, len_pct outside 0..100, a non-zero reserved field, n_sites < 0, a null
 *              sites with n_sites > 0.  TELR_E_RANGE: 2^31 - 16 sites or more.  n_sites == 0: an empty result, nothing is launched;
 *              no eligible record (or no signature): n_sites empty calls.  Everything is checked on the host before a kernel runs.
 *              The output is the same on every run.  opt / sopt NULL = the defaults. */
typedef struct telr_ins_site { int32_t tid, pos, len; } telr_ins_site;   /* len: expected insertion length, 0 = unknown */
typedef struct telr_site_opt { int32_t reach;    /* 50 */
                               int32_t len_pct;  /* 0: no length test */
                               int32_t reserved[2]; } telr_site_opt;
void telr_site_opt_default(telr_site_opt *o);
int  telr_call_at_sites(telr_ctx *ctx, const telr_result *r, int32_t n_targets, const telr_ins_opt *opt,
                        const telr_ins_site *sites, int64_t n_sites, const telr_site_opt *sopt, telr_ins_calls **out);

/* ---- several samples' insertion calls merged into ONE site list (opt-in): the step between the per-sample calls of a
 *      cohort and the list telr_call_at_sites takes.  An OWN definition like 5.10, 5.11 and 5.19: NOT bcftools merge, SURVIVOR or
 *      Jasmine, and its agreement with them is not pinned.  It reads no sequence and needs no index.
 * Input:       e[0 .. n) in any order: len = the insertion length, 0 = unknown; sample = the caller's sample number; group = a class
 *              the caller chooses (a TE family number, or 0 for all): entries of different groups never merge.
 * Order:       the complete key (tid, group, pos, sample, len, i) ascending, i = the input index: a total order.
 * Clusters:    single linkage in that order: a new one where tid changes, group changes, or pos - previous pos > dist (64-bit).
 * Site of a cluster of m members: tid, group = the cluster's; pos = the position of member (m - 1) / 2 in key order (the lower median);
 *              pos_min / pos_max = its first / last member's positions; n_members = m; n_samples = its distinct sample values;
 *              n_sized = the members with len > 0; len = the lower median of the sized members in the order (len, sample, i), 0 without
 *              one; len_min / len_max = the smallest / largest sized length (0, 0 without one); rep = the input index of the sized
 *              member holding that median, without a sized member the input index of member (m - 1) / 2.
 * Filter:      sites with n_samples < min_samples are dropped before anything below.
 * Final order: ascending by (tid, pos, n_samples descending, n_members descending, group).  A site is SHADOWED when the site before
 *              it in this order has the same (tid, pos) (only possible across groups); its winner = the output index of the first site
 *              of that (tid, pos) run, -1 for a site that is not shadowed.  The sites that are not shadowed are strictly ascending
 *              by (tid, pos): what telr_call_at_sites takes.  A site that is not shadowed is CROWDED when the previous or the next
 *              not-shadowed site is on its tid and at most dist away (64-bit); shadowed sites are skipped there and never crowded.
 *              Both are reported, not repaired.  flags = (shadowed ? 1 : 0) | (crowded ? 2 : 0).
 * Output:      all surviving sites in final order; the input indices of site k's members, in key order, at
 *              members[member_off[k] .. member_off[k + 1]); its distinct sample numbers, ascending, at samples[sample_off[k] ..
 *              sample_off[k + 1]).  The output is the same on every run.
 * TELR_E_ARG (text "telr_merge_sites: ..." in telr_last_error), on the host before any launch, *out untouched: n < 0; null entries
 *              with n > 0; a null out; dist < 0; min_samples < 1; a non-zero reserved field; a tid outside [0, n_targets); a negative
 *              pos, len, sample or group.  TELR_E_RANGE: 2^31 - 16 entries or more.  n == 0, or nothing surviving the filter: an empty
 *              result (nothing is launched at n == 0, nothing more once the filter's count is known).  opt NULL = the defaults. */
typedef struct telr_cohort_entry { int32_t tid, pos, len, sample, group; } telr_cohort_entry;
typedef struct telr_cohort_opt { int32_t dist;         /* 50 */
                                 int32_t min_samples;  /* 1  */
                                 int32_t reserved[2]; } telr_cohort_opt;
typedef struct telr_cohort_site { int32_t tid, pos, len, group, n_samples, n_members, n_sized, len_min, len_max, pos_min, pos_max, rep, flags, winner; } telr_cohort_site;
#define TELR_COHORT_SHADOWED 1
#define TELR_COHORT_CROWDED  2
typedef struct telr_cohort_sites telr_cohort_sites;
void telr_cohort_opt_default(telr_cohort_opt *o);
int  telr_merge_sites(telr_ctx *ctx, const telr_cohort_entry *e, int64_t n, int32_t n_targets, const telr_cohort_opt *opt, telr_cohort_sites **out);
int64_t telr_cohort_sites_count(const telr_cohort_sites *s);
const telr_cohort_site *telr_cohort_sites_sites(const telr_cohort_sites *s);
const int64_t *telr_cohort_sites_member_off(const telr_cohort_sites *s);      /* count + 1 offsets into telr_cohort_sites_members */
const int32_t *telr_cohort_sites_members(const telr_cohort_sites *s);
const int64_t *telr_cohort_sites_sample_off(const telr_cohort_sites *s);      /* count + 1 offsets into telr_cohort_sites_samples */
const int32_t *telr_cohort_sites_samples(const telr_cohort_sites *s);
void telr_cohort_sites_free(telr_cohort_sites *s);

/* ---- genotypes of those calls: reference reads, AF and GT (opt-in).  In the reference the three values come
 *      from Sniffles (`%AF`, `%GT`, `%DR`, src/telr/TELR_sv.py:161).  An OWN definition like the caller's, NOT Sniffles' genotyper;
 *      its agreement with Sniffles is unpinned.
 * Input: a result and calls as telr_call_insertions returns them: calls[n_calls] strictly ascending by (tid, pos), and the supporter
 *      set R_k of call k = reads[read_off[k] .. read_off[k + 1]), ascending and distinct.
 * Eligible records: not TELR_F_SECONDARY, mapq >= min_mapq.  An eligible record SPANS call k = (tid, pos) iff rec.tid == tid,
 *      rec.ts <= max(0, pos - flank) and rec.te >= pos + flank.
 * Window indel of a spanning record for call k: walk its CIGAR with p = ts.  An M of length l: p += l.  An I of length l adds l iff
 *      pos - flank <= p <= pos + flank (p unchanged).  A D of length l adds max(0, min(p + l, pos + flank) - max(p, pos - flank)),
 *      then p += l.  A record with n_cigar == 0 has window indel 0.  The pair is CLEAN iff window indel <= max_window_indel.
 * A read q outside R_k with at least one spanning record is a REFERENCE read of k if any of its spanning records is clean, and an
 *      AMBIGUOUS read of k otherwise.  Reads in R_k are neither.
 * Per call: alt = support; ref, ambig = the distinct reads of either kind, listed ascending at ref_reads[ref_off[k] ..
 *      ref_off[k + 1]) and ambig_reads[ambig_off[k] .. ambig_off[k + 1]); gt = 2 (1/1) if 100 * alt >= hom_pct * (alt + ref), else
 *      1 (0/1) if 100 * alt >= het_pct * (alt + ref), else 0 (0/0).  Ambiguous reads are in neither term.  Integer arithmetic only.
 * The CIGAR words are read on the device (the result's resident copy, TELR_MF_KEEP_CIGARS, or one upload).  The output is the same
 * on every run.  TELR_E_ARG (text in telr_last_error): a negative option, het_pct > hom_pct or either above 100, calls not strictly
 * ascending, a call's tid outside [0, n_targets) or a negative pos, a read list not ascending, a record that telr_call_insertions
 * would refuse.  TELR_E_RANGE from 2^31 - 16 (call, record) pairs on.  Zero calls: empty output.  Calls without a spanning record:
 * zeros and empty lists.  opt NULL = the defaults. */
typedef struct telr_geno_opt {
    int32_t flank;             /* 50 */
    int32_t min_mapq;          /* 20 */
    int32_t max_window_indel;  /* 20 */
    int32_t het_pct;           /* 30 */
    int32_t hom_pct;           /* 80 */
    int32_t reserved[3];       /* 0  */
} telr_geno_opt;
typedef struct telr_ins_gt { int32_t ref, ambig, alt, gt; } telr_ins_gt;
typedef struct telr_ins_geno telr_ins_geno;
void telr_geno_opt_default(telr_geno_opt *o);
int  telr_genotype_insertions(telr_ctx *ctx, const telr_result *r, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls,
                              const int64_t *read_off, const int32_t *reads, const telr_geno_opt *opt, telr_ins_geno **out);
int64_t telr_ins_geno_count(const telr_ins_geno *g);
const telr_ins_gt *telr_ins_geno_gt(const telr_ins_geno *g);
const int64_t *telr_ins_geno_ref_off(const telr_ins_geno *g);         /* count + 1 offsets into telr_ins_geno_ref_reads */
const int32_t *telr_ins_geno_ref_reads(const telr_ins_geno *g);
const int64_t *telr_ins_geno_ambig_off(const telr_ins_geno *g);       /* count + 1 offsets into telr_ins_geno_ambig_reads */
const int32_t *telr_ins_geno_ambig_reads(const telr_ins_geno *g);
void telr_ins_geno_free(telr_ins_geno *g);

/* ---- a draft contig per call, cut out of one of its supporting reads (opt-in).  Stands where the reference shells
 *      out to wtdbg2 or flye (src/telr/TELR_assembly.py:264-382).  An OWN definition: NOT an assembler, and NOT wtdbg2 or flye -- one
 *      supporting read is the backbone, the piece of it that carries the insertion between reference-aligned flanks is the draft.
 * Input: a result, the calls of telr_call_insertions on it (calls, read_off, reads as telr_genotype_insertions takes them), the
 *      signature array sigs[n_sig] as that call returned it (ascending by (tid, pos)), and read_set = the set the result was mapped from.
 * Walk of a record: states (p, u) start at (ts, qs').  M l: l unit steps (p + 1, u + 1).  I l: one step to (p, u + l).  D l: l unit
 *      steps (p + 1, u).  For a reference coordinate x: lo(x) = the smallest, hi(x) = the largest u over the states with p == x (an I
 *      at x lies between the two; an x inside a D has lo = hi).
 * Candidate of call k = (tid, pos, len): a signature s with kind 0 or 1, s.tid == tid, |s.pos - pos| <= reach and s.qid in R_k.  Then
 *      a = s.rec; b = s.rec (kind 0) or s.mate (kind 1); lpos = s.pos; rpos = s.pos (kind 0) or b.ts (kind 1);
 *      xL = max(a.ts, lpos - flank); xR = min(b.te, rpos + flank).  It is VALID iff both records have CIGAR ops,
 *      lpos - xL >= min_flank, xR - rpos >= min_flank, lo_a(xL) and hi_b(xR) exist, 1 <= n = hi_b(xR) - lo_a(xL) <= max_len, and
 *      0 <= lo_a(xL), hi_b(xR) <= qlen (true of every record whose CIGAR agrees with its coordinates).
 * Backbone: the valid candidate with the smallest key (|s.len - len|, -min(lpos - xL, xR - rpos), s.qid, s.rec, s.mate, index of s).
 * Draft:   bases [lo, hi) of the read on the record's strand; on the forward read start = lo, rc = 0 for a forward record and
 *      start = qlen - hi, rc = 1 on TELR_F_REV.  Sequence set_index of *set is that piece, reverse-complemented when rc == 1, so every
 *      draft is on the reference strand; an N keeps its mask bit.  ins_len = s.seg_len, ins_off = the strand coordinate of the
 *      signature's segment - lo.  A call without a valid candidate: sig = set_index = -1, zeros, no sequence; the set holds the
 *      other calls' drafts in call order.  It is made on the device from the packed words of read_set and is the caller's
 *      (telr_seqset_free).  Zero calls: an empty set, TELR_OK.
 * The CIGAR words are read on the device (the result's resident copy, TELR_MF_KEEP_CIGARS, or one upload).  The output is the same on
 * every run.  TELR_E_ARG (text in telr_last_error): a negative option, min_flank > flank, calls not strictly ascending, a tid, rec, mate
 * or qid out of range, a signature whose qid is not its records', signatures not ascending by (tid, pos), a read list not ascending, a
 * record that telr_call_insertions refuses, a read set whose count or lengths disagree with the records' qid / qlen.  TELR_E_RANGE from
 * 2^31 - 16 (signature, call) pairs on.  opt NULL = the defaults. */
typedef struct telr_draft_opt {
    int32_t flank;        /* 2000   */
    int32_t min_flank;    /* 500    */
    int32_t reach;        /* 50     */
    int32_t max_len;      /* 100000 */
    int32_t reserved[4];  /* 0      */
} telr_draft_opt;
typedef struct telr_draft { int32_t sig, qid, start, len, rc, ins_off, ins_len, set_index; } telr_draft;
typedef struct telr_drafts telr_drafts;
void telr_draft_opt_default(telr_draft_opt *o);
int  telr_draft_contigs(telr_ctx *ctx, const telr_result *r, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls,
                        const int64_t *read_off, const int32_t *reads, int64_t n_sig, const telr_ins_sig *sigs,
                        const telr_seqset *read_set, const telr_draft_opt *opt, telr_drafts **out, telr_seqset **set);
int64_t telr_drafts_count(const telr_drafts *d);                      /* = n_calls */
const telr_draft *telr_drafts_data(const telr_drafts *d);
void telr_draft_contigs_free(telr_drafts *d);

/* ---- a bridge of two reads for a call that no single read spans (opt-in; tests/bridge_ref.py is the checker).  A sibling
 *      of telr_draft_contigs for the calls it leaves without a draft: every supporting read runs from one flank into the element and
 *      ends there, so the call has clip signatures (kind 2) only.  An OWN definition: NOT an assembler, and NOT wtdbg2 or flye.  Two reads
 *      are joined at ONE shared k-mer; no consensus is formed (polishing follows, as it follows a draft).  Records only: the sequences are
 *      made by telr_seqset_join from the two pieces of a record.
 * Input, validation and the CIGAR source are those of telr_draft_contigs.  Strand coordinates qs', qe' as in telr_call_insertions; the
 *      walk and lo(x) / hi(x) as in telr_draft_contigs.  STRAND BASES of a record: the read as the record aligns it (the reverse
 *      complement of the forward read on TELR_F_REV).
 * Left candidate of call (tid, pos): a kind-2 signature s with s.tid == tid, |s.pos - pos| <= reach, s.qid in the call's read list and
 *      s.pos == a.te for a = s.rec (a tail clip).  cL = qlen - qe'_a; U = strand bases [qe'_a, qlen); xL = max(a.ts, s.pos - flank).
 *      VALID iff a has CIGAR ops, s.pos - xL >= min_flank, lo_a(xL) exists and is >= 0, and cL >= k.
 * Right candidate: a kind-2 signature with s.pos == b.ts for b = s.rec (a head clip).  cR = qs'_b; V = strand bases [0, qs'_b);
 *      xR = min(b.te, s.pos + flank).  VALID iff b has CIGAR ops, xR - s.pos >= min_flank, hi_b(xR) exists and is <= qlen, and cR >= k.
 * Ranking: each side by the key (-clip length, -flank length, qid, rec, index of s); the first `pairs` of each side are kept.  n_left
 *      and n_right are the valid counts before that cut.  Every kept (l, r) pair with different qid is voted.
 * Vote:   Wn = min(window, cL); the window is U[cL - Wn, cL).  A window k-mer is USABLE iff it lies wholly inside the window, none of
 *      its bases is N, and its value occurs exactly once among the window's N-free k-mers.  Every j in [0, cR - k] whose N-free k-mer of
 *      V equals a usable k-mer at U offset i is a MATCH (i, j) with diagonal d = i - j.  bin(d) = floor(d / 128) (towards minus
 *      infinity); score(b) = count(b) + count(b + 1); b* = the bin of the highest score, the smallest such b on a tie; votes =
 *      score(b*).  The BAND matches are those in bins b* and b* + 1; the JUNCTION (i*, j*) is the band match at the lower-median place
 *      when they are ordered by j (each j has at most one match); diag = i* - j*.
 * Pair choice: the pair with the most votes; on a tie the smaller left rank, then the smaller right rank.  It makes a bridge iff
 *      votes >= min_votes and 1 <= len_l + len_r <= max_len; otherwise the call has none -- no second pair is tried.
 * Bridge: left piece = strand bases [lo_a(xL), qe'_a + i*) of read a, right piece = strand bases [j*, hi_b(xR)) of read b; each is
 *      reported on the forward read with start = lo (forward) or qlen - hi (TELR_F_REV) and rc as a draft reports it.  ins_off =
 *      qe'_a - lo_a(xL); ins_len = i* + (cR - j*).  The contig is the left piece followed by the right piece: both read the same k
 *      bases at the junction, so an error-free pair joins without a seam.  sig_l / sig_r = the two signatures' indices.
 * A call with want[k] == 0 (want NULL = every call), or without a bridge: sig_l = sig_r = -1, n_left / n_right as found, zeros otherwise.
 * STATED LIMITS.  Two clips that do not overlap but share a repeat (the two LTRs of one element) are joined at the repeat: the contig
 *      then lacks what lies between them; the vote prefers the true overlap only when that overlap is longer than the repeat.  Chimeric
 *      reads are not detected.  An overlap shorter than about min_votes surviving k-mers is not found.  Recall on real elements is not
 *      measured.
 * The output is the same on every run.  TELR_E_ARG: what telr_draft_contigs refuses, plus k outside 11 .. 15, window outside k .. 4096,
 * pairs outside 1 .. 8, min_votes < 1.  TELR_E_RANGE from 2^31 - 16 (signature, call) pairs on.  opt NULL = the defaults. */
typedef struct telr_bridge_opt {
    int32_t flank;        /* 2000   */
    int32_t min_flank;    /* 500    */
    int32_t reach;        /* 50     */
    int32_t max_len;      /* 100000 */
    int32_t k;            /* 13     */
    int32_t window;       /* 4096   */
    int32_t min_votes;    /* 8      */
    int32_t pairs;        /* 4      */
} telr_bridge_opt;
typedef struct telr_bridge { int32_t sig_l, sig_r, qid_l, start_l, len_l, rc_l, qid_r, start_r, len_r, rc_r,
                             votes, diag, ins_off, ins_len, n_left, n_right; } telr_bridge;
typedef struct telr_bridges telr_bridges;
void telr_bridge_opt_default(telr_bridge_opt *o);
int  telr_bridge_contigs(telr_ctx *ctx, const telr_result *r, int32_t n_targets, int64_t n_calls, const telr_ins_call *calls,
                         const int64_t *read_off, const int32_t *reads, int64_t n_sig, const telr_ins_sig *sigs,
                         const telr_seqset *read_set, const uint8_t *want /* [n_calls], NULL = every call */,
                         const telr_bridge_opt *opt, telr_bridges **out);
int64_t telr_bridges_count(const telr_bridges *b);                    /* = n_calls */
const telr_bridge *telr_bridges_data(const telr_bridges *b);
void telr_bridge_contigs_free(telr_bridges *b);

/* ---- the reference's TE copies, annotated on the device for the liftover (opt-in).  Stands where the reference masks
 *      the reference genome with RepeatMasker and hands the BED to the liftover (src/telr/telr.py:132-159, TELR_te.py:391-469).  An OWN
 *      definition and NOT RepeatMasker: the library is indexed, the reference is cut into overlapping tiles that are mapped to it as
 *      queries, and the records become features by the interval rule below.  Hit sets differ from RepeatMasker's, above all for old,
 *      diverged copies; agreement with it is unpinned.  tests/refte_ref.py states the definition in plain Python.
 * Tiles (telr_tile_plan; host only, no device needed).  A target of length n gets no tile when n == 0, one when n <= tile, else
 *      1 + ceil((n - tile) / stride); tile j = (tid, j * stride, min(tile, n - j * stride)), listed in (tid, start) order.  Every
 *      interval of a target no longer than tile - stride + 1 lies whole inside at least one tile; no tile lies inside another.
 *      *needed = the number of tiles; when it exceeds cap nothing is copied and TELR_E_RANGE is returned: call again with
 *      cap >= *needed.  TELR_E_ARG: tile < 1, stride < 1 or > tile, tile >= 2^24 (the query limit of telr_map), a negative length, a
 *      null pointer where it is needed.  TELR_E_RANGE from 2^31 - 16 tiles on.  The callers' defaults: tile 32,768, stride 16,384
 *      (any library sequence up to 16 kb lies whole inside a tile).
 * Features (telr_annotate_hits).  r = a result whose queries are the tiles (qid = the tile's index) and whose targets are the library
 *      (tid = the family's index).
 * Hit:     a record that is not TELR_F_SECONDARY, with mapq >= min_mapq and qe - qs >= min_len: tid = tiles[qid].tid,
 *          start = tiles[qid].start + qs, end = tiles[qid].start + qe (qs / qe are on the forward query strand), family = rec.tid,
 *          strand = 1 on TELR_F_REV else 0, score = dp_score.
 * Order:   ascending by (tid, family, strand, start, end); hits with equal keys are interchangeable.
 * Feature: inside a run of equal (tid, family, strand) hit i opens a new feature iff it is the run's first or
 *          start_i >= M_i + join_gap, M_i = the maximum end of ALL earlier hits of the run (a running maximum, not the previous hit's
 *          end).  join_gap 0: only true overlaps join, book-ended tandem copies stay apart; join_gap 1: `bedtools merge`.
 *          Its fields: start of its first hit, maximum end, maximum score, n_hits.
 * Output:  ascending by (tid, start, end, family, strand); the bytes are the same on every run.  No CIGAR is read.
 * TELR_E_ARG (text in telr_last_error): a negative option, a qid outside [0, n_tiles), a record tid outside [0, n_families), a tile
 *      outside its target, qe > tiles[qid].len, coordinates out of order.  TELR_E_RANGE from 2^31 - 16 records on.  No hit: zero
 *      features, TELR_OK.  opt NULL = the defaults. */
typedef struct telr_tile { int32_t tid, start, len; } telr_tile;
int  telr_tile_plan(int32_t n_targets, const int32_t *target_len, int32_t tile, int32_t stride, telr_tile *out, int64_t cap, int64_t *needed);
typedef struct telr_refte_opt {
    int32_t min_len;   /* 100 */
    int32_t min_mapq;  /* 0   */
    int32_t join_gap;  /* 0   */
    int32_t reserved;  /* 0   */
} telr_refte_opt;
typedef struct telr_te_feat { int32_t tid, start, end, family, strand, score, n_hits; } telr_te_feat;
typedef struct telr_te_feats telr_te_feats;
void telr_refte_opt_default(telr_refte_opt *o);
int  telr_annotate_hits(telr_ctx *ctx, const telr_result *r, int64_t n_tiles, const telr_tile *tiles, int32_t n_targets,
                        const int32_t *target_len, int32_t n_families, const telr_refte_opt *opt, telr_te_feats **out);
int64_t telr_te_feats_count(const telr_te_feats *f);
const telr_te_feat *telr_te_feats_data(const telr_te_feats *f);
void telr_te_feats_free(telr_te_feats *f);

/* ---- a BAM file as input (opt-in).  The reference accepts a BAM as `--reads`: parse_input skips the alignment
 *      (src/telr/TELR_input.py:300-305) and bam2fasta makes the read file with `samtools fasta`, first name wins (:329-361).  Here
 *      the file is inflated and parsed on the device and becomes the two things the stage-1 consumers take: a resident read set and
 *      a result whose CIGARs are resident (telr_call_insertions, telr_genotype_insertions, telr_draft_contigs, telr_window_reads,
 *      telr_write_bam_dev, ...).  tests/bam_in_ref.py states the definition in plain Python.
 * Framing:  BGZF members (magic 1f 8b 08 04, the BC subfield anywhere among the extra subfields, CRC32 and ISIZE <= 65,536 at the end);
 *      members of ISIZE 0 anywhere; no_eof = 1 when the file does not end with the 28-byte EOF marker (accepted).  TELR_E_ARG with
 *      "block K" in telr_last_error: a truncated member, bytes that are no member, a deflate stream that is invalid (an over-subscribed
 *      code-length set, more than 286 / 30 symbols, no end-of-block code, bits that are no code, a length / distance symbol that does
 *      not exist; an incomplete set is accepted), that gives more or fewer bytes than ISIZE, reaches before the member's start or reads
 *      past its member, or a CRC mismatch.  Bytes between the stream's end and the trailer are ignored.  TELR_E_IO: the file cannot be read.
 * Stream:   the BAM header (magic, text, references; SAM specification 4.2) and records to the stream's end, either across any number
 *      of members.  A record that runs past the end, a block_size below 32, fields or tags that run past their record: TELR_E_ARG
 *      with "record K" (file order, from 0).
 * CIGAR of a mapped record (flag & 4 == 0, refID >= 0; refID >= n_ref or pos < 0 is TELR_E_ARG): the CG:B,I array when the record
 *      holds exactly <l_seq>S <n>N and that tag.  An H first / last and an S first / last or next to that H are clips (clip5, clip3 =
 *      their sums).  M = X -> M, D N -> D, I -> I, P and zero-length ops vanish, neighbours of one kind merge.  A clip elsewhere or
 *      an op code above 8: TELR_E_ARG.  A merged length >= 2^28, or coordinates >= 2^31: TELR_E_RANGE.  No M / I / D: the record is
 *      dropped (no_cigar).  qlen = clip5 + M + I + clip3, ts = pos, te = ts + M + D; qs = clip5, qe = qlen - clip3 forward,
 *      qs = clip3, qe = qlen - clip5 with flag 0x10.
 * Reads:    a record is sequence-bearing iff flag & 0x900 == 0, l_seq > 0 and it is unmapped or l_seq == qlen.  Read q = the q-th
 *      distinct QNAME in file order of its first sequence-bearing record; its bases are that record's SEQ (1 2 4 8 -> A C G T, any
 *      other code N), reverse-complemented with flag 0x10.  Qualities (Phred bytes, reversed with 0x10) are attached iff keep_qual
 *      and no sequence-bearing record's QUAL starts with 0xff; a kept value above 93 is TELR_E_ARG.
 * Records:  a mapped record with M / I / D is kept when its QNAME is a read's (else: orphans) and its qlen that read's length (else:
 *      len_mismatch).  blen = M + I + D; mlen = max(0, blen - NM) with an NM tag, else M; dp_score, cnt, score, subsc = AS, cm, s1,
 *      s2 (integer types c C s S i I, truncated to 32 bits; the last occurrence wins), else 0; n_sub = n_ambi = 0; mapq, tid = refID,
 *      tlen from the header.  flags: 0x100 -> TELR_F_SECONDARY, 0x800 -> TELR_F_SUPPL, neither -> TELR_F_PRIMARY, 0x10 -> TELR_F_REV.
 *      Order: qid, then class (neither; 0x800; 0x100), then file order; parent = the record's index within its read, 0 for a
 *      secondary; CIGAR words packed in that order.  2^31 - 16 or more members, records or reads: TELR_E_RANGE.  telr_bam_load
 *      holds the file next to its inflated stream in device memory; one that does not fit there: TELR_E_NOMEM (both live in the
 *      context's scratch until telr_release_scratch).  telr_bam_load_chunked has no such limit.
 * counters: members, records, mapped, kept, reads, orphans, len_mismatch, no_cigar, no_eof.  The set and the result belong to the
 *      handle (telr_bam_in_free frees them) until detached; after that they are the caller's (telr_seqset_free / telr_result_free)
 *      and the handle's accessors stay valid while they live.  Not read: CRAM, SAM, .csi, the header text beyond its length (the
 *      .bai is read by telr_bam_load_regions alone, below).
 * Chunked (telr_bam_load_chunked): the same result -- names, targets, counters, records, CIGAR words, the set's words and qualities,
 *      byte for byte -- for every accepted file and every chunk_bytes >= 1, with transient device memory that depends on the chunk and
 *      not on the file.  The file stays mapped on the host.  It is cut into chunks (telr_bam_chunk_plan: a chunk is a run of whole
 *      members in file order; it closes before the member whose ISIZE would take its sum of ISIZE above chunk_bytes and always holds
 *      at least one member; members of ISIZE 0 are members like any other); every chunk is uploaded, inflated and parsed in turn,
 *      chunk k + 1 inflating while chunk k is parsed.  The bytes of a chunk behind its last complete record (or all of it while the
 *      header is incomplete) are carried in front of the next chunk; a record or header longer than a chunk makes that carry grow
 *      and is no error.  Two passes: the first collects every record's fields and names, the host decides, the second inflates
 *      again and writes CIGAR words, bases and qualities where they stay.  A load of one chunk does not inflate again: its second
 *      pass reads the chunk where the first left it (passes is still 2: it counts the walks over the records).  Beyond the result
 *      and the set, the device holds two chunk slots (one when there is one chunk; the chunk's file bytes and its buffer: carry +
 *      inflated members), the per-record tables of one chunk and fixed tables.
 *      chunk_bytes: n > 0 that size; 0 the engine's own: free device memory (telr_device_mem) / 16, at least 1 MiB, at most 1 GiB;
 *      TELR_BAM_CHUNK_FIT: telr_bam_load's whole-file path when file size + sum of ISIZE is below half the free device memory, else
 *      as 0 (one hop of the member headers serves the decision and the load).
 *      Errors: framing (the hop over the whole file, before any upload) first, as in telr_bam_load; all others in chunk order, and
 *      within a chunk inflate (lowest block), header, record chain, records (lowest record); a quality above 93 in the second pass,
 *      lowest record.  Block and record numbers are the file's.  A file with one fault gives telr_bam_load's code and text (texts
 *      open with "telr_bam_load:" on either path); with several faults the chunk order may name another one than the whole-file
 *      order (there: inflate of every block, then the header, the chain, every record).  A failed load leaves nothing allocated
 *      beyond the context's scratch.
 *      telr_bam_in_chunk_info: chunks, passes run (1 when nothing is kept and there is no read), the largest chunk buffer (bytes
 *      allocated for one slot: carry room + inflated members; at most 64 KiB above the largest carry + the largest chunk's members,
 *      so at most max(chunk_bytes, 65,536) + largest carry + 64 KiB), the largest carry (bytes); all 0 after a whole-file load. */
#define TELR_BAM_CHUNK_FIT (-1)
typedef struct telr_bam_in telr_bam_in;
int  telr_bam_load(telr_ctx *ctx, const char *path, int32_t keep_qual, telr_bam_in **out);
int  telr_bam_load_chunked(telr_ctx *ctx, const char *path, int32_t keep_qual, int64_t chunk_bytes, telr_bam_in **out);
/* host only, no device needed.  first_member_of_chunk[c] for c < min(*n_chunks, cap).  TELR_E_ARG: a null pointer, a negative count
 * or ISIZE, chunk_bytes < 1; TELR_E_RANGE: more chunks than cap (the first cap are written and *n_chunks is exact: call again) */
int  telr_bam_chunk_plan(int64_t n_members, const int32_t *isize, int64_t chunk_bytes, int64_t *first_member_of_chunk, int64_t cap, int64_t *n_chunks);
int  telr_bam_in_chunk_info(const telr_bam_in *in, int64_t *out /* [4] */);
void telr_bam_in_free(telr_bam_in *in);
int32_t telr_bam_in_target_count(const telr_bam_in *in);
const char *const *telr_bam_in_target_names(const telr_bam_in *in);
const int32_t *telr_bam_in_target_lens(const telr_bam_in *in);
int32_t telr_bam_in_read_count(const telr_bam_in *in);
const char *const *telr_bam_in_read_names(const telr_bam_in *in);
const int32_t *telr_bam_in_read_lens(const telr_bam_in *in);
telr_seqset *telr_bam_in_seqset(const telr_bam_in *in);
telr_result *telr_bam_in_result(const telr_bam_in *in);
telr_seqset *telr_bam_in_detach_seqset(telr_bam_in *in);      /* NULL when detached before */
telr_result *telr_bam_in_detach_result(telr_bam_in *in);
int  telr_bam_in_counters(const telr_bam_in *in, int64_t *out /* [9] */);
/* the `bam2fasta` text, decoded on demand on the device: buf[off[q] .. off[q] + len[q]) = read q, off[q] = the bases before it */
int  telr_bam_in_ascii(const telr_bam_in *in, char *buf, int64_t *off);
/* milliseconds of the load's phases: host hop, upload, inflate, chain, parse, names on the host, sequences, total.  After either load
 * they are sums over the chunks (upload, inflate: both passes, device time between events on the second stream; chain: device time;
 * parse: host time of pass 1 behind the chain; sequences: the whole second pass, wall clock); total is wall clock.  With more than one
 * chunk upload and inflate overlap with the others, so total is not the sum of the rest.  telr_bam_load is the load of one chunk: its
 * upload, inflate and chain used to be host wall clock, each ending in a synchronisation, and are device times between events now */
int  telr_bam_in_phase_ms(const telr_bam_in *in, float *out /* [8] */);

/* ---- only the regions asked for, through the .bai (opt-in).  `samtools view file.bam chr:beg-end` as a load: only the
 *      BGZF members that the index names are uploaded and inflated; their records are chained, filtered by true overlap and parsed on
 *      the device.  tests/bam_region_ref.py states the definition in plain Python.
 * Regions:  (tid, beg, end), 0-based, half-open; any order, overlapping or touching.  The host clips end to the target's length (and to
 *      2^29, the reach of a .bai), sorts them and merges them into disjoint ascending regions per target.  TELR_E_ARG before anything is
 *      read beyond the header: a tid outside the header's targets, beg < 0, end <= beg after clipping, a non-zero reserved field,
 *      n_regions < 0, a null pointer with n_regions > 0.  Zero regions: the header's targets, no read, no record; nothing beyond the
 *      header is inflated and the index is not opened.
 * Selection:  a record is selected iff it is mapped (flag & 4 == 0, refID >= 0) and its reference span [pos, pos + max(1, M + D))
 *      overlaps a region on tid == refID: pos < end and pos + span > beg.  M and D are those of the CIGAR rules above, the CG:B,I array in
 *      force where they say so.  Unmapped records are never selected, placed ones included.
 * Result:   what telr_bam_load gives for a BAM that holds this file's header and exactly the selected records in file order -- targets,
 *      names, lengths, the set's words, mask words and qualities, records, CIGAR words and the counters records .. no_cigar, byte for
 *      byte, for every file that the whole-file load accepts.  members counts the members inflated for the intervals; no_eof is the
 *      file's.  A CONSEQUENCE: a read whose sequence-bearing record (neither 0x100 nor 0x800) lies outside the regions has no read here,
 *      and its selected records are orphans, exactly as after `samtools view` of the region.  Nothing repairs that.
 * Index:    <bam>.bai, or the path given; SAM specification 5.2: magic, n_ref, per reference the bins with their chunks and the 16-kb
 *      linear index, the optional n_no_coor; pseudo-bin 37450 is skipped.  Per merged region: the chunks of all bins of reg2bins(beg,
 *      end); a chunk whose end is at or below the linear index's entry for beg >> 14 is dropped (an entry of 0 is unset and drops
 *      nothing, and so does a window behind the last entry); an empty chunk (beg >= end) is dropped.  All regions' chunks are sorted by
 *      start, and two become one INTERVAL when the next starts in, or before, the member in which the current one ends (coffset(next.beg)
 *      <= coffset(cur.end)): no member belongs to two intervals and none is inflated twice.  An interval [vbeg, vend) is the members from
 *      coffset(vbeg) to coffset(vend), the last one only when uoffset(vend) > 0; they are hopped from coffset(vbeg), not from the file's
 *      start.  Its records start at uoffset(vbeg) in the first member and their chain must end exactly at uoffset(vend) in the last: a
 *      chain that runs past that point or stops before it, a record with block_size < 32, an offset beyond its member's ISIZE, or members
 *      that do not meet coffset(vend) are TELR_E_ARG, "the index does not match the file at virtual offset V".
 *      TELR_E_IO: the .bai cannot be read.  TELR_E_ARG: wrong magic; n_ref is not the header's; a count or a chunk runs past the index's
 *      end; a coffset at or beyond the BAM's size; a coffset that does not start with the BGZF magic.  A stale index that passes these
 *      checks and chains cannot be told from a fresh one.
 * Records:  every record walked inside an interval is checked as in telr_bam_load, selected or not (the bins over-select: more is walked
 *      than kept).  File-order numbers are unknown here: texts say "record at virtual offset V" and "block at file offset P".
 * Header:   read in a step of its own: the members from file offset 0, as few as hold it.  A member that also opens the first interval is
 *      inflated a second time there -- the only exception to "no member twice", counted apart (region_info[3]).
 * Chunks:   the intervals' members in file order are cut by telr_bam_chunk_plan as in telr_bam_load_chunked (chunk_bytes as there;
 *      TELR_BAM_CHUNK_FIT decides on the intervals' bytes); an interval may span chunks (the carry goes on) and a chunk may hold many
 *      intervals.  telr_bam_in_chunk_info and telr_bam_in_phase_ms keep their meaning (host hop: the index plan and the intervals' hops).
 * telr_bam_in_region_info: merged regions, intervals, members inflated for the intervals, header members, records walked, records
 *      selected; all 0 after the other two loads.  telr_bam_in_region_bytes: file bytes uploaded for the intervals, both passes.
 * telr_bai_plan: host only, no device needed: the intervals of `regions` (not clipped to target lengths: it has none) over an index of
 *      n_ref references, vbeg[i] / vend[i] for i < min(*n_intervals, cap).  TELR_E_RANGE: more intervals than cap (the first cap are
 *      written and *n_intervals is exact: call again).  telr_bai_plan_error: the reason of the calling thread's last refusal. */
typedef struct telr_region { int32_t tid, beg, end, reserved; } telr_region;
int  telr_bam_load_regions(telr_ctx *ctx, const char *bam_path, const char *bai_path /* NULL: bam_path + ".bai" */, int32_t keep_qual, int64_t chunk_bytes,
                           int64_t n_regions, const telr_region *regions, telr_bam_in **out);
int  telr_bam_in_region_info(const telr_bam_in *in, int64_t *out /* [6] */);
int64_t telr_bam_in_region_bytes(const telr_bam_in *in);
int  telr_bai_plan(const char *bai_path, int32_t n_ref, int64_t n_regions, const telr_region *regions, uint64_t *vbeg, uint64_t *vend, int64_t cap, int64_t *n_intervals);
const char *telr_bai_plan_error(void);

/* ---- a FASTA / FASTQ file -- plain, gzip or BGZF -- as a read set, parsed and packed on the device (opt-in).  The
 *      text is never held as host text: it goes to the device in chunks (inflated there for BGZF, by one host thread running zlib for
 *      gzip) and becomes names, lengths, 2-bit words, mask words and Phred bytes in the set's layout.  tests/reads_in_ref.py states
 *      the definition in plain Python.
 * Container, by content: BGZF -- the file opens 1f 8b 08 and telr_bam_load's framing accepts the whole file (every member a BC subfield
 *      and ISIZE <= 65,536; empty members anywhere; no EOF marker: no_eof = 1, accepted); gzip -- any other file that opens 1f 8b: one
 *      or several RFC 1952 members of any size, zlib checks each CRC and ISIZE; plain -- a file that opens '@' or '>'; an empty file is
 *      an empty set; anything else TELR_E_ARG.
 * Text:  lines end in "\n", the last one may lack it; one "\r" directly before the "\n", or at the end of the text, belongs to the
 *      terminator.  The first byte decides the kind.  FASTQ ('@'): lines in fours -- line 4k starts with '@', line 4k + 1 holds the
 *      bases, line 4k + 2 starts with '+' (the rest of it is ignored), line 4k + 3 holds as many quality characters; anything else
 *      (an empty line where '@' is due, a trailing empty line, a record on more lines, 1 - 3 lines at the end) is TELR_E_ARG naming
 *      the lowest offending record.  FASTA ('>'): a line that starts with '>' opens a record, every other line adds its bytes without
 *      the terminator, an empty line adds nothing, a header alone is a record of length 0.  A name: the bytes behind the '@' / '>' up
 *      to the first space, tab, "\r" or the line's end; it may be empty.  Bases as in telr_seqset_create: A C G T U in either case are
 *      codes 0 1 2 3 3, any other byte sets the mask bit and has code 0, padding up to 64 bases has code 0 and mask 0.
 * Qualities:  keep_qual on a FASTQ: the set carries byte - 33; a character outside 33 .. 126 is TELR_E_ARG naming the lowest record.
 *      Without keep_qual only the quality line's length is checked.  A FASTA with keep_qual gives a set without qualities.
 * Limits:  a record above INT32_MAX bases, or 2^31 - 16 records or more: TELR_E_RANGE.
 * Errors:  every text opens with "telr_reads_load:"; "record N: ..." for grammar and qualities (the lowest record; in one record
 *      grammar first), "block K: ..." for a BGZF member (telr_bam_load's texts), "gzip: ..." for what zlib reports.  They are found in
 *      chunk order; a file with one fault gives the same code and text at every chunk_bytes.  A failed load leaves nothing allocated
 *      beyond the context's scratch.
 * Chunks:  chunk_bytes: n > 0 that many bytes of text at the most (BGZF: telr_bam_chunk_plan over the members' ISIZE; gzip and plain:
 *      consecutive chunk_bytes of text, of which those below 4 KiB that close no record are gathered on the host up to 4 KiB);
 *      0 the engine's own size, as in telr_bam_load_chunked; negative: TELR_E_ARG.  The result does not depend on it.  One pass: each
 *      chunk's words are written as a piece and the pieces are copied end to end into the set at the end, so the transient device
 *      memory is one more copy of the finished set's arrays (with keep_qual that includes a byte per base) plus two chunk slots.
 * counters: container (0 plain, 1 gzip, 2 BGZF), fastq (1 / 0), members (BGZF or gzip members; 0 for plain), text_bytes, lines,
 *      records, bases, no_eof.  chunk_info: chunks, the largest chunk buffer (bytes), the largest carry, peak transient device bytes.
 *      phase_ms: host hop, upload, inflate (gzip: the zlib thread's time), lines, records, names, pack, join, total (wall clock; upload
 *      and inflate overlap with the rest). */
typedef struct telr_reads_in telr_reads_in;
int  telr_reads_load(telr_ctx *ctx, const char *path, int32_t keep_qual, int64_t chunk_bytes, telr_reads_in **out);
void telr_reads_in_free(telr_reads_in *in);
int32_t telr_reads_in_count(const telr_reads_in *in);
const char *const *telr_reads_in_names(const telr_reads_in *in);
const int32_t *telr_reads_in_lens(const telr_reads_in *in);
telr_seqset *telr_reads_in_seqset(const telr_reads_in *in);
telr_seqset *telr_reads_in_detach_seqset(telr_reads_in *in);      /* NULL when detached before */
int  telr_reads_in_counters(const telr_reads_in *in, int64_t *out /* [8] */);
int  telr_reads_in_chunk_info(const telr_reads_in *in, int64_t *out /* [4] */);
int  telr_reads_in_phase_ms(const telr_reads_in *in, float *out /* [9] */);

/* ---- window reads (a12) -------------------------------------------------------
 * Replaces the per-locus `pysam.AlignmentFile(bam).fetch(chr, bp-1000, bp+1000)` loop of prep_assembly_inputs
 * (src/telr/TELR_assembly.py:384-415, read_type="all"): for every window w = (win_tid, [win_lo, win_hi)) the ascending,
 * distinct query ids with ANY record (primary, secondary, supplementary) overlapping it: ts < win_hi and te > win_lo.
 * recs: any array of records (telr_result_alns of the stage-1 result, or records put together by the caller).  Host
 * code, no device needed.  out_off[n_win+1]; the ids of window w are out_qid[out_off[w] .. out_off[w+1]).  *needed =
 * total number of ids; when it exceeds cap nothing is copied and TELR_E_RANGE is returned: call again with cap >= *needed. */
int  telr_window_reads(const telr_aln *recs, int64_t n_rec, int32_t n_win, const int32_t *win_tid, const int32_t *win_lo,
                       const int32_t *win_hi, int64_t *out_off, int32_t *out_qid, int64_t cap, int64_t *needed);

/* ---- timing of the last telr_map / telr_index_build call (HIP events on the
 *      engine's own stream).  Stage names: telr_stage_name(i). ---------------- */
#define TELR_N_STAGES 16
int  telr_stage_ms(const telr_ctx *ctx, float *ms_out /* [TELR_N_STAGES] */);
const char *telr_stage_name(int i);
/* algorithmic work counters of the last telr_map call (SURVEY §8d terms) */
typedef struct telr_counters {
    int64_t query_bases, minimizers, probes, anchors, chains, dp_problems, dp_cells,
            window_bases, cigar_ops, records;
    /* engine-only (the oracle leaves them 0): queries with more anchors than one workgroup sorts in LDS (a read in a tandem
     * array / satellite), and the ranges that held at least one such query and therefore took the two-step seeding + the
     * library's segmented sort for it */
    int64_t over_queries, over_ranges;
} telr_counters;
int  telr_last_counters(const telr_ctx *ctx, telr_counters *out);
/* per DP class (TELR_N_DPCLS classes) of the last telr_map call:
 * out[c*4+0] problems, [c*4+1] DP cells, [c*4+2] anti-diagonal steps (sum of m+n),
 * [c*4+3] algorithmic bytes (2-bit bases read once + 4 B per CIGAR run + 32 B result) */
#define TELR_N_DPCLS 25
int  telr_last_dp_classes(const telr_ctx *ctx, int64_t *out /* [TELR_N_DPCLS*4] */);
/* what defines each DP class (no device needed): widest band in diagonals, lanes per problem, registers per lane, dwords per
 * trace-back row, trace-back interleaved across the problems of a wave (0/1), trace-back in tiles of four rows (0/1) */
int  telr_debug_dp_class_table(int32_t *out /* [TELR_N_DPCLS][6] */);
/* how telr_map would cut reads of these lengths into ranges and run them (no device needed; TELR_BATCH_MBP / TELR_BATCH_KBP /
 * TELR_PIPELINE are read as telr_map reads them).  max_len: the longest read; per_base: anchors per read base (0: unknown);
 * has_qtarget / vote: the call has per-query targets / sub-read voting applies to it; debug, pipe_nomem: the context's.
 * out[0] mode (0 one range at a time, 1 per-query targets: one range, else the ranges in turn, 2 two ranges in flight),
 * out[1] bases per range at most, out[2] number of ranges; range_end (nullable, n entries suffice): the end of every range */
int  telr_debug_map_plan(const int32_t *len, int32_t n, int32_t max_len, double per_base, int has_qtarget, int vote, int debug,
                         int pipe_nomem, int64_t *out /* [3] */, int32_t *range_end);
/* ---- test taps behind the banded DP: CIGAR stitching, the per-chain sums and the retry pass, as telr_map runs them ----
 * telr_debug_stitch: the stitch and chain-sum kernels on hand-made per-problem results.  Chain k owns the problems
 * [p_off[k], p_off[k + 1]) (at least one each) and reads its first one forwards when has_left[k]; prob: five ints per problem
 * {score, bi, bj, mlen, mcols}; the CIGAR words (len << 4 | op, op 0..2) of problem x are cig[cig_off[x] .. cig_off[x + 1]) in
 * storage order: end to start of the DP problem, as the trace-back leaves them.  cx_scale as in telr_map_opt (0: no rounding).
 * chain_out: nine ints per chain {dp, mlen, blen, l_bi, l_bj, r_bi, r_bj, n_cigar, first op in cig_out}.
 * TELR_E_RANGE when cig_cap ops do not hold the stitched CIGARs. */
int  telr_debug_stitch(telr_ctx *ctx, int32_t n_chain, const int32_t *p_off, const int32_t *has_left, const int32_t *prob,
                       const int64_t *cig_off, const uint32_t *cig, int32_t cx_scale, int32_t *chain_out, uint32_t *cig_out,
                       int64_t cig_cap);
/* telr_debug_align: both DP passes, stitching and the records' numbers of a caller's chains.  chains: seven ints per chain {qid,
 * tid, rev, qs, qe, rs, re}, the query interval on the chain's strand; chain k owns the rows [prob_off[k], prob_off[k + 1]) of
 * probs, twelve ints each {qid, q_off, tid, t_off, m, n, dlo, dhi, kind, qstep, tstep, qcomp} with the bands telr_map builds:
 * [kind 1]? (kind 0 | 3 | 5)+ [kind 2]? on the chain's sequences and strand, the kind-1 row (left extension) exactly when qs > 0
 * and rs > 0, the kind-2 row (right extension) exactly when qe < qlen and re < tlen.  chain_out: nine ints per chain {qs, qe, ts,
 * te, mlen, blen, dp_score, n_cigar, first op in cig_out} as in a record; prob_out: nine ints per problem {DP class of the first
 * pass, retry flag, score, bi, bj, mlen, mcols, CIGAR ops, cells} after the retry pass; *n_retry: problems on the retry list;
 * acc_out: the per-class accounts (telr_last_dp_classes) and, last, the sum of the target window bases. */
int  telr_debug_align(telr_ctx *ctx, const telr_seqset *queries, const telr_seqset *targets, const telr_map_opt *mo, int32_t n_chain,
                      const int32_t *chains, const int32_t *prob_off, const int32_t *probs, int32_t *chain_out, int32_t *prob_out,
                      uint32_t *cig_out, int64_t cig_cap, int32_t *n_retry, int64_t *acc_out /* [TELR_N_DPCLS*4 + 1] */);

#ifdef __cplusplus
}
#endif
#endif /* TELR_HIP_H */
