// sam_host.hip.h — the host writers: PAF, SAM, and the coordinate-sorted BAM + .bai built on the CPU.  Included by
// telr_engine.hip (they read telr_result and run on the host pool).  What a record, the header and the index consist of is in
// sam_records.h; here a writer is layout -> walk -> print (SAM) or layout -> walk -> encode, sort, BGZF blocks, index (BAM).
// The reference's call sites consume PAF columns 0,1,4,5,7,8,9,10,11 (TELR_liftover.py:215-240,356-380; TELR_te.py:89-95,136-142)
// and SAM records with NM/MD/AS/SA/cs (hand-off H1: Sniffles, samtools depth, pysam; docs/02_Usage.md:76).
#pragma once
#include <zlib.h>

static void cigar_text(const uint32_t *cg, int n, int clip5, int clip3, char clipc, std::string &out)
{
    char buf[24];
    if (clip5 > 0) { snprintf(buf, sizeof(buf), "%d%c", clip5, clipc); out += buf; }
    for (int i = 0; i < n; ++i) { snprintf(buf, sizeof(buf), "%u%c", cg[i] >> 4, "MID"[cg[i] & 0xf]); out += buf; }
    if (clip3 > 0) { snprintf(buf, sizeof(buf), "%d%c", clip3, clipc); out += buf; }
}

extern "C" int telr_write_paf(const telr_result *r, const char *const *qnames, const char *const *tnames, int with_cigar,
                              const char *path, int append)
{
    if (!r || !qnames || !tnames) return TELR_E_ARG;
    result_wait(r);
    FILE *f = path ? fopen(path, append ? "a" : "w") : stdout;
    if (!f) return TELR_E_ARG;
    std::string line;
    for (const telr_aln &a : r->alns) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s\t%d\t%d\t%d\t%c\t%s\t%d\t%d\t%d\t%d\t%d\t%d\tNM:i:%d\tAS:i:%d\ttp:A:%c\tcm:i:%d\ts1:i:%d",
                 qnames[a.qid], a.qlen, a.qs, a.qe, (a.flags & TELR_F_REV) ? '-' : '+', tnames[a.tid], a.tlen, a.ts, a.te, a.mlen, a.blen, a.mapq,
                 a.blen - a.mlen, a.dp_score, (a.flags & TELR_F_SECONDARY) ? 'S' : 'P', a.cnt, a.score);
        line = buf;
        if (!(a.flags & TELR_F_SECONDARY)) { snprintf(buf, sizeof(buf), "\ts2:i:%d", a.subsc); line += buf; }
        if (with_cigar && a.n_cigar > 0) { line += "\tcg:Z:"; cigar_text(r->cig + a.cigar_off, a.n_cigar, 0, 0, 'S', line); }
        line += '\n';
        fwrite(line.data(), 1, line.size(), f);
    }
    if (path) fclose(f);
    return TELR_OK;
}

// the quality arguments of the _qual writers: every byte of every read inside phred_offset .. phred_offset + 93 (checked before
// a file is opened)
static int qual_args_check(const char *q_qual, const int64_t *q_qual_off, int32_t phred_offset, int32_t n_queries, const int32_t *q_len)
{
    if (!q_qual) return TELR_OK;
    if (!q_qual_off || phred_offset < 0 || phred_offset > 255 - 93) return TELR_E_ARG;
    for (int q = 0; q < n_queries; ++q) {
        const unsigned char *src = (const unsigned char*)q_qual + q_qual_off[q];
        for (int x = 0; x < q_len[q]; ++x) if (src[x] < phred_offset || src[x] > phred_offset + 93) return TELR_E_ARG;
    }
    return TELR_OK;
}
// the read on the other strand
static void revcomp_into(const char *qs, int ql, std::string &rc)
{
    rc.resize((size_t)ql);
    for (int x = 0; x < ql; ++x) rc[x] = COMP_TAB[(unsigned char)qs[ql - 1 - x]];
}

extern "C" int telr_write_sam_qual(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                                   const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                                   const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                                   const char *pg_line, const char *path, const char *q_qual, const int64_t *q_qual_off, int32_t phred_offset)
{
    if (!r || !qnames || !q_ascii || !q_off || !q_len || !tnames || !t_ascii || !t_off || !t_len) return TELR_E_ARG;
    if (qual_args_check(q_qual, q_qual_off, phred_offset, n_queries, q_len) != TELR_OK) return TELR_E_ARG;
    result_wait(r);
    FILE *f = path ? fopen(path, "w") : stdout;
    if (!f) return TELR_E_ARG;
    const bool sorted = (flags & TELR_SAM_SORTED) != 0, prim_only = (flags & TELR_SAM_PRIMARY_ONLY) != 0;
    if (!(flags & TELR_SAM_NO_HEADER)) {
        const std::string text = sam_header_text(sorted, n_targets, tnames, t_len, rg_id, rg_sm, rg_lb, pg_line);
        fwrite(text.data(), 1, text.size(), f);
    }
    // TELR_SAM_SORTED: lines are collected with their key and written in coordinate order, unmapped reads last (what
    // `samtools sort | samtools view` prints)
    std::vector<std::pair<int64_t, std::string>> keyed;
    auto emit = [&](int64_t key, const std::string &l) { if (sorted) keyed.emplace_back(key, l); else fwrite(l.data(), 1, l.size(), f); };
    // records are sorted by (qid, rank); group per query
    const size_t n = r->alns.size();
    size_t i = 0;
    std::string rc, line, md, cs, sa, qfw, qrv;
    char buf[64];
    for (int q = 0; q < n_queries; ++q) {
        size_t j = i;
        while (j < n && r->alns[j].qid == q) ++j;
        const char *qs = q_ascii + q_off[q]; const int ql = q_len[q];
        if (q_qual) {          // Phred + 33, in the read's direction and reversed
            const unsigned char *src = (const unsigned char*)q_qual + q_qual_off[q];
            qfw.resize((size_t)ql);
            for (int x = 0; x < ql; ++x) qfw[x] = (char)(src[x] - phred_offset + 33);
            qrv.assign(qfw.rbegin(), qfw.rend());
        }
        if (j == i) {
            if (!(flags & TELR_SAM_NO_UNMAPPED)) {
                line.clear(); line += qnames[q]; line += "\t4\t*\t0\t0\t*\t*\t0\t0\t";
                if (ql > 0) line.append(qs, (size_t)ql); else line += '*';
                line += '\t';
                if (q_qual && ql > 0) line += qfw; else line += '*';
                if (rg_id) { line += "\tRG:Z:"; line += rg_id; }
                line += '\n';
                emit(SAM_KEY_UNMAPPED, line);
            }
            continue;
        }
        revcomp_into(qs, ql, rc);
        for (size_t k = i; k < j; ++k) {
            const telr_aln &a = r->alns[k];
            const RecLayout L = rec_layout(a, ql, flags);
            if (prim_only && (L.sec || L.sup)) continue;                 // samtools view -F0x900
            const char *qstr = L.rev ? rc.data() : qs;                   // query on the alignment strand
            const uint32_t *cg = r->cig + a.cigar_off;
            md.clear(); cs.clear();
            const int nm = aln_walk(qstr, t_ascii + t_off[a.tid], cg, a.n_cigar, L.clip5, a.ts, flags, md, cs);
            line.clear();
            line += qnames[q];
            snprintf(buf, sizeof(buf), "\t%d\t", L.flag); line += buf;
            line += tnames[a.tid];
            snprintf(buf, sizeof(buf), "\t%d\t%d\t", a.ts + 1, a.mapq); line += buf;
            if (a.n_cigar > 0) cigar_text(cg, a.n_cigar, L.clip5, L.clip3, L.hard ? 'H' : 'S', line); else line += '*';
            line += "\t*\t0\t0\t";
            // SEQ, and QUAL: the qualities of the bases SEQ holds, in its orientation; '*' where there is none
            if (L.l_seq > 0) line.append(qstr + L.seq_lo, (size_t)L.l_seq); else line += '*';
            line += '\t';
            if (q_qual && L.l_seq > 0) line.append((L.rev ? qrv : qfw).data() + L.seq_lo, (size_t)L.l_seq); else line += '*';
            snprintf(buf, sizeof(buf), "\tNM:i:%d\tAS:i:%d", nm, a.dp_score); line += buf;
            if (flags & TELR_SAM_MD) { line += "\tMD:Z:"; line += md; }
            if (flags & TELR_SAM_CS) { line += "\tcs:Z:"; line += cs; }
            if (!L.sec) {
                sa.clear();
                sa_text(&r->alns[i], j - i, k - i, ql, r->cig, tnames, sa);
                if (!sa.empty()) { line += "\tSA:Z:"; line += sa; }
            }
            snprintf(buf, sizeof(buf), "\ttp:A:%c\tcm:i:%d\ts1:i:%d", L.sec ? 'S' : 'P', a.cnt, a.score); line += buf;
            if (!L.sec) { snprintf(buf, sizeof(buf), "\ts2:i:%d", a.subsc); line += buf; }
            if (rg_id) { line += "\tRG:Z:"; line += rg_id; }
            line += '\n';
            emit(L.key, line);
        }
        i = j;
    }
    if (sorted) {
        std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<int64_t, std::string> &x, const std::pair<int64_t, std::string> &y) { return x.first < y.first; });
        for (auto &kv : keyed) fwrite(kv.second.data(), 1, kv.second.size(), f);
    }
    if (path) fclose(f);
    return TELR_OK;
}
extern "C" int telr_write_sam(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                              const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                              const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                              const char *pg_line, const char *path)
{
    return telr_write_sam_qual(r, n_queries, qnames, q_ascii, q_off, q_len, n_targets, tnames, t_ascii, t_off, t_len, flags, rg_id, rg_sm, rg_lb, pg_line, path, nullptr, nullptr, 0);
}

// ---------------------------------------------------------------------------------------
// Coordinate-sorted BAM + BAI (replaces `samtools sort -o BAM SAM; samtools index BAM`,
// reference src/telr/TELR_alignment.py:103-114; hand-off H1 to Sniffles / pysam).
static bool bgzf_block(const char *src, size_t n, int level, std::string &out)
{
    uLong bound = compressBound((uLong)n) + 64;
    out.resize(18 + bound + 8);
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    zs.next_in = (Bytef*)src; zs.avail_in = (uInt)n; zs.next_out = (Bytef*)&out[18]; zs.avail_out = (uInt)bound;
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { deflateEnd(&zs); return false; }
    size_t clen = zs.total_out; deflateEnd(&zs);
    memcpy(&out[0], BGZF_HEAD, sizeof(BGZF_HEAD));
    uint16_t bsize = (uint16_t)(clen + 25);
    memcpy(&out[16], &bsize, 2);
    uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)src, (uInt)n), isize = (uint32_t)n;
    memcpy(&out[18 + clen], &crc, 4); memcpy(&out[18 + clen + 4], &isize, 4);
    out.resize(18 + clen + 8);
    return true;
}
// the part of a BAM record that mapped and unmapped reads share: the fixed fields, the name, the CIGAR words, SEQ and QUAL of
// bases [seq_lo, seq_lo + l_seq) of qstr.  qual: the read's quality bytes in ITS direction (null: 0xff).  block_size stays 0
// until bam_rec_close.
static void bam_rec_open(std::string &o, int32_t tid, int32_t pos, int mapq, int bin, int flag, const char *name, const uint32_t *cig, uint32_t n_cig,
                         const char *qstr, int seq_lo, int l_seq, const unsigned char *qual, int32_t phred_offset, bool rev, int ql)
{
    const size_t l_name = strlen(name) + 1;
    put32(o, 0);
    put32(o, (uint32_t)tid); put32(o, (uint32_t)pos);
    o += (char)(uint8_t)l_name; o += (char)(uint8_t)mapq; put16(o, (uint16_t)bin);
    put16(o, (uint16_t)n_cig); put16(o, (uint16_t)flag);
    put32(o, (uint32_t)l_seq); put32(o, (uint32_t)-1); put32(o, (uint32_t)-1); put32(o, 0);
    o.append(name, l_name);
    if (n_cig) o.append((const char*)cig, (size_t)n_cig * 4);
    for (int x = 0; x < l_seq; x += 2) { const uint8_t hi = nt16(qstr[seq_lo + x]), lo = x + 1 < l_seq ? nt16(qstr[seq_lo + x + 1]) : 0; o += (char)(hi << 4 | lo); }
    // QUAL: Phred values (not + 33) of SEQ's bases in SEQ's orientation
    if (!qual) o.append((size_t)l_seq, (char)0xff);
    else for (int x = 0; x < l_seq; ++x) o += (char)(qual[rev ? ql - 1 - (seq_lo + x) : seq_lo + x] - phred_offset);
}
static void bam_rec_close(std::string &o) { const uint32_t bs = (uint32_t)o.size() - 4; memcpy(&o[0], &bs, 4); }

extern "C" int telr_write_bam_qual(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                                   const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                                   const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                                   const char *pg_line, const char *bam_path, int32_t write_index, int32_t level,
                                   const char *q_qual, const int64_t *q_qual_off, int32_t phred_offset)
{
    if (!r || !qnames || !q_ascii || !q_off || !q_len || !tnames || !t_ascii || !t_off || !t_len || !bam_path) return TELR_E_ARG;
    if (qual_args_check(q_qual, q_qual_off, phred_offset, n_queries, q_len) != TELR_OK) return TELR_E_ARG;
    auto qual_of = [&](int q) { return q_qual ? (const unsigned char*)q_qual + q_qual_off[q] : nullptr; };
    result_wait(r);
    const size_t n = r->alns.size();
    // --- 1. binary records (one per alignment + one per unmapped read), built in parallel over queries
    std::vector<size_t> qfirst((size_t)n_queries + 1, 0);
    { size_t i = 0; for (int q = 0; q < n_queries; ++q) { qfirst[q] = i; while (i < n && r->alns[i].qid == q) ++i; } qfirst[n_queries] = i; }
    std::vector<int> q_unmapped;
    for (int q = 0; q < n_queries; ++q) if (qfirst[q] == qfirst[q + 1] && !(flags & TELR_SAM_NO_UNMAPPED)) q_unmapped.push_back(q);
    const size_t nrec = n + q_unmapped.size();
    std::vector<std::string> recs(nrec);
    std::vector<int64_t> key(nrec);
    const int NT = host_threads();
    parallel_ranges(NT, n_queries, [&](int, int qa, int qb) {
        std::string rc, md, cs, sa, tagbuf;
        std::vector<uint32_t> bc;
        for (int q = qa; q < qb; ++q) {
            const size_t i0 = qfirst[q], i1 = qfirst[q + 1];
            if (i0 == i1) continue;
            const char *qs = q_ascii + q_off[q]; const int ql = q_len[q];
            revcomp_into(qs, ql, rc);
            for (size_t k = i0; k < i1; ++k) {
                const telr_aln &a = r->alns[k];
                const RecLayout L = rec_layout(a, ql, flags);
                const char *qstr = L.rev ? rc.data() : qs;
                const uint32_t *cg = r->cig + a.cigar_off;
                md.clear(); cs.clear();
                const int nm = aln_walk(qstr, t_ascii + t_off[a.tid], cg, a.n_cigar, L.clip5, a.ts, flags, md, cs);
                bc.clear();
                if (L.clip5 > 0) bc.push_back((uint32_t)L.clip5 << 4 | (L.hard ? 5u : 4u));
                bc.insert(bc.end(), cg, cg + a.n_cigar);          // M=0 I=1 D=2 as in BAM
                if (L.clip3 > 0) bc.push_back((uint32_t)L.clip3 << 4 | (L.hard ? 5u : 4u));
                const bool long_cigar = bc.size() > 65535;
                tagbuf.clear();
                auto tag_i = [&](const char *t, int32_t v) { tagbuf += t; tagbuf += 'i'; tagbuf.append((const char*)&v, 4); };
                auto tag_z = [&](const char *t, const std::string &v) { tagbuf += t; tagbuf += 'Z'; tagbuf += v; tagbuf += '\0'; };
                tag_i("NM", nm); tag_i("AS", a.dp_score);
                if (flags & TELR_SAM_MD) tag_z("MD", md);
                if (flags & TELR_SAM_CS) tag_z("cs", cs);
                if (!L.sec) {
                    sa.clear();
                    sa_text(&r->alns[i0], i1 - i0, k - i0, ql, r->cig, tnames, sa);
                    if (!sa.empty()) tag_z("SA", sa);
                }
                tagbuf += "tpA"; tagbuf += L.sec ? 'S' : 'P';
                tag_i("cm", a.cnt); tag_i("s1", a.score);
                if (!L.sec) tag_i("s2", a.subsc);
                if (rg_id) tag_z("RG", rg_id);
                // -L: more than 65,535 operations go into a CG:B,I tag, the placeholder <l_seq>S<ref_len>N into the record
                const uint32_t placeholder[2] = { (uint32_t)L.l_seq << 4 | 4u, (uint32_t)(a.te - a.ts) << 4 | 3u };
                if (long_cigar) { tagbuf += "CGBI"; put32(tagbuf, (uint32_t)bc.size()); tagbuf.append((const char*)bc.data(), bc.size() * 4); }
                std::string &o = recs[k];
                const uint32_t n_cig = long_cigar ? 2u : (uint32_t)bc.size();
                o.reserve(36 + strlen(qnames[q]) + 1 + n_cig * 4 + (L.l_seq + 1) / 2 + L.l_seq + tagbuf.size());
                bam_rec_open(o, a.tid, a.ts, a.mapq, reg2bin(a.ts, a.te > a.ts ? a.te : a.ts + 1), L.flag, qnames[q], long_cigar ? placeholder : bc.data(), n_cig,
                             qstr, L.seq_lo, L.l_seq, qual_of(q), phred_offset, L.rev, ql);
                o += tagbuf;
                bam_rec_close(o);
                key[k] = L.key;
            }
        }
    });
    for (size_t u = 0; u < q_unmapped.size(); ++u) {
        const int q = q_unmapped[u];
        std::string &o = recs[n + u];
        bam_rec_open(o, -1, -1, 0, 4680, 4, qnames[q], nullptr, 0, q_ascii + q_off[q], 0, q_len[q], qual_of(q), phred_offset, false, q_len[q]);
        if (rg_id) { o += "RGZ"; o += rg_id; o += '\0'; }
        bam_rec_close(o);
        key[n + u] = SAM_KEY_UNMAPPED;
    }
    // --- 2. coordinate sort (stable)
    std::vector<uint32_t> order(nrec);
    for (size_t i = 0; i < nrec; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    // --- 3. uncompressed stream: header + records, cut into BGZF blocks of <= BAM_BLK bytes
    const std::string head = bam_header(n_targets, tnames, t_len, rg_id, rg_sm, rg_lb, pg_line);
    std::vector<uint64_t> ustart(nrec + 1);        // uncompressed offset of every record (sorted order)
    uint64_t upos = head.size();
    for (size_t i = 0; i < nrec; ++i) { ustart[i] = upos; upos += recs[order[i]].size(); }
    ustart[nrec] = upos;
    const uint64_t utotal = upos;
    std::string ubuf; ubuf.resize(utotal);
    memcpy(&ubuf[0], head.data(), head.size());
    parallel_ranges(NT, (int)nrec, [&](int, int a0, int a1) { for (int i = a0; i < a1; ++i) memcpy(&ubuf[ustart[i]], recs[order[i]].data(), recs[order[i]].size()); });
    const size_t nblk = (size_t)((utotal + BAM_BLK - 1) / BAM_BLK);
    std::vector<std::string> cblk(nblk);
    bool ok = true;
    parallel_ranges(NT, (int)nblk, [&](int, int b0, int b1) {
        for (int b = b0; b < b1; ++b) { size_t o = (size_t)b * BAM_BLK, l = std::min((size_t)BAM_BLK, (size_t)utotal - o); if (!bgzf_block(&ubuf[o], l, level > 0 ? level : 1, cblk[b])) ok = false; }
    });
    if (!ok) return TELR_E_NOMEM;
    std::vector<uint64_t> coff(nblk + 1, 0);
    for (size_t b = 0; b < nblk; ++b) coff[b + 1] = coff[b] + cblk[b].size();
    FILE *f = fopen(bam_path, "wb");
    if (!f) return TELR_E_ARG;
    for (size_t b = 0; b < nblk; ++b) fwrite(cblk[b].data(), 1, cblk[b].size(), f);
    fwrite(BGZF_EOF, 1, sizeof(BGZF_EOF), f);
    fclose(f);
    if (!write_index) return TELR_OK;
    // --- 4. BAI: laid out over the stream's offsets, then moved to the blocks' file offsets (the records are sorted here: always in file order)
    std::string bai; std::vector<size_t> fix;
    (void)bai_build(n, [&](size_t i) { const telr_aln &a = r->alns[order[i]]; return BaiEntry{ a.tid, a.ts, a.te, ustart[i], ustart[i + 1] }; },
                    [](uint64_t u) { return u / BAM_BLK; }, q_unmapped.size(), n_targets, t_len, bai, &fix);
    bai_finish(bai, fix, coff.data(), nblk);
    const std::string bai_path = std::string(bam_path) + ".bai";
    f = fopen(bai_path.c_str(), "wb");
    if (!f) return TELR_E_ARG;
    fwrite(bai.data(), 1, bai.size(), f);
    fclose(f);
    return TELR_OK;
}
extern "C" int telr_write_bam(const telr_result *r, int32_t n_queries, const char *const *qnames, const char *q_ascii, const int64_t *q_off,
                              const int32_t *q_len, int32_t n_targets, const char *const *tnames, const char *t_ascii, const int64_t *t_off,
                              const int32_t *t_len, int32_t flags, const char *rg_id, const char *rg_sm, const char *rg_lb,
                              const char *pg_line, const char *bam_path, int32_t write_index, int32_t level)
{
    return telr_write_bam_qual(r, n_queries, qnames, q_ascii, q_off, q_len, n_targets, tnames, t_ascii, t_off, t_len, flags, rg_id, rg_sm, rg_lb, pg_line, bam_path, write_index, level,
                               nullptr, nullptr, 0);
}
