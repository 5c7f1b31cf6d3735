"""A plain encoder of the BAM stream and the .bai the writers (telr_write_bam, telr_write_bam_dev, telr_write_bam_slice) are
documented to produce: numpy / struct only, one alignment column at a time into Python strings.

Written from
  * the SAM specification: the BAM record layout (4.2), reg2bin (5.3), the 4-bit SEQ codes `=ACMGRSVTWYHKDBN` with the first
    base of a pair in the high nibble, the CIGAR op codes MIDNSHP=X, the placeholder `<l_seq>S<ref_len>N` + CG:B,I for more
    than 65,535 operations, the .bai layout (5.2: bins -> chunks, pseudo-bin 37450, 16-kb linear index, n_no_coor);
  * the optional-fields document: MD = [0-9]+(([A-Z]|\\^[A-Z]+)[0-9]+)*, NM = edit distance, SA = (rname,pos,strand,CIGAR,mapQ,NM;)+;
  * minimap2's manual: the short cs form (`:n` `*tq` `+seq` `-seq`, lower case), tp:A:P/S, cm, s1, s2; SA CIGARs reduced to
    clip / M / I / D totals; secondaries printed without SEQ;
  * what include/telr_hip.h and the head of bam_dev.hip.h say about THIS writer: tag order NM AS [MD] [cs] [SA] tp cm s1 [s2]
    [RG] [CG], every integer tag of type `i`, QUAL 0xff, sort by refID / position / forward before reverse / input order,
    unmapped reads last in read order, the header text.

Choices of the writers that the specification leaves open, followed here because they are documented:
  * a base that is not A C G T (either case) prints as N: 4-bit code 15 in SEQ, `N` / `n` in MD and cs (telr_hip.h: "Bases
    print as the engine sees them");
  * a column with an N on either side is a mismatch, N against N included (telr_hip.h, n_ambi: "ambiguous columns count as
    mismatches"): it counts in NM and is printed in MD / cs.  samtools calmd would count N against N as a match;
  * a record with te == ts (no reference base) gets the bin and linear window of [ts, ts + 1), as samtools does for a record
    whose CIGAR consumes no reference;
  * the NM of an SA entry is the edit distance of that record (the walk's NM; the writers print blen - mlen, which the record
    rules make the same number);
  * hard clips only on supplementary records without TELR_SAM_SOFTCLIP; a secondary keeps soft clips although its SEQ is `*`.
Not modelled: `U` (the host writer reads it as T, the device as N; no input of the pipeline holds it).

`sam_text` decodes such a stream to the SAM file telr_write_sam prints for the same records (tests/test_gpu_sam_text.py).  The text
writer prints the read's own characters in SEQ where the stream has 4-bit codes: the two agree for reads of A C G T N in upper case.
"""
import struct
from collections import namedtuple

import numpy as np

from telr_amd._abi import ALN_DTYPE, F_PRIMARY, F_SECONDARY, F_SUPPL, F_REV  # noqa: F401

SAM_MD, SAM_CS, SAM_SOFTCLIP, SAM_NO_UNMAPPED = 1, 2, 4, 8          # TELR_SAM_* (include/telr_hip.h)
SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}

Stream = namedtuple("Stream", "raw head_len offsets recs")


def reg2bin(beg, end):
    """SAM specification 5.3: the bin of the zero-based half-open interval [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def norm(s):
    """the bases as the writers print them: upper case, anything but A C G T is N"""
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def seq4(s):
    """4-bit SEQ of a printed sequence: two bases per byte, the first in the high nibble, an odd tail padded with 0"""
    out = bytearray()
    for i in range(0, len(s), 2):
        hi = SEQ_CODES.index(s[i])
        lo = SEQ_CODES.index(s[i + 1]) if i + 1 < len(s) else 0
        out.append(hi << 4 | lo)
    return bytes(out)


def columns(q, t, cigar):
    """the alignment as a list of columns (op, query base or None, target base or None); q and t start at the first aligned base"""
    cols, qi, ti = [], 0, 0
    for c in cigar:
        op, n = int(c) & 15, int(c) >> 4
        for _ in range(n):
            if op == 0:
                cols.append(("M", q[qi], t[ti])); qi += 1; ti += 1
            elif op == 1:
                cols.append(("I", q[qi], None)); qi += 1
            elif op == 2:
                cols.append(("D", None, t[ti])); ti += 1
            else:
                raise ValueError("CIGAR op %d" % op)
        cols.append(("|", None, None))          # op boundary: two D ops (or two I ops) with nothing between stay two events
    return cols, qi, ti


def is_match(qc, tc):
    return qc == tc and qc != "N"


def walk_tags(cols):
    """(NM, MD, cs, matches, inserted, deleted) of a column list"""
    nm = matches = n_ins = n_del = 0
    md, run, in_del = "", 0, False
    cs, csrun, in_ins, in_csdel = "", 0, False, False
    for op, qc, tc in cols:
        if op == "M" and is_match(qc, tc):
            run += 1; csrun += 1; matches += 1
            in_del = in_ins = in_csdel = False
            continue
        if csrun:
            cs += ":%d" % csrun; csrun = 0
        if op == "|":
            in_del = in_ins = in_csdel = False
        elif op == "M":
            nm += 1
            md += "%d%s" % (run, tc); run = 0
            cs += "*" + tc.lower() + qc.lower()
            in_del = in_ins = in_csdel = False
        elif op == "I":
            nm += 1; n_ins += 1
            if not in_ins:
                cs += "+"
            cs += qc.lower(); in_ins = True; in_del = in_csdel = False
        else:
            nm += 1; n_del += 1
            if not in_del:
                md += "%d^" % run; run = 0
            md += tc; in_del = True
            if not in_csdel:
                cs += "-"
            cs += tc.lower(); in_csdel = True; in_ins = False
    md += "%d" % run
    return nm, md, cs, matches, n_ins, n_del


def _i(tag, v):
    return tag.encode() + b"i" + struct.pack("<i", int(v))


def _z(tag, s):
    return tag.encode() + b"Z" + s.encode() + b"\0"


def header(tnames, tlens, rg, cmdline):
    text = "@HD\tVN:1.6\tSO:coordinate\n"
    for n, l in zip(tnames, tlens):
        text += "@SQ\tSN:%s\tLN:%d\n" % (n, l)
    if rg:
        text += "@RG\tID:%s\tSM:%s\tLB:%s\n" % tuple(rg)
    text += "@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:%s\n" % cmdline
    h = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(tnames))
    for n, l in zip(tnames, tlens):
        h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return h


def describe(alns, cigars, reads, targets):
    """per input record: what the tags and the SA entries of its read need (the column walk happens here, once)"""
    out = []
    for a in alns:
        read = norm(reads[int(a["qid"])])
        rev = bool(a["flags"] & F_REV)
        qlen = len(read)
        printed = revcomp(read) if rev else read
        clip5 = qlen - int(a["qe"]) if rev else int(a["qs"])
        clip3 = int(a["qs"]) if rev else qlen - int(a["qe"])
        cg = cigars[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]
        t = norm(targets[int(a["tid"])][int(a["ts"]):int(a["te"])])
        cols, qn, tn = columns(printed[clip5:qlen - clip3], t, cg)
        assert qn == qlen - clip5 - clip3 and tn == len(t), "CIGAR does not span the record's intervals"
        nm, md, cs, matches, n_ins, n_del = walk_tags(cols)
        out.append(dict(printed=printed, rev=rev, clip5=clip5, clip3=clip3, cg=[int(c) for c in cg], nm=nm, md=md, cs=cs, matches=matches,
                        n_ins=n_ins, n_del=n_del, sec=bool(a["flags"] & F_SECONDARY), sup=bool(a["flags"] & F_SUPPL)))
    return out


def sa_entry(a, d, tnames):
    s = "%s,%d,%s," % (tnames[int(a["tid"])], int(a["ts"]) + 1, "-" if d["rev"] else "+")
    if d["clip5"]:
        s += "%dS" % d["clip5"]
    s += "%dM" % (int(a["qe"]) - int(a["qs"]) - d["n_ins"])
    if d["n_ins"]:
        s += "%dI" % d["n_ins"]
    if d["n_del"]:
        s += "%dD" % d["n_del"]
    if d["clip3"]:
        s += "%dS" % d["clip3"]
    return s + ",%d,%d;" % (int(a["mapq"]), d["nm"])


def bam_stream(alns, cigars, reads, targets, qnames, tnames, flags, rg=None, cmdline="telr_map"):
    """-> Stream(raw = the uncompressed BAM bytes, head_len, offsets = start of every record in file order, recs = one dict per
    record in file order: off, size, idx (input record, None for an unmapped read), qid, tid, pos, end, bin, flag, the tag
    strings and the absolute offsets of the record's fields)"""
    alns = np.asarray(alns, dtype=ALN_DTYPE)
    desc = describe(alns, cigars, reads, targets)
    rg_id = rg[0] if rg else None
    built = []
    for k, (a, d) in enumerate(zip(alns, desc)):
        qid = int(a["qid"])
        hard = d["sup"] and not flags & SAM_SOFTCLIP
        clipop = 5 if hard else 4
        ops = ([d["clip5"] << 4 | clipop] if d["clip5"] else []) + d["cg"] + ([d["clip3"] << 4 | clipop] if d["clip3"] else [])
        if d["sec"]:
            seq = ""
        elif hard:
            seq = d["printed"][d["clip5"]:len(d["printed"]) - d["clip3"]]
        else:
            seq = d["printed"]
        ts, te = int(a["ts"]), int(a["te"])
        tags = _i("NM", d["nm"]) + _i("AS", a["dp_score"])
        if flags & SAM_MD:
            tags += _z("MD", d["md"])
        if flags & SAM_CS:
            tags += _z("cs", d["cs"])
        sa = ""
        if not d["sec"]:
            for k2, (b, e) in enumerate(zip(alns, desc)):
                if k2 != k and int(b["qid"]) == qid and not e["sec"]:
                    sa += sa_entry(b, e, tnames)
            if sa:
                tags += _z("SA", sa)
        tags += b"tpA" + (b"S" if d["sec"] else b"P") + _i("cm", a["cnt"]) + _i("s1", a["score"])
        if not d["sec"]:
            tags += _i("s2", a["subsc"])
        if rg_id:
            tags += _z("RG", rg_id)
        rec_ops = ops
        if len(ops) > 65535:
            rec_ops = [len(seq) << 4 | 4, (te - ts) << 4 | 3]
            tags += b"CGBI" + struct.pack("<I", len(ops)) + struct.pack("<%dI" % len(ops), *ops)
        name = qnames[qid].encode() + b"\0"
        assert len(name) <= 255
        flag = (0x10 if d["rev"] else 0) | (0x100 if d["sec"] else 0) | (0x800 if d["sup"] else 0)
        bn = reg2bin(ts, te if te > ts else ts + 1)
        body = struct.pack("<iiBBHHHiiii", int(a["tid"]), ts, len(name), int(a["mapq"]) & 255, bn, len(rec_ops), flag, len(seq), -1, -1, 0)
        body += name + struct.pack("<%dI" % len(rec_ops), *rec_ops) + seq4(seq) + b"\xff" * len(seq) + tags
        built.append(((int(a["tid"]), ts, 1 if d["rev"] else 0, k), body,
                      dict(idx=k, qid=qid, tid=int(a["tid"]), pos=ts, end=te, bin=bn, flag=flag, nm=d["nm"], md=d["md"], cs=d["cs"], sa=sa,
                           l_name=len(name), n_cig=len(rec_ops), n_ops=len(ops), l_seq=len(seq), l_tags=len(tags))))
    built.sort(key=lambda x: x[0])
    if not flags & SAM_NO_UNMAPPED:
        have = set(int(q) for q in alns["qid"])
        for q in range(len(reads)):
            if q in have:
                continue
            seq = norm(reads[q])
            name = qnames[q].encode() + b"\0"
            tags = _z("RG", rg_id) if rg_id else b""
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, reg2bin(-1, 0), 0, 4, len(seq), -1, -1, 0)
            body += name + seq4(seq) + b"\xff" * len(seq) + tags
            built.append((None, body, dict(idx=None, qid=q, tid=-1, pos=-1, end=-1, bin=4680, flag=4, nm=None, md=None, cs=None, sa="",
                                           l_name=len(name), n_cig=0, n_ops=0, l_seq=len(seq), l_tags=len(tags))))
    head = header(tnames, [len(t) for t in targets], rg, cmdline)
    parts, offsets, recs, p = [head], [], [], len(head)
    for _, body, info in built:
        info["off"] = p; info["size"] = 4 + len(body)
        info["p_cig"] = p + 36 + info["l_name"]
        info["p_seq"] = info["p_cig"] + 4 * info["n_cig"]
        info["p_qual"] = info["p_seq"] + (info["l_seq"] + 1) // 2
        info["p_tags"] = info["p_qual"] + info["l_seq"]
        offsets.append(p); recs.append(info)
        parts.append(struct.pack("<i", len(body))); parts.append(body)
        p += 4 + len(body)
    return Stream(b"".join(parts), len(head), offsets, recs)


def bai_reference(stream, tlens):
    """the .bai of the stream in UNCOMPRESSED offsets: {"refs": [{"bins": {bin: [(beg, end) of every record, file order]},
    "linear": [...], "meta": (beg, end, n_mapped, 0) or None}], "n_no_coor": n}.  The linear index holds, for every 16-kb
    window up to the last one a record touches, the smallest offset of a record overlapping it; an untouched window repeats the
    window before it (samtools), 0 before the first."""
    refs = [dict(bins={}, linear=[], meta=None) for _ in tlens]
    n_no_coor = 0
    for r in stream.recs:
        if r["tid"] < 0:
            n_no_coor += 1
            continue
        R = refs[r["tid"]]
        beg, end = r["off"], r["off"] + r["size"]
        R["bins"].setdefault(r["bin"], []).append((beg, end))
        e = r["end"] if r["end"] > r["pos"] else r["pos"] + 1
        lin = R["linear"]
        for w in range(r["pos"] >> 14, ((e - 1) >> 14) + 1):
            while len(lin) <= w:
                lin.append(None)
            if lin[w] is None or beg < lin[w]:
                lin[w] = beg
        m = R["meta"]
        R["meta"] = (beg if m is None else m[0], end, (0 if m is None else m[2]) + 1, 0)
    for R in refs:
        prev = 0
        for w, v in enumerate(R["linear"]):
            if v is None:
                R["linear"][w] = prev
            prev = R["linear"][w]
    return dict(refs=refs, n_no_coor=n_no_coor)


# ---- the stream as SAM text ----------------------------------------------------------------------------------------------
def sam_records(stream):
    """the SAM lines (no newline) of the stream's records, in the stream's order.  Columns from the record's fixed part; tags
    in the record's order (`i` -> :i:, `A` -> :A:, `Z` -> :Z:); SEQ `*` when l_seq is 0, QUAL `*` when it is 0 or the bytes are
    0xff; a CG:B,I tag becomes the CIGAR column and is not printed (the text has no 65,535-operation limit)."""
    raw = stream.raw
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    tnames = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, p)[0]
        tnames.append(raw[p + 4:p + 4 + ln - 1].decode()); p += 8 + ln
    assert p == stream.head_len
    lines = []
    for r in stream.recs:
        o = r["off"]
        bs, refid, pos, lrn, mapq, _bin, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", raw, o)
        name = raw[o + 36:o + 36 + lrn - 1].decode()
        ops = list(struct.unpack_from("<%dI" % ncig, raw, r["p_cig"]))
        seq = "".join(SEQ_CODES[raw[r["p_seq"] + (x >> 1)] >> (0 if x & 1 else 4) & 15] for x in range(lseq))
        qual = raw[r["p_qual"]:r["p_qual"] + lseq]
        tags, t, e = [], r["p_tags"], o + 4 + bs
        while t < e:
            tag, ty = raw[t:t + 2].decode(), chr(raw[t + 2]); t += 3
            if ty == "i":
                tags.append("%s:i:%d" % (tag, struct.unpack_from("<i", raw, t)[0])); t += 4
            elif ty == "A":
                tags.append("%s:A:%s" % (tag, chr(raw[t]))); t += 1
            elif ty == "Z":
                z = raw.index(b"\0", t); tags.append("%s:Z:%s" % (tag, raw[t:z].decode())); t = z + 1
            else:
                assert (tag, ty, chr(raw[t])) == ("CG", "B", "I"), (tag, ty)
                n = struct.unpack_from("<I", raw, t + 1)[0]
                ops = list(struct.unpack_from("<%dI" % n, raw, t + 5)); t += 5 + 4 * n
        assert t == e
        cols = [name, "%d" % flag, tnames[refid] if refid >= 0 else "*", "%d" % (pos + 1), "%d" % mapq,
                "".join("%d%s" % (c >> 4, CIGAR_OPS[c & 15]) for c in ops) or "*",
                "*" if nref < 0 else "=" if nref == refid else tnames[nref], "%d" % (npos + 1), "%d" % tlen,
                seq or "*", "*" if not lseq or qual == b"\xff" * lseq else bytes(b + 33 for b in qual).decode()]
        lines.append("\t".join(cols + tags))
    return lines


def sam_text(stream, coordinate_sorted=True, keep=None):
    """the SAM file telr_write_sam prints for the stream's records: the stream's own header text and one line per record.
    coordinate_sorted: the stream's order.  Otherwise @HD says SO:unsorted GO:query and the lines stand in (read, rank) order,
    which is the input order of the records, an unmapped read at its read's place.  keep(flag) -> bool drops lines."""
    text = stream.raw[8:8 + struct.unpack_from("<i", stream.raw, 4)[0]].decode()
    lines = list(zip(stream.recs, sam_records(stream)))
    if not coordinate_sorted:
        hd = "@HD\tVN:1.6\tSO:coordinate\n"
        assert text.startswith(hd)
        text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + text[len(hd):]
        lines.sort(key=lambda x: (x[0]["qid"], x[0]["idx"] if x[0]["idx"] is not None else -1))
    return text + "".join(l + "\n" for r, l in lines if keep is None or keep(r["flag"]))


# ---- reading files back (zlib + struct) ---------------------------------------------------------------------------------
def parse_bai(bai):
    """-> {"refs": [{"bins": {bin: [(vbeg, vend)]}, "linear": [...], "meta": (..) or None}], "n_no_coor"} in VIRTUAL offsets"""
    assert bai[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    q, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, q)[0]; q += 4
        bins, meta, last = {}, None, -1
        for _ in range(n_bin):
            b, nch = struct.unpack_from("<Ii", bai, q); q += 8
            ch = [struct.unpack_from("<QQ", bai, q + 16 * c) for c in range(nch)]; q += 16 * nch
            if b == 37450:
                assert nch == 2 and meta is None
                meta = ch[0] + ch[1]
            else:
                assert b not in bins and b < 37449
                bins[b] = ch
        n_intv = struct.unpack_from("<i", bai, q)[0]; q += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, bai, q)); q += 8 * n_intv
        refs.append(dict(bins=bins, linear=lin, meta=meta))
    n_no_coor = struct.unpack_from("<Q", bai, q)[0]; q += 8
    assert q == len(bai)
    return dict(refs=refs, n_no_coor=n_no_coor)


def compare_bai(bai, blocks, ref_index):
    """the parsed .bai of a file against the reference index; blocks = [(file offset, uncompressed start, length)] of the file.
    Virtual offsets are translated through the file's own block table.  Rule for chunks: the specification lets a writer
    merge neighbouring chunks of a bin; samtools merges two when the first ends in the BGZF block the second starts in.  So
    a bin's chunk list must be the reference's per-record list in which a neighbouring pair MAY be joined only under that
    condition -- every record of the bin covered, chunks beginning and ending at records of the bin, in file order."""
    by_off = {b[0]: b for b in blocks}

    def u_of(v):
        b = by_off[v >> 16]
        assert (v & 0xffff) <= b[2], "offset beyond its block"
        return b[1] + (v & 0xffff)

    def blk_of(u):
        k = max(i for i, b in enumerate(blocks) if b[1] <= u)
        return k
    got = parse_bai(bai)
    assert got["n_no_coor"] == ref_index["n_no_coor"], ("n_no_coor", got["n_no_coor"], ref_index["n_no_coor"])
    assert len(got["refs"]) == len(ref_index["refs"])
    for t, (G, R) in enumerate(zip(got["refs"], ref_index["refs"])):
        assert sorted(G["bins"]) == sorted(R["bins"]), ("bins of reference %d" % t, sorted(G["bins"]), sorted(R["bins"]))
        for b, want in R["bins"].items():
            have = [(u_of(x), u_of(y)) for x, y in G["bins"][b]]
            i = 0
            for beg, end in have:
                assert i < len(want) and want[i][0] == beg, ("chunk of bin %d does not begin at its next record" % b, t, beg, want[i:i + 2])
                while want[i][1] != end:
                    assert i + 1 < len(want) and want[i][1] < end, ("chunk of bin %d does not end at a record of the bin" % b, t, end)
                    assert blk_of(want[i][1]) == blk_of(want[i + 1][0]) or want[i][1] == want[i + 1][0], ("chunks merged across BGZF blocks", t, b)
                    i += 1
                i += 1
            assert i == len(want), ("records of bin %d not covered" % b, t, len(want) - i)
        if R["meta"] is None:
            assert G["meta"] is None
        else:
            assert G["meta"] is not None, "no pseudo-bin for reference %d" % t
            assert (u_of(G["meta"][0]), u_of(G["meta"][1])) + tuple(G["meta"][2:]) == R["meta"], ("pseudo-bin", t, G["meta"], R["meta"])
        assert [u_of(v) for v in G["linear"]] == R["linear"], ("linear index of reference %d" % t, [u_of(v) for v in G["linear"]][:8], R["linear"][:8])


def parse_records(raw):
    """the records of an inflated BAM stream: [(offset, refid, pos, bin, mapq, flag, name, cigar ops, l_seq, seq bytes, tag bytes)]"""
    assert raw[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    out = []
    while p < len(raw):
        bs, refid, pos, lrn, mapq, bn, ncig, flag, lseq = struct.unpack_from("<iiiBBHHHi", raw, p)
        q = p + 36
        name = raw[q:q + lrn - 1].decode(); q += lrn
        cig = struct.unpack_from("<%dI" % ncig, raw, q); q += 4 * ncig
        seq = raw[q:q + (lseq + 1) // 2]; q += (lseq + 1) // 2 + lseq
        out.append((p, refid, pos, bn, mapq, flag, name, cig, lseq, seq, raw[q:p + 4 + bs]))
        p += 4 + bs
    assert p == len(raw)
    return out


def read_bgzf(path):
    """every BGZF block of a file inflated with zlib, its CRC-32 and ISIZE checked, its sizes held to the format's limits
    (BSIZE + 1 <= 65,536, ISIZE <= 65,280 as the writers cut the stream) -> (stream, [(file offset, uncompressed start, length,
    BTYPE of the first deflate block)]); the last block is the 28-byte EOF marker"""
    import zlib
    data = open(path, "rb").read()
    out, off, u, blocks = [], 0, 0, []
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04" and off + 18 <= len(data), ("not a BGZF block", off)
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        assert xlen == 6 and data[off + 12:off + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, off + 16)[0] + 1
        assert bsize <= 65536 and off + bsize <= len(data)
        raw = zlib.decompress(data[off + 18:off + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, off + bsize - 8)
        assert isize == len(raw) and crc == zlib.crc32(raw), ("CRC / ISIZE of the block at", off)
        assert isize <= 65280
        blocks.append((off, u, len(raw), data[off + 18] >> 1 & 3))
        out.append(raw); off += bsize; u += len(raw)
    assert blocks and blocks[-1][2] == 0 and data[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"), "no EOF block"
    assert all(b[2] > 0 for b in blocks[:-1]), "an empty block inside the file"
    return b"".join(out), blocks
