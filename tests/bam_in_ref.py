"""What telr_bam_load is documented to compute (include/telr_hip.h), stated in plain Python: struct / numpy only.

  * hop / inflate_member / load: the definition -- BGZF framing, a bit-by-bit RFC 1951 inflater that also reports what a stream
    exercises, the BAM header and records, the CIGAR rules, the reads (`bam2fasta`: `samtools fasta` + first-name-wins,
    TELR_input.py:329-361) and the result records;
  * fixed_deflate: a fixed-Huffman deflate writer for hand-chosen (literal | (length, distance)) sequences -- zlib never emits
    a distance above 32,506;
  * member / bgzf / bam_header / bam_record: a BGZF / BAM writer for "foreign" files (not this project's writer);
  * deflate_cases / record_cases / error_cases: the inputs of tests/test_bam_in_ref.py and tests/test_gpu_bam_in.py.

Choices the specification leaves open, documented in the header and followed here:
  * an incomplete code-length set is accepted, bits that are no code of it are an error (zlib refuses most incomplete sets);
    an over-subscribed set, more than 286 / 30 symbols, or no end-of-block code is an error;
  * bytes between the end of the deflate stream and the trailer are ignored;
  * the last occurrence of a tag wins; an integer tag is truncated to 32 bits;
  * errors are reported in the order framing (whole file), inflate (lowest block), header, record chain, records (lowest record).
"""
import struct
import zlib

import numpy as np

from telr_amd._abi import ALN_DTYPE, F_PRIMARY, F_SECONDARY, F_SUPPL, F_REV

E_ARG, E_RANGE, E_NOMEM, E_IO = -3, -4, -5, -6
# inflate status codes (telr_amd/csrc/inflate_core.h)
I_OK, I_INPUT, I_BTYPE, I_STORED, I_CODELEN, I_SYMBOL, I_DIST, I_LONG, I_SHORT, I_CRC = range(10)
I_TEXT = ["ok", "the deflate stream reads past its member", "deflate block type 3", "stored block: LEN / NLEN disagree",
          "invalid code-length set", "invalid code or symbol", "distance before the member's start", "more output than ISIZE",
          "less output than ISIZE", "CRC-32 mismatch"]
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
COUNTERS = ("members", "records", "mapped", "kept", "reads", "orphans", "len_mismatch", "no_cigar", "no_eof")


class BamInError(Exception):
    def __init__(self, code, text):
        Exception.__init__(self, "%d: %s" % (code, text))
        self.code, self.text = code, text


class InflateError(Exception):
    def __init__(self, status):
        Exception.__init__(self, I_TEXT[status])
        self.status = status


# ---- deflate ------------------------------------------------------------------------------------------------------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def _code_table(lens):
    """canonical code of a length list -> {(length, code value): symbol}; raises on an over-subscribed set"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            raise InflateError(I_CODELEN)
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    tab = {}
    for s, l in enumerate(lens):
        if l:
            tab[(l, nxt[l])] = s
            nxt[l] += 1
    return tab


def inflate_member(data, isize=None):
    """raw deflate bytes -> (output, facts).  With isize the output is held to it as the device decoder holds it.  facts: btypes
    (set), blocks, max_code (longest literal/length or distance code of any table), max_dist, max_len, overlap (a match with
    distance < length), dist_codes (a block whose table has a distance code), end_match (the last token is a match)"""
    nbits = len(data) * 8
    pos = 0
    out = bytearray()
    facts = dict(btypes=set(), blocks=0, max_code=0, max_dist=0, max_len=0, overlap=False, dist_codes=False, end_match=False)

    def take(k):
        nonlocal pos
        if pos + k > nbits:
            raise InflateError(I_INPUT)
        v = 0
        for i in range(k):
            v |= (data[(pos + i) >> 3] >> ((pos + i) & 7) & 1) << i
        pos += k
        return v

    def symbol(tab):
        nonlocal pos
        code = 0
        for l in range(1, 16):
            if pos + l > nbits:
                # (the decoder peeks zeros behind the input: a code completed by them is "past the member")
                bit = 0
            else:
                bit = data[(pos + l - 1) >> 3] >> ((pos + l - 1) & 7) & 1
            code = code << 1 | bit
            if (l, code) in tab:
                if pos + l > nbits:
                    raise InflateError(I_INPUT)
                pos += l
                return tab[(l, code)]
        raise InflateError(I_INPUT if nbits - pos < 15 else I_SYMBOL)

    def room(n):
        if isize is not None and len(out) + n > isize:
            raise InflateError(I_LONG)

    while True:
        last = take(1)
        btype = take(2)
        if btype == 3:
            raise InflateError(I_BTYPE)
        facts["btypes"].add(btype); facts["blocks"] += 1
        if btype == 0:
            pos = (pos + 7) & ~7
            ln, nl = take(16), take(16)
            if ln ^ 0xffff != nl:
                raise InflateError(I_STORED)
            if (pos >> 3) + ln > len(data):
                raise InflateError(I_INPUT)
            room(ln)
            out += data[pos >> 3:(pos >> 3) + ln]
            pos += 8 * ln
            facts["end_match"] = False
        else:
            if btype == 1:
                ll, dl = _FIXED_LENS, [5] * 30
            else:
                hl, hd, hc = take(5) + 257, take(5) + 1, take(4) + 4
                if hl > 286 or hd > 30:
                    raise InflateError(I_CODELEN)
                cl = [0] * 19
                for i in range(hc):
                    cl[_ORDER[i]] = take(3)
                ctab = _code_table(cl)
                lens = []
                while len(lens) < hl + hd:
                    s = symbol(ctab)
                    if s < 16:
                        lens.append(s); continue
                    if s == 16:
                        if not lens:
                            raise InflateError(I_CODELEN)
                        prev, rep = lens[-1], 3 + take(2)
                    elif s == 17:
                        prev, rep = 0, 3 + take(3)
                    else:
                        prev, rep = 0, 11 + take(7)
                    if len(lens) + rep > hl + hd:
                        raise InflateError(I_CODELEN)
                    lens += [prev] * rep
                if lens[256] == 0:
                    raise InflateError(I_CODELEN)
                ll, dl = lens[:hl], lens[hl:]
            ltab, dtab = _code_table(ll), _code_table(dl)
            facts["max_code"] = max([facts["max_code"]] + list(ll) + list(dl))
            facts["dist_codes"] = facts["dist_codes"] or any(dl)
            while True:
                s = symbol(ltab)
                if s < 256:
                    room(1)
                    out.append(s); facts["end_match"] = False
                    continue
                if s == 256:
                    break
                if s - 257 >= 29:
                    raise InflateError(I_SYMBOL)
                ln = _LEN_BASE[s - 257] + take(_LEN_EXTRA[s - 257])
                d = symbol(dtab)
                if d >= 30:
                    raise InflateError(I_SYMBOL)
                dist = _DIST_BASE[d] + take(_DIST_EXTRA[d])
                if dist > len(out):
                    raise InflateError(I_DIST)
                room(ln)
                for _ in range(ln):
                    out.append(out[-dist])
                facts["max_dist"] = max(facts["max_dist"], dist); facts["max_len"] = max(facts["max_len"], ln)
                facts["overlap"] = facts["overlap"] or dist < ln
                facts["end_match"] = True
        if last:
            break
    if isize is not None and len(out) != isize:
        raise InflateError(I_SHORT)
    return bytes(out), facts


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, k):
        """k bits of v, least significant first (header fields, extra bits)"""
        self.acc |= v << self.n; self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, c, l):
        """a Huffman code: most significant bit first"""
        for b in range(l - 1, -1, -1):
            self.bits(c >> b & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255); self.acc, self.n = 0, 0
        return bytes(self.out)


def _fixed_lit(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xc0 + s - 280, 8)


def fixed_deflate(tokens):
    """one final fixed-Huffman block of tokens: an int is a literal, a (length, distance) pair a match"""
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            ln, dist = t
            ls = max(i for i in range(29) if _LEN_BASE[i] <= ln and (i == 28) == (ln == 258))
            _fixed_lit(w, 257 + ls); w.bits(ln - _LEN_BASE[ls], _LEN_EXTRA[ls])
            ds = max(i for i in range(30) if _DIST_BASE[i] <= dist)
            w.code(ds, 5); w.bits(dist - _DIST_BASE[ds], _DIST_EXTRA[ds])
        else:
            _fixed_lit(w, t)
    _fixed_lit(w, 256)
    return w.done()


def tokens_output(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


# ---- BGZF ---------------------------------------------------------------------------------------------------------------------
def member(comp, raw=None, isize=None, crc=None, extra=b""):
    """a BGZF member around deflate bytes `comp`; extra: subfields placed before BC"""
    isize = len(raw) if isize is None else isize
    crc = zlib.crc32(raw) if crc is None else crc
    xlen = len(extra) + 6
    total = 12 + xlen + len(comp) + 8
    assert total <= 65536
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" + struct.pack("<H", total - 1) + comp + \
        struct.pack("<II", crc, isize)


def deflate_raw(raw, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(raw) + c.flush()


def bgzf(stream, cuts=None, level=6, eof=True, extra=b""):
    """the stream as members cut at `cuts` (ascending offsets; None: 65,280-byte members; a repeated offset = an empty member)"""
    if cuts is None:
        cuts = list(range(65280, len(stream), 65280))
    out, a = b"", 0
    for b in list(cuts) + [len(stream)]:
        out += member(deflate_raw(stream[a:b], level), stream[a:b], extra=extra); a = b
    return out + (EOF_MARKER if eof else b"")


def hop(data):
    """the file's members: [(offset of the deflate bytes, their length, ISIZE, CRC)]; BamInError on a framing defect"""
    out, p, k = [], 0, 0
    while p < len(data):
        def bad(why):
            return BamInError(E_ARG, "block %d: %s" % (k, why))
        if p + 12 > len(data):
            raise bad("truncated member")
        if data[p:p + 4] != b"\x1f\x8b\x08\x04":
            raise bad("not a BGZF member (wrong magic, or bytes after the last member)")
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        if p + 12 + xlen > len(data):
            raise bad("truncated member")
        q, bsize = p + 12, None
        while q + 4 <= p + 12 + xlen:
            slen = struct.unpack_from("<H", data, q + 2)[0]
            if data[q:q + 2] == b"BC" and slen == 2 and q + 6 <= p + 12 + xlen:
                bsize = struct.unpack_from("<H", data, q + 4)[0] + 1
                break
            q += 4 + slen
        if bsize is None:
            raise bad("no BC subfield")
        if bsize < 12 + xlen + 8:
            raise bad("BSIZE smaller than the member's own fields")
        if p + bsize > len(data):
            raise bad("truncated member")
        crc, isize = struct.unpack_from("<II", data, p + bsize - 8)
        if isize > 65536:
            raise bad("ISIZE above 65,536")
        out.append((p + 12 + xlen, bsize - 12 - xlen - 8, isize, crc))
        p += bsize; k += 1
    return out


def inflate_one(comp, isize, crc):
    """one member by the definition -> its bytes; InflateError.  zlib does the work where it agrees that the member is sound (the
    plain inflater above is held to zlib on every deflate case by tests/test_bam_in_ref.py); anything else goes through the plain
    inflater, whose verdict is the definition's"""
    try:
        d = zlib.decompressobj(-15)
        raw = d.decompress(comp)
        if d.eof and len(raw) == isize and zlib.crc32(raw) == crc:
            return raw
    except zlib.error:
        pass
    raw, _ = inflate_member(comp, isize)
    if zlib.crc32(raw) != crc:
        raise InflateError(I_CRC)
    return raw


def inflate_file(data):
    """-> (the inflated stream, number of members, no_eof)"""
    ms = hop(data)
    parts = []
    for k, (off, n, isize, crc) in enumerate(ms):
        try:
            parts.append(inflate_one(data[off:off + n], isize, crc))
        except InflateError as e:
            raise BamInError(E_ARG, "block %d: %s" % (k, I_TEXT[e.status]))
    return b"".join(parts), len(ms), 0 if data[-28:] == EOF_MARKER else 1


# ---- BAM writer ("foreign" files) ---------------------------------------------------------------------------------------------
CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


def ops_of(text):
    """'10M2I' -> [10 << 4 | 0, 2 << 4 | 1]"""
    out, n = [], ""
    for c in text:
        if c.isdigit():
            n += c
        else:
            out.append(int(n) << 4 | CIGAR_OPS.index(c)); n = ""
    return out


def bam_header(tnames, tlens, text="@HD\tVN:1.6\n"):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(tnames))
    for n, l in zip(tnames, tlens):
        h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return h


def bam_record(name, flag, refid=-1, pos=-1, mapq=0, ops=(), seq="", qual=None, tags=b"", codes=None):
    """seq: text over SEQ_CODES (or codes: the 4-bit values themselves); qual: bytes of l_seq Phred values, None = 0xff"""
    codes = [SEQ_CODES.index(c) for c in seq] if codes is None else list(codes)
    n = len(codes)
    packed = bytes((codes[i] << 4 | (codes[i + 1] if i + 1 < n else 0)) for i in range(0, n, 2))
    q = b"\xff" * n if qual is None else bytes(qual)
    assert len(q) == n
    nm = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm), mapq, 4680, len(ops) & 0xffff, flag, n, -1, -1, 0)
    body += nm + struct.pack("<%dI" % len(ops), *ops) + packed + q + tags
    return struct.pack("<i", len(body)) + body


def tag_int(tag, typ, v):
    return tag.encode() + typ.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[typ], v)


def tag_cg(ops):
    return b"CGBI" + struct.pack("<I", len(ops)) + struct.pack("<%dI" % len(ops), *ops)


# ---- the definition -----------------------------------------------------------------------------------------------------------
def normalise(ops):
    """raw CIGAR words -> (clip5, clip3, normalised words, sum M, sum I, sum D); ValueError('clip' | 'op' | 'range')"""
    ops = [int(o) for o in ops]
    i, j, clip5, clip3 = 0, len(ops), 0, 0
    if i < j and ops[i] & 15 == 5:
        clip5 += ops[i] >> 4; i += 1
    if i < j and ops[i] & 15 == 4:
        clip5 += ops[i] >> 4; i += 1
    if j > i and ops[j - 1] & 15 == 5:
        clip3 += ops[j - 1] >> 4; j -= 1
    if j > i and ops[j - 1] & 15 == 4:
        clip3 += ops[j - 1] >> 4; j -= 1
    words, sums = [], [0, 0, 0]
    for o in ops[i:j]:
        op, n = o & 15, o >> 4
        if op > 8:
            raise ValueError("op")
        if op in (4, 5):
            raise ValueError("clip")
        if op == 6 or n == 0:
            continue
        m = {0: 0, 7: 0, 8: 0, 1: 1, 2: 2, 3: 2}[op]
        sums[m] += n
        if words and words[-1][0] == m:
            words[-1][1] += n
        else:
            words.append([m, n])
    if any(n >= 1 << 28 for _, n in words) or sum(sums) + clip5 + clip3 >= 1 << 31:
        raise ValueError("range")
    return clip5, clip3, [n << 4 | m for m, n in words], sums[0], sums[1], sums[2]


def _i32(v):
    return ((int(v) + (1 << 31)) % (1 << 32)) - (1 << 31)


def parse_tags(b):
    """-> ({tag: int} of the integer tags, the CG:B,I array or None); ValueError on a malformed tag area"""
    ints, cg, p = {}, None, 0
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    while p < len(b):
        if p + 3 > len(b):
            raise ValueError("tags")
        tag, typ = b[p:p + 2].decode("latin-1"), chr(b[p + 2]); p += 3
        if typ in sizes:
            if p + sizes[typ] > len(b):
                raise ValueError("tags")
            if typ in fmt:
                ints[tag] = _i32(struct.unpack_from(fmt[typ], b, p)[0])
            p += sizes[typ]
        elif typ in "ZH":
            e = b.find(b"\0", p)
            if e < 0:
                raise ValueError("tags")
            p = e + 1
        elif typ == "B":
            if p + 5 > len(b):
                raise ValueError("tags")
            sub, cnt = chr(b[p]), struct.unpack_from("<I", b, p + 1)[0]
            if sub not in "cCsSiIf":
                raise ValueError("tags")
            if p + 5 + cnt * sizes[sub] > len(b):
                raise ValueError("tags")
            if tag == "CG" and sub == "I":
                cg = list(struct.unpack_from("<%dI" % cnt, b, p + 5))
            p += 5 + cnt * sizes[sub]
        else:
            raise ValueError("tags")
    return ints, cg


def parse_stream(raw):
    """-> (tnames, tlens, [record dict in file order]); BamInError"""
    def need(p, n, what):
        if p + n > len(raw):
            raise BamInError(E_ARG, "header: %s runs past the stream" % what)
    need(0, 12, "magic")
    if raw[:4] != b"BAM\1":
        raise BamInError(E_ARG, "header: no BAM magic")
    l_text = struct.unpack_from("<i", raw, 4)[0]
    if l_text < 0:
        raise BamInError(E_ARG, "header: negative text length")
    need(8, l_text + 4, "text")
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    if n_ref < 0:
        raise BamInError(E_ARG, "header: negative reference count")
    tnames, tlens = [], []
    for _ in range(n_ref):
        need(p, 4, "reference")
        ln = struct.unpack_from("<i", raw, p)[0]
        if ln < 1:
            raise BamInError(E_ARG, "header: reference name length")
        need(p + 4, ln + 4, "reference")
        tnames.append(raw[p + 4:p + 4 + ln - 1].split(b"\0")[0].decode("latin-1")); tlens.append(struct.unpack_from("<i", raw, p + 4 + ln)[0])
        p += 8 + ln
    offs = []
    while p < len(raw):
        k = len(offs)
        if p + 4 > len(raw):
            raise BamInError(E_ARG, "record %d: runs past the stream" % k)
        bs = struct.unpack_from("<i", raw, p)[0]
        if bs < 32:
            raise BamInError(E_ARG, "record %d: block_size below 32" % k)
        if p + 4 + bs > len(raw):
            raise BamInError(E_ARG, "record %d: runs past the stream" % k)
        offs.append(p); p += 4 + bs
    recs = []
    for k, p in enumerate(offs):
        bs, refid, pos, lrn, mapq, _bin, ncig, flag, lseq = struct.unpack_from("<iiiBBHHHi", raw, p)
        end = p + 4 + bs
        if lrn < 1 or lseq < 0 or 36 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq > 4 + bs:
            recs.append(dict(k=k, err=BamInError(E_ARG, "record %d: fields run past the record" % k)))
            continue
        q = p + 36
        name = raw[q:q + lrn - 1].split(b"\0")[0]; q += lrn
        ops = list(struct.unpack_from("<%dI" % ncig, raw, q)); q += 4 * ncig
        seq = raw[q:q + (lseq + 1) // 2]; q += (lseq + 1) // 2
        qual = raw[q:q + lseq]; q += lseq
        try:
            ints, cg = parse_tags(raw[q:end])
        except ValueError:
            recs.append(dict(k=k, err=BamInError(E_ARG, "record %d: malformed tags" % k)))
            continue
        recs.append(dict(k=k, refid=refid, pos=pos, mapq=mapq, flag=flag, lseq=lseq, name=name, ops=ops, seq=seq, qual=qual, ints=ints, cg=cg))
    return tnames, tlens, recs


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def seq_text(seq, lseq, rev):
    s = "".join({1: "A", 2: "C", 4: "G", 8: "T"}.get((seq[i >> 1] >> (0 if i & 1 else 4)) & 15, "N") for i in range(lseq))
    return "".join(_COMP[c] for c in reversed(s)) if rev else s


class Loaded:
    pass


def load(data, keep_qual=False):
    """the whole definition: file bytes -> Loaded(tnames, tlens, qnames, seqs (text), quals (list of bytes, or None), alns
    (ALN_DTYPE), cigars (uint32), counters (dict over COUNTERS)); BamInError"""
    raw, n_members, no_eof = inflate_file(data)
    return load_stream(raw, keep_qual, n_members, no_eof)


def load_stream(raw, keep_qual=False, n_members=0, no_eof=0):
    """the definition behind the framing: the inflated stream -> Loaded"""
    tnames, tlens, recs = parse_stream(raw)
    C = dict.fromkeys(COUNTERS, 0)
    C["members"], C["records"], C["no_eof"] = n_members, len(recs), no_eof
    for r in recs:
        if "err" in r:
            raise r["err"]
        r["mapped"] = not r["flag"] & 4 and r["refid"] >= 0
        r["qlen"] = None
        r["use"] = False
        if not r["mapped"]:
            continue
        C["mapped"] += 1
        k = r["k"]
        if r["refid"] >= len(tnames) or r["pos"] < 0:
            raise BamInError(E_ARG, "record %d: refID or pos outside the header's references" % k)
        ops = r["ops"]
        if len(ops) == 2 and ops[0] == (r["lseq"] << 4 | 4) and ops[1] & 15 == 3 and r["cg"] is not None:
            ops = r["cg"]
        try:
            clip5, clip3, words, sm, si, sd = normalise(ops)
        except ValueError as e:
            if str(e) == "range":
                raise BamInError(E_RANGE, "record %d: CIGAR lengths beyond the record's coordinate bits" % k)
            raise BamInError(E_ARG, "record %d: %s" % (k, "a clip inside the CIGAR" if str(e) == "clip" else "CIGAR op code above 8"))
        if r["pos"] + sm + sd >= 1 << 31:
            raise BamInError(E_RANGE, "record %d: CIGAR lengths beyond the record's coordinate bits" % k)
        r["qlen"] = clip5 + sm + si + clip3
        r.update(clip5=clip5, clip3=clip3, words=words, sm=sm, si=si, sd=sd)
        if not words:
            C["no_cigar"] += 1
        else:
            r["use"] = True
    # the reads
    qid_of, qnames, seqs, quals, any_ff = {}, [], [], [], False
    for r in recs:
        if r["flag"] & 0x900 or r["lseq"] <= 0 or (r["mapped"] and r["lseq"] != r["qlen"]):
            continue
        if r["qual"][0] == 0xff:
            any_ff = True
        if r["name"] in qid_of:
            continue
        rev = bool(r["flag"] & 0x10)
        qid_of[r["name"]] = len(qnames); qnames.append(r["name"].decode("latin-1"))
        seqs.append(seq_text(r["seq"], r["lseq"], rev))
        quals.append(bytes(reversed(r["qual"])) if rev else bytes(r["qual"]))
        r["first"] = True
    with_qual = bool(keep_qual) and not any_ff and len(qnames) > 0
    if with_qual:
        for r in recs:
            if r.get("first") and max(r["qual"]) > 93:
                raise BamInError(E_ARG, "record %d: a base quality above 93" % r["k"])
    C["reads"] = len(qnames)
    kept = []
    for r in recs:
        if not r["use"]:
            continue
        q = qid_of.get(r["name"])
        if q is None:
            C["orphans"] += 1
        elif r["qlen"] != len(seqs[q]):
            C["len_mismatch"] += 1
        else:
            cls = 2 if r["flag"] & 0x100 else 1 if r["flag"] & 0x800 else 0
            kept.append((q, cls, r["k"], r))
    kept.sort(key=lambda x: x[:3])
    C["kept"] = len(kept)
    alns = np.zeros(len(kept), ALN_DTYPE)
    cigars, within, prev_q = [], 0, None
    for i, (q, cls, _, r) in enumerate(kept):
        within = within + 1 if q == prev_q else 0
        prev_q = q
        a = alns[i]
        rev = bool(r["flag"] & 0x10)
        blen = r["sm"] + r["si"] + r["sd"]
        T = r["ints"]
        a["qid"], a["tid"], a["tlen"], a["qlen"] = q, r["refid"], tlens[r["refid"]], r["qlen"]
        a["qs"], a["qe"] = (r["clip3"], r["qlen"] - r["clip5"]) if rev else (r["clip5"], r["qlen"] - r["clip3"])
        a["ts"], a["te"] = r["pos"], r["pos"] + r["sm"] + r["sd"]
        a["blen"] = blen
        a["mlen"] = max(0, _i32(blen - T["NM"])) if "NM" in T else r["sm"]
        a["dp_score"], a["cnt"], a["score"], a["subsc"] = T.get("AS", 0), T.get("cm", 0), T.get("s1", 0), T.get("s2", 0)
        a["mapq"] = r["mapq"]
        a["flags"] = (F_SECONDARY if cls == 2 else F_SUPPL if cls == 1 else F_PRIMARY) | (F_REV if rev else 0)
        a["parent"] = 0 if cls == 2 else within
        a["n_cigar"], a["cigar_off"] = len(r["words"]), len(cigars)
        cigars += r["words"]
    L = Loaded()
    L.tnames, L.tlens, L.qnames, L.seqs = tnames, tlens, qnames, seqs
    L.quals = quals if with_qual else None
    L.alns, L.cigars, L.counters = alns, np.array(cigars, np.uint32), C
    return L


def packed_words(seqs):
    """the set's two word arrays (telr_seqset_packed's layout) from read texts"""
    tot = sum((len(s) + 63) // 64 * 64 for s in seqs)
    w2, wn, b = np.zeros(tot // 16, np.uint32), np.zeros(tot // 32, np.uint32), 0
    for s in seqs:
        for j, c in enumerate(s):
            x = b + j
            if c == "N":
                wn[x >> 5] |= np.uint32(1 << (x & 31))
            else:
                w2[x >> 4] |= np.uint32("ACGT".index(c) << 2 * (x & 15))
        b += (len(s) + 63) // 64 * 64
    return w2, wn


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _text(n, seed=7):
    """BAM-like bytes: 4-letter text with repeats, some binary"""
    rng = np.random.RandomState(seed)
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    for _ in range(n // 600):                                   # copies of earlier pieces: matches at many distances
        a, l = rng.randint(0, max(1, n - 300)), rng.randint(8, 200)
        d = rng.randint(0, max(1, n - 300))
        base[d:d + l] = base[a:a + l][:len(base[d:d + l])]
    return base.tobytes()[:n]


def _fib_bytes(nsym):
    a, b, out = 1, 1, bytearray()
    for s in range(nsym):
        out += bytes([s]) * a
        a, b = b, a + b
    rng = np.random.RandomState(3)
    arr = np.frombuffer(bytes(out), np.uint8).copy(); rng.shuffle(arr)
    return arr.tobytes()


def deflate_cases():
    """[dict(name, raw, comp, claim)]: claim(facts) says which edge the stream reaches"""
    t = _text(65280)
    cs = []

    def add(name, raw, comp, claim):
        assert 12 + 6 + len(comp) + 8 <= 65536, name
        cs.append(dict(name=name, raw=raw, comp=comp, claim=claim))
    add("level0", t, deflate_raw(t, 0), lambda f: f["btypes"] == {0})
    add("fixed", t, deflate_raw(t, 6, 8, zlib.Z_FIXED), lambda f: f["btypes"] == {1} and f["max_dist"] > 0)
    add("default", t, deflate_raw(t), lambda f: 2 in f["btypes"] and f["max_dist"] > 1024)
    add("huffman_only", t, deflate_raw(t, 6, 8, zlib.Z_HUFFMAN_ONLY), lambda f: 2 in f["btypes"] and f["max_len"] == 0)
    rle = bytes(np.repeat(np.frombuffer(_text(8000, 9), np.uint8), np.random.RandomState(5).randint(1, 20, 8000)))[:65280]
    add("rle", rle, deflate_raw(rle, 6, 8, zlib.Z_RLE), lambda f: f["max_dist"] == 1 and f["overlap"])
    add("memlevel1", t, deflate_raw(t, 6, 1), lambda f: f["blocks"] >= 8)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    add("full_flush", t, c.compress(t[:30000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(t[30000:]) + c.flush(), lambda f: 0 in f["btypes"] and 2 in f["btypes"])
    for n in range(16, 30):
        fb = _fib_bytes(n)
        comp = deflate_raw(fb, 6, 8, zlib.Z_HUFFMAN_ONLY)
        if inflate_member(comp)[1]["max_code"] == 15:
            break
    add("fib15", fb, comp, lambda f: f["max_code"] == 15)
    add("out0", b"", deflate_raw(b""), lambda f: True)
    add("out1", b"x", deflate_raw(b"x"), lambda f: True)
    big = _text(65536, 11)
    add("out65536", big, deflate_raw(big), lambda f: True)
    # hand-written streams
    lit = list(_text(32768, 13))
    toks = lit + [(258, 32768)] * 100
    add("dist32768", tokens_output(toks), fixed_deflate(toks), lambda f: f["max_dist"] == 32768)
    toks = [97, (258, 1), 98, (258, 1)]
    add("len258_dist1", tokens_output(toks), fixed_deflate(toks), lambda f: f["max_len"] == 258 and f["max_dist"] == 1 and f["overlap"])
    toks = [1, 2, 3, (3, 3), 4, (3, 2)]
    add("len3", tokens_output(toks), fixed_deflate(toks), lambda f: f["max_len"] == 3)
    toks = list(b"telr") + [(70, 4), 5, (11, 75)]
    add("end_match", tokens_output(toks), fixed_deflate(toks), lambda f: f["end_match"])
    return cs


def _oversubscribed():
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)                                            # nineteen codes of one bit
    w.bits(0, 16)
    return w.done()


def deflate_error_cases():
    """[dict(name, comp, isize, crc, status)]: one member each"""
    t = _text(3000, 17)
    good = deflate_raw(t)
    d = fixed_deflate([1, 2, 3, (3, 5)])
    return [dict(name="wrong_crc", comp=good, isize=len(t), crc=zlib.crc32(t) ^ 1, status=I_CRC),
            dict(name="wrong_isize", comp=good, isize=len(t) + 1, crc=zlib.crc32(t), status=I_SHORT),
            dict(name="isize_small", comp=good, isize=len(t) - 1, crc=zlib.crc32(t), status=I_LONG),
            dict(name="dist_before_start", comp=d, isize=6, crc=0, status=I_DIST),
            dict(name="past_end", comp=good[:-9], isize=len(t), crc=zlib.crc32(t), status=I_INPUT),
            dict(name="oversubscribed", comp=_oversubscribed(), isize=10, crc=0, status=I_CODELEN)]


def write_case_file(path):
    """the deflate cases as tools/ubench/inflate_host.cpp reads them"""
    with open(path, "wb") as f:
        f.write(b"BIC1")
        rows = [(c["name"], I_OK, len(c["raw"]), zlib.crc32(c["raw"]), c["comp"]) for c in deflate_cases()]
        rows += [(c["name"], c["status"], c["isize"], c["crc"], c["comp"]) for c in deflate_error_cases()]
        for name, expect, isize, crc, comp in rows:
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<IIII", expect, isize, crc, len(comp)) + comp)


def _dna(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def record_stream():
    """-> (header bytes, [record bytes]): one foreign BAM that holds every record case of the list in the issue (under 200 records)"""
    rng = np.random.RandomState(21)
    tn, tl = ["chrA", "chrB"], [50000, 7000]
    R = []
    q = lambda n: bytes(rng.randint(0, 60, n).astype(np.uint8))
    alltags = tag_int("NM", "C", 3) + tag_int("AS", "s", -7) + tag_int("cm", "c", 5) + tag_int("s1", "S", 60000) + tag_int("s2", "i", -2) + \
        tag_int("zz", "I", 4000000000) + b"tpAP" + b"MDZ10A5\0" + b"xfB" + b"s" + struct.pack("<Ihh", 2, 1, -1) + b"hxH1AFF\0" + b"fff" + struct.pack("<f", 1.5)
    # read lengths 1, 15, 16, 17, 63, 64, 65: plain forward / reverse matches, QUAL present
    for i, n in enumerate((1, 15, 16, 17, 63, 64, 65)):
        R.append(bam_record("len%d" % n, 0x10 if i & 1 else 0, 0, 100 + 10 * i, 30, ops_of("%dM" % n), _dna(rng, n), q(n), alltags if i == 0 else b""))
    # = X N P ops, H + S clips, zero-length op, adjacent ops that merge
    s = _dna(rng, 5 + 20 + 3 + 10 + 4)
    R.append(bam_record("ops1", 0, 0, 500, 60, ops_of("7H5S10=10X0M3I2P50N10M6D4S9H"), s, q(len(s)), tag_int("NM", "i", 19)))
    R.append(bam_record("ops1r", 0x10, 1, 700, 60, ops_of("3S12M2D2N8M1S"), _dna(rng, 24), q(24)))
    # every 4-bit code, odd l_seq
    R.append(bam_record("codes", 0, 0, 900, 1, ops_of("17M"), codes=list(range(16)) + [1], qual=q(17)))
    R.append(bam_record("codesr", 0x10, 0, 901, 1, ops_of("2S15M"), codes=list(range(15, -1, -1)) + [8], qual=q(17)))
    # a long read: primary + secondary without SEQ + supplementary with hard clips
    s = _dna(rng, 3000)
    R.append(bam_record("long1", 0, 0, 2000, 50, ops_of("100S1400M30I70M1400S"), s, q(3000), tag_int("NM", "i", 40) + tag_int("AS", "i", 2800)))
    R.append(bam_record("long1", 0x100, 1, 10, 0, ops_of("100S1400M30I70M1400S"), "", None, tag_int("s1", "i", 99)))
    R.append(bam_record("long1", 0x800 | 0x10, 0, 9000, 12, ops_of("1600H1000M400H"), _dna(rng, 1000), q(1000)))
    R.append(bam_record("long1", 0x800, 0, 9500, 12, ops_of("1500S100M1400S"), s, q(3000)))
    # an orphan (secondary whose name has no sequence-bearing record), a length mismatch, no M/I/D at all
    R.append(bam_record("orphan", 0x100, 0, 40, 0, ops_of("30M"), "", None))
    R.append(bam_record("long1", 0x100, 0, 60, 0, ops_of("30M"), "", None))
    R.append(bam_record("clips_only", 0, 0, 77, 0, ops_of("12S"), _dna(rng, 12), q(12)))
    # two primaries under one name (the second adds no sequence)
    s = _dna(rng, 40)
    R.append(bam_record("twice", 0, 0, 1200, 20, ops_of("40M"), s, q(40)))
    R.append(bam_record("twice", 0, 1, 1300, 21, ops_of("20M1D20M"), _dna(rng, 40), q(40)))
    # unmapped with and without 0x10
    R.append(bam_record("unm_f", 4, -1, -1, 0, (), _dna(rng, 33) + "N", q(34)))
    R.append(bam_record("unm_r", 4 | 0x10, -1, -1, 0, (), "N" + _dna(rng, 70), q(71)))
    # no tags / more than 65,535 ops through CG
    big = []
    for _ in range(33000):
        big += [1 << 4 | 0, 1 << 4 | 1]
    big += ops_of("5M")
    n = 33000 * 2 + 5
    R.append(bam_record("cg", 0, 0, 3000, 33, [n << 4 | 4, (33000 + 5) << 4 | 3], _dna(rng, n), q(n), tag_int("NM", "i", 33000) + tag_cg(big)))
    # filler: many short records so that members of 1 byte and straddles have something to cut
    for i in range(40):
        n = int(rng.randint(20, 120))
        R.append(bam_record("f%d" % i, 0x10 * (i & 1), i % 2, 100 * i, i, ops_of("%dM" % n), _dna(rng, n), q(n), tag_int("cm", "C", i)))
    return bam_header(tn, tl), R


def record_cases():
    """[dict(name, data, keep_qual)]: whole files"""
    head, R = record_stream()
    body = b"".join(R)
    stream = head + body
    cs = []
    # records straddling one and >= 3 members, members of 1 byte, empty members inside the file, a split header
    p0 = len(head) + sum(len(r) for r in R[:7])
    cuts = [10, 10, len(head) - 3, p0 + 20, p0 + 21, p0 + 22, p0 + 22, p0 + 60]
    big_i = next(i for i, r in enumerate(R) if r[36:39] == b"cg\0")
    big_at = len(head) + sum(len(r) for r in R[:big_i])        # the CG record: far over three members
    cuts += list(range(big_at + 100, len(stream), 40000))
    cs.append(dict(name="foreign_cut", data=bgzf(stream, sorted(cuts)), keep_qual=True))
    cs.append(dict(name="foreign_plain_noqualkept", data=bgzf(stream), keep_qual=False))
    cs.append(dict(name="foreign_no_eof_extra", data=bgzf(stream, list(range(50000, len(stream), 50000)), level=1, eof=False, extra=b"XY\x03\0abc"), keep_qual=True))
    # QUAL absent on one record: no qualities in the set although asked for
    R2 = list(R); R2[3] = bam_record("len17", 0x10, 0, 130, 30, ops_of("17M"), "ACGTACGTACGTACGTA", None)
    cs.append(dict(name="foreign_one_qual_absent", data=bgzf(head + b"".join(R2), level=0), keep_qual=True))
    cs.append(dict(name="header_only", data=bgzf(head), keep_qual=True))
    return cs


def error_cases():
    """[dict(name, data, code, text)]: text must appear in telr_last_error"""
    head, R = record_stream()
    R = R[:12]
    stream = head + b"".join(R)
    t = stream[len(head):]
    first = member(deflate_raw(head), head)
    cs = []

    def two(name, second, text):
        cs.append(dict(name=name, data=first + second + EOF_MARKER, code=E_ARG, text=text))
    comp = deflate_raw(t)
    two("wrong_crc", member(comp, t, crc=zlib.crc32(t) ^ 0x10), "block 1")
    two("wrong_isize", member(comp, t, isize=len(t) + 1), "block 1")
    two("dist_before_start", member(fixed_deflate([1, 2, 3, (3, 5)]), b"123123"), "block 1")
    m = member(comp[:-9], t)
    two("past_end", m, "block 1")
    two("oversubscribed", member(_oversubscribed(), b"0123456789"), "block 1")
    cs.append(dict(name="wrong_magic", data=first + b"\x1f\x8b\x08\x00" + b"\0" * 30, code=E_ARG, text="block 1"))
    cs.append(dict(name="truncated_member", data=(first + member(comp, t))[:-5], code=E_ARG, text="block 1"))
    cs.append(dict(name="bytes_after", data=first + EOF_MARKER + b"junk", code=E_ARG, text="block 2"))
    bad = bam_record("midclip", 0, 0, 5, 9, ops_of("10M5S10M"), "A" * 25, None)
    cs.append(dict(name="clip_in_the_middle", data=bgzf(stream + bad), code=E_ARG, text="record %d" % len(R)))
    bad = bam_record("op9", 0, 0, 5, 9, [10 << 4 | 9], "A" * 10, None)
    cs.append(dict(name="op_above_8", data=bgzf(stream + bad + R[0]), code=E_ARG, text="record %d" % len(R)))
    cs.append(dict(name="truncated_last_record", data=bgzf(stream[:-7]), code=E_ARG, text="record %d" % (len(R) - 1)))
    bad = bam_record("huge", 0, 0, 5, 9, [((1 << 28) - 1) << 4 | 0, 1 << 4 | 7], "A" * 10, None)
    cs.append(dict(name="length_2_28", data=bgzf(stream + bad), code=E_RANGE, text="record %d" % len(R)))
    return cs
