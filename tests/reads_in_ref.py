"""telr_reads_load's definition in plain Python (include/telr_hip.h has it in words), and the cases that hold the
device loader to it.

  inflate_any(data)          the container by content -> (container, text, members, no_eof)
  parse(text, keep_qual)     the text -> Parsed(names, seqs, quals, fastq, lines), or (code, text) for a refusal
  load(data, keep_qual)      both; ReadsInError for a refusal

Errors: the container first (BGZF: the lowest block; gzip: what zlib says, "gzip: ..."), then the text's lowest offending record, grammar
before qualities inside one record.
"""
import random
import struct
import zlib

import bam_in_ref as B

E_ARG, E_RANGE = -3, -4
PLAIN, GZIP, BGZF = 0, 1, 2
COUNTERS = ("container", "fastq", "members", "text_bytes", "lines", "records", "bases", "no_eof")
W = "telr_reads_load: "
NO_AT, SHORT, NO_PLUS, LEN, QUAL = ("no '@' where a record starts", "the text ends inside the record", "no '+' line behind the bases",
                                    "bases and qualities differ in number", "a quality character outside 33..126")
NO_KIND = "the text opens with neither '@' nor '>'"
NO_CONTAINER = "neither gzip nor BGZF, and the file opens with neither '@' nor '>'"


class ReadsInError(Exception):
    def __init__(self, code, text):
        Exception.__init__(self, "%d: %s" % (code, text))
        self.code, self.text = code, text


class Parsed:
    def __init__(self, names, seqs, quals, fastq, lines):
        self.names, self.seqs, self.quals, self.fastq, self.lines = names, seqs, quals, fastq, lines


def lines_of(text):
    """the text's lines without their terminators: "\\n", "\\r\\n", or a lone "\\r" in front of the text's end"""
    parts = text.split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def name_of(line):
    n = line[1:]
    for i, c in enumerate(n):
        if c in b" \t\r":
            return n[:i].decode("latin-1")
    return n.decode("latin-1")


def parse(text, keep_qual=False):
    if not text:
        return Parsed([], [], None, 0, 0)
    if text[:1] not in (b"@", b">"):
        return E_ARG, W + NO_KIND
    ls = lines_of(text)
    names, seqs = [], []
    if text[:1] == b"@":
        quals = []
        for r in range((len(ls) + 3) // 4):
            rec = ls[4 * r:4 * r + 4]
            why = None
            if not rec[0].startswith(b"@"):
                why = NO_AT
            elif len(rec) < 4:
                why = SHORT
            elif not rec[2].startswith(b"+"):
                why = NO_PLUS
            elif len(rec[1]) != len(rec[3]):
                why = LEN
            elif keep_qual and any(c < 33 or c > 126 for c in rec[3]):
                why = QUAL
            if why:
                return E_ARG, W + "record %d: %s" % (r, why)
            names.append(name_of(rec[0])); seqs.append(rec[1]); quals.append(bytes(c - 33 for c in rec[3]) if keep_qual else None)
        return Parsed(names, seqs, quals if keep_qual else None, 1, len(ls))
    cur = None
    for ln in ls:
        if ln.startswith(b">"):
            if cur is not None:
                seqs.append(b"".join(cur))
            names.append(name_of(ln)); cur = []
        else:
            cur.append(ln)
    seqs.append(b"".join(cur))
    return Parsed(names, seqs, None, 0, len(ls))


def inflate_any(data):
    """-> (container, text, members, no_eof); ReadsInError"""
    if not data:
        return PLAIN, b"", 0, 0
    if data[:2] == b"\x1f\x8b":
        ms = None
        if data[2:3] == b"\x08":
            try:
                ms = B.hop(data)
            except B.BamInError:
                ms = None
        if ms is not None:
            parts = []
            for k, (off, n, isize, crc) in enumerate(ms):
                try:
                    parts.append(B.inflate_one(data[off:off + n], isize, crc))
                except B.InflateError as e:
                    raise ReadsInError(E_ARG, W + "block %d: %s" % (k, B.I_TEXT[e.status]))
            return BGZF, b"".join(parts), len(ms), 0 if data[-28:] == B.EOF_MARKER else 1
        out, rest, members = [], data, 0
        while rest:
            d = zlib.decompressobj(47)
            try:
                out.append(d.decompress(rest))
            except zlib.error as e:
                raise ReadsInError(E_ARG, W + "gzip: %s" % e)
            if not d.eof:
                raise ReadsInError(E_ARG, W + "gzip: the file ends inside a member")
            members += 1
            rest = d.unused_data
        return GZIP, b"".join(out), members, 0
    if data[:1] in (b"@", b">"):
        return PLAIN, data, 0, 0
    raise ReadsInError(E_ARG, W + NO_CONTAINER)


class Loaded:
    pass


def load(data, keep_qual=False):
    container, text, members, no_eof = inflate_any(data)
    p = parse(text, keep_qual)
    if isinstance(p, tuple):
        raise ReadsInError(*p)
    L = Loaded()
    L.names, L.seqs, L.quals, L.fastq = p.names, p.seqs, p.quals, p.fastq
    L.counters = dict(container=container, fastq=p.fastq, members=members, text_bytes=len(text), lines=p.lines, records=len(p.seqs),
                      bases=sum(len(s) for s in p.seqs), no_eof=no_eof)
    return L


_NORM = bytearray(b"N" * 256)
for _c, _b in zip(b"ACGTUacgtu", b"ACGTTACGTT"):
    _NORM[_c] = _b
_NORM = bytes(_NORM)


def norm(seq):
    """a read's bytes as the set holds them: A C G T, anything else N (str, what bam_in_ref.packed_words takes)"""
    return bytes(seq).translate(_NORM).decode()


def qual_layout(seqs, quals):
    """the Phred bytes in the set's base layout: read i at the 64-base padded lengths before it, zero in the padding"""
    out = bytearray()
    for s, q in zip(seqs, quals):
        out += q + bytes((len(s) + 63) // 64 * 64 - len(s))
    return bytes(out)


# ---- containers ---------------------------------------------------------------------------------------------------------------
CONTAINERS = ("plain", "gz6", "gz3m", "gz0", "bgzf")


def gz(text, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def container(kind, text, cuts=None, eof=True):
    if kind == "plain":
        return text
    if kind == "gz6":
        return gz(text, 6)
    if kind == "gz0":
        return gz(text, 0)
    if kind == "gz3m":
        a, b = len(text) // 3, 2 * len(text) // 3
        return gz(text[:a], 6) + gz(text[a:b], 1) + gz(text[b:], 9)
    if kind == "bgzf":
        return B.bgzf(text, cuts, eof=eof)
    raise ValueError(kind)


def want_container(kind, text):
    """the container counter of a file made by container(): a plain empty text is an empty file"""
    return {"plain": PLAIN, "bgzf": BGZF}.get(kind, GZIP)


# ---- cases --------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]          # 4,095 / 4,096: the scan's tile of 4,096 records


def _dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _q(rng, n):
    return bytes(rng.randrange(33, 127) for _ in range(n))


def fastq(recs, eol=b"\n", last_eol=True, plus=b"+"):
    """recs: [(name bytes, bases, quality characters)]; eol: bytes, or a function of the line number"""
    out, j = b"", 0
    for name, s, q in recs:
        for ln in (b"@" + name, s, plus, q):
            out += ln + (eol(j) if callable(eol) else eol); j += 1
    if not last_eol:
        out = out[:-len(eol(j - 1) if callable(eol) else eol)]
    return out


def fasta(recs, width=60, eol=b"\n", last_eol=True):
    """width: a number, or a function of (record, line) -> the line's width"""
    out = b""
    for i, (name, s) in enumerate(recs):
        out += b">" + name + eol
        p, k = 0, 0
        while p < len(s):
            w = width(i, k) if callable(width) else width
            out += s[p:p + w] + eol; p += w; k += 1
    if not last_eol and out.endswith(eol):
        out = out[:-len(eol)]
    return out


def _recs(rng, lens, prefix=b"r"):
    return [(prefix + str(i).encode(), _dna(rng, n), _q(rng, n)) for i, n in enumerate(lens)]


def _case(name, text, cuts=None, chunks=(), eof=True):
    return dict(name=name, text=text, cuts=cuts, chunks=tuple(chunks), eof=eof)


def _sized(rng, size):
    """a FASTQ of exactly `size` bytes: 200-base reads and one that fills the rest"""
    text = fastq(_recs(rng, [200] * ((size - 600) // 410)))
    rest = size - len(text)                      # the last record: '@' name LF bases LF '+' LF qualities LF = 2 n + len(name) + 6
    nm = 1 if (rest - 7) % 2 == 0 else 2
    n = (rest - 6 - nm) // 2
    text += fastq([(b"z" * nm, _dna(rng, n), _q(rng, n))])
    assert len(text) == size, (len(text), size)
    return text


def fastq_cases():
    rng = random.Random(11)
    cs = []
    cs.append(_case("fq_lengths", fastq(_recs(rng, LENGTHS))))
    cs.append(_case("fq_names_0_17", fastq([(b"n" * k + (b" extra words" if k % 3 == 0 else b"\tx" if k % 3 == 1 else b""), _dna(rng, 37), _q(rng, 37)) for k in range(18)])))
    cs.append(_case("fq_crlf", fastq(_recs(rng, LENGTHS), eol=b"\r\n")))
    cs.append(_case("fq_crlf_mixed", fastq(_recs(rng, LENGTHS), eol=lambda j: b"\r\n" if (j * 7 + j // 3) % 3 == 0 else b"\n")))
    cs.append(_case("fq_no_last_lf", fastq(_recs(rng, [5, 64, 17]), last_eol=False)))
    cs.append(_case("fq_last_lone_cr", fastq(_recs(rng, [5, 64, 17]), last_eol=False) + b"\r"))
    odd = b"acgtuUNnRYKMSWBDHVrykm*- AC\x80\xff\x00.GT"
    cs.append(_case("fq_alphabet", fastq([(b"odd", odd, _q(rng, len(odd))), (b"lower", b"acgtacgtnnacgu" * 5, _q(rng, 70))])))
    cs.append(_case("fq_qual_at_plus", fastq([(b"a", b"ACGTA", b"@IIII"), (b"b", b"ACGTAC", b"+IIII@"), (b"c", b"AC", b"@+")])))
    cs.append(_case("fq_plus_name", fastq(_recs(rng, [20, 3]), plus=b"+r1 the same name again")))
    cs.append(_case("fq_qual_33_126", fastq([(b"e", b"ACGTACGT", b"!~!~~!!~"), (b"f", b"A", b"~"), (b"g", b"C", b"!")])))
    for n in COUNTS:
        cs.append(_case("fq_count_%d" % n, fastq(_recs(rng, [1 + (i * 5 + i // 7) % 3 for i in range(n)]))))
    cs.append(_case("fq_long_70001", fastq(_recs(rng, [3, 70001, 2]))))
    for size in (65520, 65536, 65537):          # the scan's tile of 4,096 blocks of 16 text bytes, and one byte more
        cs.append(_case("fq_text_%d" % size, _sized(rng, size)))
    return cs


def fasta_cases():
    rng = random.Random(12)
    cs = []
    recs = [(b"s%d some text" % i, _dna(rng, n)) for i, n in enumerate(LENGTHS)]
    for w in (1, 60, 64, 70):
        cs.append(_case("fa_width_%d" % w, fasta(recs, w)))
    cs.append(_case("fa_width_mixed", fasta(recs, lambda i, k: (7, 60, 1, 33, 64)[(i + 2 * k) % 5])))
    cs.append(_case("fa_crlf", fasta(recs, 60, eol=b"\r\n")))
    cs.append(_case("fa_no_last_lf", fasta(recs[:6], 16, last_eol=False)))
    cs.append(_case("fa_last_lone_cr", fasta(recs[:6], 16, last_eol=False) + b"\r"))
    cs.append(_case("fa_empty_lines", b">a\n\nACGT\n\n\nAC\n>b\n\n>c\n\nTTTT\nGG\n\n"))
    cs.append(_case("fa_header_only", b">first\n>second x\nACGTACGTAC\nGT\n>mid\n>after\nAAAA\n>last\n"))
    cs.append(_case("fa_single_lines", fasta(recs, 1000)))
    cs.append(_case("fa_one_line", b">only"))
    cs.append(_case("fa_one_line_lf", b">\n"))
    cs.append(_case("fa_alphabet", b">x\nacgtuUNn*RY\nK M\x80\xffAC\n"))
    cs.append(_case("fa_long_70001", fasta([(b"a", _dna(rng, 3)), (b"big", _dna(rng, 70001)), (b"c", _dna(rng, 2))], 70)))
    cs.append(_case("fa_count_4097", fasta([(b"%d" % i, _dna(rng, 1 + i % 3)) for i in range(4097)], 2)))
    return cs


def seam_cases():
    """cuts (BGZF members, and chunk_bytes for gzip and plain) inside a name, inside the bases, directly before a line feed, between
    "\\r" and "\\n", directly behind a record's last line feed, behind the '+'"""
    rng = random.Random(13)
    cs = []
    for eol, tag in ((b"\n", "lf"), (b"\r\n", "crlf")):
        recs = [(b"read%d/first" % i, _dna(rng, 40 + i), _q(rng, 40 + i)) for i in range(4)]
        text = fastq(recs, eol=eol)
        r1 = len(fastq(recs[:1], eol=eol))                      # where record 1 starts
        nm, bs = r1 + 4, r1 + len(b"@read1/first") + len(eol) + 9
        lf = text.index(b"\n", r1)                              # the header's line feed
        plus = text.index(b"+", r1 + 60) + 1
        r2 = len(fastq(recs[:2], eol=eol))
        places = sorted(set([nm, bs, lf, r2, plus] + ([lf - 1, lf] if eol == b"\r\n" else [])))
        cs.append(_case("seam_fq_%s" % tag, text, cuts=places, chunks=places))
        cs.append(_case("seam_fq_%s_each" % tag, text, cuts=list(range(1, len(text), 7))))
    recs = [(b"s%d" % i, _dna(rng, 150 + i)) for i in range(4)]
    text = fasta(recs, 60)
    r1 = len(fasta(recs[:1], 60))
    places = sorted(set([r1 + 2, r1 + 10, text.index(b"\n", r1), r1, len(fasta(recs[:2], 60)), r1 + 4 + 61]))
    cs.append(_case("seam_fa", text, cuts=places, chunks=places))
    cs.append(_case("seam_fa_each", text, cuts=list(range(1, len(text), 11))))
    big = fastq(_recs(rng, [10, 12000, 7, 30]))
    cs.append(_case("seam_fq_span", big, cuts=list(range(5000, len(big), 5000)), chunks=(5000,)))
    bigfa = fasta([(b"a", _dna(rng, 10)), (b"b", _dna(rng, 24000)), (b"c", _dna(rng, 30))], 60)
    cs.append(_case("seam_fa_span", bigfa, cuts=list(range(5000, len(bigfa), 5000)), chunks=(5000,)))
    small = fastq(_recs(rng, [5, 6, 7]))
    cs.append(_case("seam_empty_member", small, cuts=[20, 20, 41, 41, 41]))
    cs.append(_case("seam_no_eof", small, cuts=[33], eof=False))
    cs.append(_case("seam_eof_only", b""))
    return cs


def cases():
    return fastq_cases() + fasta_cases() + seam_cases()


def _ecase(name, data, code, text, keep_qual=False, exact=True):
    return dict(name=name, data=data, code=code, text=text, keep_qual=keep_qual, exact=exact)


def text_error_cases():
    """faults of the text: (name, text, code, the error text, keep_qual)"""
    rng = random.Random(14)
    recs = _recs(rng, [10, 20, 30, 40, 50])
    good = fastq(recs)
    ls = good.split(b"\n")[:-1]

    def join(lines):
        return b"\n".join(lines) + b"\n"

    def drop_at(r):
        x = list(ls); x[4 * r] = x[4 * r][1:]; return join(x)
    out = []
    out.append(_ecase("first_byte", b"ACGT\nACGT\n", E_ARG, NO_KIND))
    out.append(_ecase("no_at_0", drop_at(0), E_ARG, NO_KIND))
    out.append(_ecase("no_at_mid", drop_at(2), E_ARG, "record 2: " + NO_AT))
    out.append(_ecase("no_at_last", drop_at(4), E_ARG, "record 4: " + NO_AT))
    x = list(ls); x[4 * 1 + 2] = b"-"; out.append(_ecase("no_plus", join(x), E_ARG, "record 1: " + NO_PLUS))
    x = list(ls); x[4 * 3 + 1] += b"A"; out.append(_ecase("seq_longer", join(x), E_ARG, "record 3: " + LEN))
    x = list(ls); x[4 * 3 + 1] = x[4 * 3 + 1][:-1]; out.append(_ecase("seq_shorter", join(x), E_ARG, "record 3: " + LEN))
    for k in (1, 2, 3):
        out.append(_ecase("trailing_%d" % k, good + join(ls[:k]), E_ARG, "record 5: " + SHORT))
    out.append(_ecase("trailing_1_no_lf", good + b"@x", E_ARG, "record 5: " + SHORT))
    out.append(_ecase("empty_line_mid", join(ls[:8] + [b""] + ls[8:]), E_ARG, "record 2: " + NO_AT))
    out.append(_ecase("trailing_empty_line", good + b"\n", E_ARG, "record 5: " + NO_AT))
    out.append(_ecase("two_line_record", join(ls[:5] + [b"ACGT"] + ls[5:]), E_ARG, "record 1: " + NO_PLUS))
    for c, tag in ((32, "32"), (127, "127")):
        x = list(ls); q = bytearray(x[4 * 2 + 3]); q[7] = c; x[4 * 2 + 3] = bytes(q)
        out.append(_ecase("qual_%s" % tag, join(x), E_ARG, "record 2: " + QUAL, keep_qual=True))
        out.append(_ecase("qual_%s_ignored" % tag, join(x), 0, "", keep_qual=False))
    x = list(ls); q = bytearray(x[4 * 1 + 3]); q[3] = 31; x[4 * 1 + 3] = bytes(q); x[4 * 3] = x[4 * 3][1:]
    out.append(_ecase("qual_below_grammar", join(x), E_ARG, "record 1: " + QUAL, keep_qual=True))
    return out


def file_error_cases():
    """faults of the container: whole files"""
    rng = random.Random(15)
    text = fastq(_recs(rng, [100, 200, 300, 400]))
    out = []
    bg = bytearray(B.bgzf(text, [300, 700]))
    ms = B.hop(bytes(bg))

    def flipped(data, at):
        x = bytearray(data); x[at] ^= 0x10; return bytes(x)
    out.append(dict(name="bgzf_flipped_bit", data=flipped(bg, ms[1][0] + ms[1][1] // 2), container=BGZF))
    x = bytearray(bg); x[ms[1][0] + ms[1][1]] ^= 0xff
    out.append(dict(name="bgzf_wrong_crc", data=bytes(x), container=BGZF))
    x = bytearray(bg); struct.pack_into("<I", x, ms[1][0] + ms[1][1] + 4, ms[1][2] + 1)
    out.append(dict(name="bgzf_wrong_isize", data=bytes(x), container=BGZF))
    out.append(dict(name="bgzf_truncated", data=bytes(bg[:ms[2][0] + 5]), container=GZIP))
    g = gz(text)
    out.append(dict(name="gzip_flipped_bit", data=flipped(g, len(g) // 2), container=GZIP))
    x = bytearray(g); x[-8] ^= 0xff
    out.append(dict(name="gzip_wrong_crc", data=bytes(x), container=GZIP))
    x = bytearray(g); x[-4] ^= 0x01
    out.append(dict(name="gzip_wrong_isize", data=bytes(x), container=GZIP))
    out.append(dict(name="gzip_truncated", data=g[:len(g) // 2], container=GZIP))
    out.append(dict(name="gzip_member_then_bytes", data=g + b"trailing bytes", container=GZIP))
    out.append(dict(name="not_a_container", data=b"\x00\x01ACGT", container=PLAIN))
    return out


def big_member_file():
    """one BGZF-shaped member of more than 65,536 bytes of text: no BGZF, a gzip member like any other"""
    rng = random.Random(16)
    text = fastq([(b"r%d" % i, b"ACGT" * 200, b"I" * 800) for i in range(50)])
    assert len(text) > 65536
    return B.member(B.deflate_raw(text), text) + B.EOF_MARKER, text


# ---- the case file of tools/ubench/reads_text_host.cpp ------------------------------------------------------------------------
_STATUS = {NO_AT: 1, SHORT: 2, NO_PLUS: 3, LEN: 4, QUAL: 5}


def host_cases():
    """(name, text, keep_qual) of every case and every text fault"""
    out = [(c["name"], c["text"], c["text"][:1] == b"@") for c in cases()]
    out += [(c["name"], c["text"], False) for c in fastq_cases()[:6]]
    out += [(e["name"], e["data"], e["keep_qual"]) for e in text_error_cases()]
    return out


def write_case_file(path):
    """-> the number of cases.  Per case: name, keep_qual, the wanted status and record, the text; for status 0 the records (length,
    name), the 2-bit words, the mask words and the Phred bytes of the definition"""
    import numpy as np
    hc = host_cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(hc)))
        for name, text, kq in hc:
            p = parse(text, kq)
            status, record = 0, -1
            if isinstance(p, tuple):
                if NO_KIND in p[1]:
                    status = 100
                else:
                    head, why = p[1][len(W):].split(": ", 1)
                    status, record = _STATUS[why], int(head.split()[1])
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<IiqQ", 1 if kq else 0, status, record, len(text)) + text)
            if status:
                continue
            f.write(struct.pack("<II", len(p.seqs), p.fastq))
            for n, s in zip(p.names, p.seqs):
                b = n.encode("latin-1")
                f.write(struct.pack("<iI", len(s), len(b)) + b)
            w2, wn = B.packed_words([norm(s) for s in p.seqs])
            f.write(struct.pack("<Q", len(w2)) + np.asarray(w2, "<u4").tobytes() + struct.pack("<Q", len(wn)) + np.asarray(wn, "<u4").tobytes())
            q = qual_layout(p.seqs, p.quals) if p.quals is not None else b""
            f.write(struct.pack("<IQ", 1 if p.quals is not None else 0, len(q)) + q)
    return len(hc)
