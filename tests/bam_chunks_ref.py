"""What telr_bam_chunk_plan is documented to compute (include/telr_hip.h), in plain Python, and the files that put a chunk seam where a
chunked load can go wrong: the inputs of tests/test_bam_chunks_ref.py and tests/test_gpu_bam_chunks.py.

  * plan(isize, chunk_bytes): a chunk is a run of consecutive whole BGZF members; it closes before the member whose ISIZE would take
    its sum of ISIZE above chunk_bytes, and always holds at least one member.  Members of ISIZE 0 are members like any other;
  * chunk_streams(data, chunk_bytes): the inflated bytes of every chunk of a file;
  * seam_cases(): [dict(name, data, keep_qual, seam)] -- seam = (record index, offset inside the record) of a member cut where the case
    claims one, or None; with chunk_bytes = 1 every cut between members of two bytes and more is a chunk seam.
"""
import struct

import bam_in_ref as R


def plan(isize, chunk_bytes):
    """-> [first member of chunk c]"""
    assert chunk_bytes >= 1
    first, total = [], 0
    for m, n in enumerate(isize):
        if m == 0 or total + n > chunk_bytes:
            first.append(m); total = 0
        total += n
    return first


def chunk_streams(data, chunk_bytes):
    """the file's chunks as inflated bytes, in file order"""
    ms = R.hop(data)
    first = plan([m[2] for m in ms], chunk_bytes) + [len(ms)]
    return [b"".join(R.inflate_one(data[o:o + n], isz, crc) for o, n, isz, crc in ms[a:b]) for a, b in zip(first, first[1:])]


def member_cuts(data):
    """the offsets in the inflated stream at which a member ends and another one begins"""
    out, p = [], 0
    for _, _, isz, _ in R.hop(data)[:-1]:
        p += isz; out.append(p)
    return out


def record_starts(head, recs):
    out, p = [], len(head)
    for r in recs:
        out.append(p); p += len(r)
    return out


def _field_offsets(rec):
    """offsets inside a record (from its block_size field) of read_name, the CIGAR array, SEQ, QUAL and the tags"""
    lrn, ncig, lseq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    name = 36; cig = name + lrn; seq = cig + 4 * ncig; qual = seq + (lseq + 1) // 2; tags = qual + lseq
    return dict(name=name, cigar=cig, seq=seq, qual=qual, tags=tags)


def seam_cases():
    head, recs = R.record_stream()
    rng_q = lambda n, s: bytes((7 * i + s) % 60 for i in range(n))
    cs = []

    def one(name, recs_, i, off, keep_qual=True, eof=True, head_=head):
        """a file whose only inner member cuts lie 2 bytes before and exactly at offset `off` of record i: the second cut is the
        claimed seam, the 2-byte member before it is a chunk of its own at chunk_bytes = 1"""
        st = record_starts(head_, recs_)
        at = st[i] + off
        cs.append(dict(name=name, data=R.bgzf(head_ + b"".join(recs_), [at - 2, at], eof=eof), keep_qual=keep_qual, seam=(i, off), head=head_, recs=recs_))

    # a record with every field long enough to be cut inside: 100 bases (odd base 51 lies in byte 25 of SEQ), a B tag of 20 shorts
    tagb = b"xbB" + b"s" + struct.pack("<I", 20) + struct.pack("<20h", *range(20)) + R.tag_int("NM", "i", 4)
    big = R.bam_record("seamrecord", 0, 0, 321, 44, R.ops_of("10S30M2I20M3D30M8S"), "ACGTTGCAAC" * 10, rng_q(100, 3), tagb)
    base = recs[:5] + [big] + recs[5:9]
    i = 5
    F = _field_offsets(big)
    for off in (1, 2, 3):
        one("block_size_%d" % off, base, i, off)
    one("record_boundary", base, i, 0)
    one("inside_read_name", base, i, F["name"] + 4)
    one("inside_cigar", base, i, F["cigar"] + 10)                       # the middle of the third op
    one("inside_seq_odd_base", base, i, F["seq"] + 26)                  # behind byte 25: bases 50 | 51 ... 52 starts the next chunk's byte
    one("inside_qual", base, i, F["qual"] + 37)
    one("inside_b_tag", base, i, F["tags"] + 8 + 11)                    # inside the eleventh byte of the array's values
    # a supplementary and a secondary record two chunks before their primary; an orphan alone in the last chunk
    s = "ACGGTCAT" * 25
    prim = R.bam_record("far", 0, 0, 2000, 50, R.ops_of("20S150M30S"), s, rng_q(200, 5), R.tag_int("NM", "i", 2))
    supp = R.bam_record("far", 0x800, 1, 90, 9, R.ops_of("170H30M"), s[170:], rng_q(30, 6))
    seco = R.bam_record("far", 0x100, 1, 10, 0, R.ops_of("20S150M30S"), "", None)
    orph = R.bam_record("nobody", 0x100, 0, 40, 0, R.ops_of("30M"), "", None)
    rs = [supp, seco] + recs[0:3] + recs[3:6] + [prim, recs[6], recs[8], orph]          # (recs[7], ops1, is an orphan of its own: left out)
    st = record_starts(head, rs)
    cs.append(dict(name="supp_sec_two_chunks_before_primary_orphan_last", data=R.bgzf(head + b"".join(rs), [st[2], st[5], st[8], st[11]]), keep_qual=True,
                   seam=(11, 0), head=head, recs=rs))
    # the long1 and twice groups with a chunk between the two records of a name, in both orders: the first name wins
    long1 = [r for r in recs if r[36:42] == b"long1\0"]
    twice = [r for r in recs if r[36:42] == b"twice\0"]
    for tag, order in (("file_order", lambda x: x), ("reversed", lambda x: x[::-1])):
        l, t = order([long1[0], long1[3]]), order(twice)           # long1: the primary and the supplementary that carries the whole SEQ
        rs = [l[0], t[0]] + recs[0:4] + [l[1], t[1]] + long1[1:3]
        st = record_starts(head, rs)
        cs.append(dict(name="first_name_wins_" + tag, data=R.bgzf(head + b"".join(rs), [st[2], st[6]]), keep_qual=True, seam=(6, 0), head=head, recs=rs))
    # a header longer than 65,536 bytes: it spans chunks at either chunk size of the tests
    tn = ["contig_number_%05d_of_a_fragmented_assembly" % k for k in range(1500)]
    tl = [1000 + k for k in range(1500)]
    text = "@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(tn, tl))
    hbig = R.bam_header(tn, tl, text)
    assert len(hbig) > 2 * 65536
    rs = recs[0:7]
    cs.append(dict(name="long_header", data=R.bgzf(hbig + b"".join(rs), list(range(30000, len(hbig) + 200, 30000))), keep_qual=True, seam=None, head=hbig, recs=rs))
    # the last chunk is the EOF marker only (the member before it is above one byte) / there is no EOF marker
    rs = recs[0:9]
    cs.append(dict(name="eof_marker_alone", data=R.bgzf(head + b"".join(rs), [len(head) + 50]), keep_qual=True, seam=None, head=head, recs=rs))
    one("no_eof_marker", base, i, F["qual"] + 1, eof=False)
    # keep_qual with the one record without QUAL in the last chunk: no chunk's qualities may survive
    noq = R.bam_record("noqual", 0, 0, 130, 30, R.ops_of("17M"), "ACGTACGTACGTACGTA", None)
    rs = recs[0:9] + [noq]
    st = record_starts(head, rs)
    cs.append(dict(name="one_ff_in_the_last_chunk", data=R.bgzf(head + b"".join(rs), [st[4], st[9]]), keep_qual=True, seam=(9, 0), head=head, recs=rs))
    return cs


FILLER_COPIES = 700


def filler_file(n_copies):
    """a file of n_copies times the 40 filler records of record_stream (names made distinct), in 65,280-byte members: about 4 MB and 64
    members at n_copies = 1000.  The longest record does not depend on n_copies."""
    head, recs = R.record_stream()
    fill = [r for r in recs if r[36:37] == b"f" and r[37:38].isdigit()]
    body = bytearray()
    for c in range(n_copies):
        for r in fill:
            # the name keeps its length: its first byte counts the copies in a letter, the rest is numbered by position
            nm = bytearray(r); nm[36] = 65 + c % 26
            body += nm
    # names repeat every 26 copies: later copies are second primaries under a known name (no new read), which the definition handles
    return R.bgzf(head + bytes(body))
