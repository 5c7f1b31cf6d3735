"""The plain BAM encoder (tests/bam_reference.py) against strings written out by hand from the SAM specification, the
optional-fields document and minimap2's manual, and the hand-built cases of tests/bam_edges.py against their own edges.
CPU only: tests/test_gpu_bam_edges.py holds the writers to this reference."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bam_edges as be
import bam_reference as br
from telr_amd._abi import ALN_DTYPE, F_PRIMARY, F_SECONDARY, F_SUPPL, F_REV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T20 = "ACGTACGTACGTACGTACGT"
OPS = {"M": 0, "I": 1, "D": 2}


def aln(qid, tid, qlen, qs, qe, ts, cigar, flags, cigs, **kw):
    ops = [(int(n) << 4) | OPS[o] for n, o in re.findall(r"(\d+)([MID])", cigar)]
    a = np.zeros(1, ALN_DTYPE)
    a["qid"] = qid; a["tid"] = tid; a["qlen"] = qlen; a["qs"] = qs; a["qe"] = qe; a["ts"] = ts
    a["te"] = ts + sum(x >> 4 for x in ops if x & 15 != 1); a["n_cigar"] = len(ops); a["cigar_off"] = len(cigs); a["flags"] = flags; a["mapq"] = 60
    for k, v in kw.items():
        a[k] = v
    cigs += ops
    return a


def tags_of(t):
    """{tag: (type, value)} and the order of the tags"""
    out, order, p = {}, [], 0
    while p < len(t):
        tag, ty = t[p:p + 2].decode(), chr(t[p + 2]); p += 3
        if ty == "i":
            v = struct.unpack_from("<i", t, p)[0]; p += 4
        elif ty == "A":
            v = chr(t[p]); p += 1
        elif ty == "Z":
            e = t.index(b"\0", p); v = t[p:e].decode(); p = e + 1
        elif ty == "B":
            assert chr(t[p]) == "I"
            n = struct.unpack_from("<I", t, p + 1)[0]; v = list(struct.unpack_from("<%dI" % n, t, p + 5)); p += 5 + 4 * n
        else:
            raise AssertionError("tag type " + ty)
        out[tag] = (ty, v); order.append(tag)
    return out, order


def cigar_text(ops):
    return "".join("%d%s" % (c >> 4, br.CIGAR_OPS[c & 15]) for c in ops)


# name, target, ts, read as stored, qs, qe, reverse, CIGAR of the aligned part | MD, cs, NM, SEQ bytes (hex), CIGAR of the record
HAND = [
    ("perfect", T20, 0, "ACGTACGT", 0, 8, 0, "8M", "8", ":8", 0, "12481248", "8M"),
    ("one mismatch", T20, 0, "ACGAACGT", 0, 8, 0, "8M", "3T4", ":3*ta:4", 1, "12411248", "8M"),
    ("first column", T20, 0, "TCGTACGT", 0, 8, 0, "8M", "0A7", "*at:7", 1, "82481248", "8M"),
    ("last column", T20, 0, "ACGTACGA", 0, 8, 0, "8M", "7T0", ":7*ta", 1, "12481241", "8M"),
    ("first and last", T20, 0, "TCGTACGA", 0, 8, 0, "8M", "0A6T0", "*at:6*ta", 2, "82481241", "8M"),
    ("adjacent mismatches", T20, 0, "ACTAACGT", 0, 8, 0, "8M", "2G0T4", ":2*gt*ta:4", 2, "12811248", "8M"),
    ("every column", T20, 0, "TTTA", 0, 4, 0, "4M", "0A0C0G0T0", "*at*ct*gt*ta", 4, "8881", "4M"),
    ("deletion", T20, 0, "ACGTGT", 0, 6, 0, "4M2D2M", "4^AC2", ":4-ac:2", 2, "124848", "4M2D2M"),
    ("deletion then mismatch", T20, 0, "ACGTTT", 0, 6, 0, "4M2D2M", "4^AC0G1", ":4-ac*gt:1", 3, "124888", "4M2D2M"),
    ("mismatch then deletion", T20, 0, "ACGAGT", 0, 6, 0, "4M2D2M", "3T0^AC2", ":3*ta-ac:2", 3, "124148", "4M2D2M"),
    ("insertion", T20, 0, "ACGTTTACGT", 0, 10, 0, "4M2I4M", "8", ":4+tt:4", 2, "1248881248", "4M2I4M"),
    ("M of length 1", T20, 0, "ATTCGT", 0, 6, 0, "1M2I3M", "4", ":1+tt:3", 2, "188248", "1M2I3M"),
    ("D then I", T20, 0, "ACGTGGGT", 0, 8, 0, "4M2D2I2M", "4^AC2", ":4-ac+gg:2", 4, "12484448", "4M2D2I2M"),
    ("I then D", T20, 0, "ACGTGGGT", 0, 8, 0, "4M2I2D2M", "4^AC2", ":4+gg-ac:2", 4, "12484448", "4M2I2D2M"),
    ("D I D", T20, 0, "ACGTGGT", 0, 7, 0, "4M1D1I1D2M", "4^A0^C2", ":4-a+g-c:2", 3, "12484480", "4M1D1I1D2M"),
    ("N in the read", T20, 0, "ACNTACGT", 0, 8, 0, "8M", "2G5", ":2*gn:5", 1, "12f81248", "8M"),
    ("N in the target", "ACNTACGTAC", 0, "ACGTACGT", 0, 8, 0, "8M", "2N5", ":2*ng:5", 1, "12481248", "8M"),
    ("N in both", "ACNTACGTAC", 0, "ACNTACGT", 0, 8, 0, "8M", "2N5", ":2*nn:5", 1, "12f81248", "8M"),
    ("lower case and IUPAC", T20, 0, "acgRacgt", 0, 8, 0, "8M", "3T4", ":3*tn:4", 1, "124f1248", "8M"),
    ("odd length", T20, 0, "ACG", 0, 3, 0, "3M", "3", ":3", 0, "1240", "3M"),
    ("one base", T20, 3, "T", 0, 1, 0, "1M", "1", ":1", 0, "80", "1M"),
    ("start inside the target", T20, 4, "ACGTAC", 0, 6, 0, "6M", "6", ":6", 0, "124812", "6M"),
    ("reverse strand", T20, 0, "ACGTTCGT", 0, 8, 1, "8M", "3T4", ":3*ta:4", 1, "12411248", "8M"),
    ("soft clips", T20, 0, "GGACGTACGTT", 2, 10, 0, "8M", "8", ":8", 0, "441248124880", "2S8M1S"),
    ("soft clips, reverse", T20, 0, "GGACGTACGTT", 2, 10, 1, "8M", "8", ":8", 0, "112481248220", "1S8M2S"),
    ("5' clip only", T20, 0, "GGACGTACGT", 2, 10, 0, "8M", "8", ":8", 0, "4412481248", "2S8M"),
    ("3' clip only", T20, 0, "ACGTACGTT", 0, 8, 0, "8M", "8", ":8", 0, "1248124880", "8M1S"),
    # the optional-fields document's own example: 10 matches, an A on the reference, 5 matches, the deletion of AC, 6 matches
    ("MD example of the specification", "CCCCCCCCCCAGGGGGACTTTTTT", 0, "CCCCCCCCCCGGGGGGTTTTTT", 0, 22, 0, "16M2D6M", "10A5^AC6", ":10*ag:5-ac:6", 3,
     "2222222222444444888888", "16M2D6M"),
    ("numbers of three digits", "C" * 100 + "A" + "C" * 19, 0, "C" * 100 + "G" + "C" * 19, 0, 120, 0, "120M", "100A19", ":100*ag:19", 1, "22" * 50 + "42" + "22" * 9, "120M"),
]


@pytest.mark.parametrize("h", HAND, ids=[h[0].replace(" ", "_") for h in HAND])
def test_hand_derived_records(h):
    name, target, ts, read, qs, qe, rev, cigar, md, cs, nm, seq_hex, rec_cigar = h
    cigs = []
    a = aln(0, 0, len(read), qs, qe, ts, cigar, F_PRIMARY | (F_REV if rev else 0), cigs, dp_score=-5, cnt=3, score=40, subsc=7)
    s = br.bam_stream(a, np.array(cigs, np.uint32), [read], [target], ["rd"], ["tg"], br.SAM_MD | br.SAM_CS | br.SAM_SOFTCLIP, None, "x")
    (off, refid, pos, bn, mapq, flag, qname, ops, l_seq, seq, tags), = br.parse_records(s.raw)
    t, order = tags_of(tags)
    assert (refid, pos, mapq, flag, qname) == (0, ts, 60, 16 if rev else 0, "rd")
    assert bn == 4681 and cigar_text(ops) == rec_cigar and l_seq == len(read) and seq.hex() == seq_hex
    assert t["MD"] == ("Z", md) and t["cs"] == ("Z", cs) and t["NM"] == ("i", nm)
    assert order == ["NM", "AS", "MD", "cs", "tp", "cm", "s1", "s2"]
    assert (t["AS"], t["tp"], t["cm"], t["s1"], t["s2"]) == (("i", -5), ("A", "P"), ("i", 3), ("i", 40), ("i", 7))
    assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", md)
    # QUAL 0xff, mate fields absent, block_size to the last tag byte
    body = s.raw[off:]
    assert struct.unpack_from("<i", body, 0)[0] == len(body) - 4 and struct.unpack_from("<iii", body, 24) == (-1, -1, 0)
    q0 = 36 + 3 + 4 * len(ops) + (l_seq + 1) // 2
    assert body[q0:q0 + l_seq] == b"\xff" * l_seq and body[q0 + l_seq:] == tags
    # the same record as SAM text: the table's own strings, SEQ spelled from its 4-bit codes
    seq_txt = "".join({"1": "A", "2": "C", "4": "G", "8": "T", "f": "N"}[x] for x in seq_hex[:l_seq])
    assert br.sam_records(s) == ["rd\t%d\ttg\t%d\t60\t%s\t*\t0\t0\t%s\t*\tNM:i:%d\tAS:i:-5\tMD:Z:%s\tcs:Z:%s\ttp:A:P\tcm:i:3\ts1:i:40\ts2:i:7"
                                 % (16 if rev else 0, ts + 1, rec_cigar, seq_txt, nm, md, cs)]


def test_hand_derived_tag_bytes_and_header():
    cigs = []
    a = aln(0, 0, 8, 0, 8, 0, "8M", F_PRIMARY, cigs, dp_score=6, cnt=1, score=8, subsc=0)
    s = br.bam_stream(a, np.array(cigs, np.uint32), ["ACGAACGT"], [T20], ["r"], ["chr1"], br.SAM_MD | br.SAM_CS, ("g1", "sm", "lb"), "cmd -x")
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:20\n@RG\tID:g1\tSM:sm\tLB:lb\n@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:cmd -x\n"
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 20)
    assert s.raw[:s.head_len] == head and s.offsets == [len(head)]
    want = (struct.pack("<iiiBBHHHiiii", 32 + 2 + 4 + 4 + 8 + 63, 0, 0, 2, 60, 4681, 1, 0, 8, -1, -1, 0) + b"r\0" + struct.pack("<I", 8 << 4) + bytes.fromhex("12411248") + b"\xff" * 8
            + b"NMi\1\0\0\0ASi\6\0\0\0MDZ3T4\0csZ:3*ta:4\0tpAPcmi\1\0\0\0s1i\x08\0\0\0s2i\0\0\0\0RGZg1\0")
    assert s.raw[s.head_len:] == want
    line = "r\t0\tchr1\t1\t60\t8M\t*\t0\t0\tACGAACGT\t*\tNM:i:1\tAS:i:6\tMD:Z:3T4\tcs:Z::3*ta:4\ttp:A:P\tcm:i:1\ts1:i:8\ts2:i:0\tRG:Z:g1\n"
    assert br.sam_text(s) == text + line
    assert br.sam_text(s, coordinate_sorted=False) == "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + text[text.index("@SQ"):] + line


def test_hand_derived_sa_clips_secondary_and_unmapped():
    """a read of two pieces (forward on t0, reverse on t1, overlapping a secondary of the first), an unmapped read between"""
    read = "ACGTACGT" + "TACGTAC"          # the second piece is GTACGTA (t1[2:9]) as the read shows its reverse strand
    cigs = []
    al = np.concatenate([aln(0, 0, 15, 0, 8, 0, "8M", F_PRIMARY, cigs, mapq=60), aln(0, 0, 15, 0, 8, 4, "8M", F_SECONDARY, cigs, mapq=0),
                         aln(0, 1, 15, 8, 15, 2, "7M", F_SUPPL | F_REV, cigs, mapq=30), aln(2, 1, 4, 0, 4, 0, "4M", F_PRIMARY, cigs)])
    reads, names = [read, "GNA", "ACGT"], ["two", "lost", "z"]
    for flags, clip, l_seq, seq in ((br.SAM_SOFTCLIP, "7M8S", 15, "GTACGTAACGTACGT"), (0, "7M8H", 7, "GTACGTA")):
        s = br.bam_stream(al, np.array(cigs, np.uint32), reads, [T20, T20], names, ["t0", "t1"], flags, None, "x")
        recs = br.parse_records(s.raw)
        # refID, position, forward before reverse, input order; the unmapped read last
        assert [(r[1], r[2], r[5], r[6]) for r in recs] == [(0, 0, 0, "two"), (0, 4, 0x100, "two"), (1, 0, 0, "z"), (1, 2, 0x810, "two"), (-1, -1, 4, "lost")]
        pri, sec, z, sup, un = recs
        assert tags_of(pri[10])[0]["SA"] == ("Z", "t1,3,-,7M8S,30,0;") and cigar_text(pri[7]) == "8M7S" and pri[8] == 15
        assert tags_of(sup[10])[0]["SA"] == ("Z", "t0,1,+,8M7S,60,0;") and cigar_text(sup[7]) == clip and sup[8] == l_seq
        assert sup[9] == br.seq4(seq) and tags_of(sup[10])[1] == ["NM", "AS", "SA", "tp", "cm", "s1", "s2"]
        t, order = tags_of(sec[10])
        assert order == ["NM", "AS", "tp", "cm", "s1"] and t["tp"] == ("A", "S") and sec[8] == 0 and sec[9] == b"" and cigar_text(sec[7]) == "8M7S"
        assert "SA" not in tags_of(z[10])[0]
        assert (un[3], un[4], un[7], un[8], un[9], un[10]) == (4680, 0, (), 3, bytes.fromhex("4f10"), b"")
        # as SAM text: coordinate order, and the order of the reads with the unmapped one at its place
        sq = "@SQ\tSN:t0\tLN:20\n@SQ\tSN:t1\tLN:20\n@PG\tID:telr_amd\tPN:telr_amd\tVN:0.1.0\tCL:x\n"
        l_pri = "two\t0\tt0\t1\t60\t8M7S\t*\t0\t0\tACGTACGTTACGTAC\t*\tNM:i:0\tAS:i:0\tSA:Z:t1,3,-,7M8S,30,0;\ttp:A:P\tcm:i:0\ts1:i:0\ts2:i:0\n"
        l_sec = "two\t256\tt0\t5\t0\t8M7S\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:0\ttp:A:S\tcm:i:0\ts1:i:0\n"
        l_z = "z\t0\tt1\t1\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0\tAS:i:0\ttp:A:P\tcm:i:0\ts1:i:0\ts2:i:0\n"
        l_sup = "two\t2064\tt1\t3\t30\t%s\t*\t0\t0\t%s\t*\tNM:i:0\tAS:i:0\tSA:Z:t0,1,+,8M7S,60,0;\ttp:A:P\tcm:i:0\ts1:i:0\ts2:i:0\n" % (clip, seq)
        l_un = "lost\t4\t*\t0\t0\t*\t*\t0\t0\tGNA\t*\n"
        assert br.sam_text(s) == "@HD\tVN:1.6\tSO:coordinate\n" + sq + l_pri + l_sec + l_z + l_sup + l_un
        assert br.sam_text(s, coordinate_sorted=False) == "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + sq + l_pri + l_sec + l_sup + l_un + l_z
        assert br.sam_text(s, keep=lambda f: not f & 0x900) == "@HD\tVN:1.6\tSO:coordinate\n" + sq + l_pri + l_z + l_un
    s = br.bam_stream(al, np.array(cigs, np.uint32), reads, [T20, T20], names, ["t0", "t1"], br.SAM_NO_UNMAPPED, ("g", "g", "l"), "x")
    assert len(s.recs) == 4 and all(r[10].endswith(b"RGZg\0") for r in br.parse_records(s.raw))


def test_hand_derived_reverse_primary_with_sa():
    """a read whose first 7 bases lie on the reverse strand at t[1:8] with one mismatch (primary) and whose last 5 lie forward at
    t[12:17] (supplementary).  The reverse strand of the read is TACGTCGTTCGT: 5 clipped bases, then CGTTCGT against CGTACGT."""
    cigs = []
    al = np.concatenate([aln(0, 0, 12, 0, 7, 1, "7M", F_PRIMARY | F_REV, cigs, mlen=6, blen=7), aln(0, 0, 12, 7, 12, 12, "5M", F_SUPPL, cigs, mapq=30, mlen=5, blen=5)])
    s = br.bam_stream(al, np.array(cigs, np.uint32), ["ACGAACGACGTA"], [T20], ["rv"], ["tg"], br.SAM_MD | br.SAM_CS | br.SAM_SOFTCLIP, None, "x")
    assert br.sam_records(s) == [
        "rv\t16\ttg\t2\t60\t5S7M\t*\t0\t0\tTACGTCGTTCGT\t*\tNM:i:1\tAS:i:0\tMD:Z:3A3\tcs:Z::3*at:3\tSA:Z:tg,13,+,7S5M,30,0;\ttp:A:P\tcm:i:0\ts1:i:0\ts2:i:0",
        "rv\t2048\ttg\t13\t30\t7S5M\t*\t0\t0\tACGAACGACGTA\t*\tNM:i:0\tAS:i:0\tMD:Z:5\tcs:Z::5\tSA:Z:tg,2,-,5S7M,60,1;\ttp:A:P\tcm:i:0\ts1:i:0\ts2:i:0"]


def test_reg2bin_at_the_boundaries_of_every_level():
    """the specification's definition at intervals worked out by hand: bin = offset of the level + index of the window, for the
    smallest window (16 kb, 128 kb, 1 Mb, 8 Mb, 64 Mb, 512 Mb) that holds [beg, end)"""
    hand = [((0, 1), 4681), ((0, 16384), 4681), ((16383, 16384), 4681), ((16384, 16385), 4682), ((0, 16385), 585), ((16383, 16385), 585),
            ((49052, 49152), 4683), ((49053, 49153), 585), ((131071, 131073), 73), ((131072, 131073), 4689), ((393116, 393216), 4704), ((393117, 393217), 73),
            ((1048575, 1048577), 9), ((1048576, 1048577), 4745), ((3145628, 3145728), 4872), ((3145629, 3145729), 9), ((8388607, 8388609), 1), ((8388608, 8388708), 5193),
            ((8388508, 8388608), 5192), ((8388509, 8388609), 1), ((67108863, 67108865), 0), ((67108764, 67108864), 8776), ((67108864, 67108964), 8777),
            ((67108864, 134217728), 2), ((0, 1 << 29), 0), (((1 << 29) - 1, 1 << 29), 37448), ((-1, 0), 4680)]
    for (beg, end), want in hand:
        assert br.reg2bin(beg, end) == want, (beg, end)
    # and against the other way to say it: the smallest window holding the interval
    rng = np.random.default_rng(5)
    for _ in range(4000):
        sh = int(rng.choice([14, 17, 20, 23, 26]))
        bd = int(rng.integers(1, (1 << 29 - sh))) << sh
        beg = bd - int(rng.integers(0, 3)); end = max(beg + 1, bd + int(rng.integers(-1, 3)))
        want = 0
        for s_, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
            if beg >> s_ == (end - 1) >> s_:
                want = base + (beg >> s_); break
        assert br.reg2bin(beg, end) == want


def test_hand_derived_index():
    """three records on one target of 40,000 bases, one on the next, an unmapped read: bins, chunks, the 16-kb windows"""
    t = "ACGT" * 10000
    cigs = []
    al = np.concatenate([aln(0, 0, 100, 0, 100, 16300, "100M", F_PRIMARY, cigs), aln(1, 0, 50, 0, 50, 10, "50M", F_PRIMARY, cigs),
                         aln(2, 0, 10, 0, 10, 32768, "10M", F_PRIMARY | F_REV, cigs), aln(4, 1, 8, 0, 8, 0, "8M", F_PRIMARY, cigs)])
    reads = [t[16300:16400], t[10:60], be.revcomp(t[32768:32778]), "ACG", "ACGTACGT"]
    s = br.bam_stream(al, np.array(cigs, np.uint32), reads, [t, T20], list("abcde"), ["t0", "t1"], 0, None, "x")
    o = s.offsets + [len(s.raw)]
    assert [r["idx"] for r in s.recs] == [1, 0, 2, 3, None]
    ix = br.bai_reference(s, [len(t), 20])
    assert ix["n_no_coor"] == 1
    assert ix["refs"][0] == dict(bins={4681: [(o[0], o[1])], 585: [(o[1], o[2])], 4683: [(o[2], o[3])]}, linear=[o[0], o[1], o[2]], meta=(o[0], o[3], 3, 0))
    assert ix["refs"][1] == dict(bins={4681: [(o[3], o[4])]}, linear=[o[3]], meta=(o[3], o[4], 1, 0))


def _frame(raw, path, level=6, blk=65280):
    with open(path, "wb") as f:
        for p in range(0, len(raw), blk):
            z = zlib.compressobj(level, zlib.DEFLATED, -15)
            d = z.compress(raw[p:p + blk]) + z.flush()
            f.write(bytes.fromhex("1f8b08040000000000ff0600424302") + b"\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(raw[p:p + blk]), len(raw[p:p + blk])))
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def test_reference_stream_passes_the_validator(tmp_path):
    """the reference stream, framed with zlib, through tools/validate_bam.py (every block, the record chain, the order) and back
    through the reader the GPU test uses"""
    for c in be.sa_cases()[:1] + be.sort_cases(big=False) + be.framing_cases()[:2]:
        s = be.stream_of(c)
        p = str(tmp_path / (c["name"] + ".bam"))
        _frame(s.raw, p)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "validate_bam.py"), p, str(len(s.recs))], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got, blocks = br.read_bgzf(p)
        assert got == s.raw and [b[1] for b in blocks[:-1]] == list(range(0, len(s.raw), 65280))


@pytest.fixture(scope="module")
def cases():
    return be.cases()


def test_every_case_is_valid_and_reaches_its_edge(cases):
    from telr_amd import _lib
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) and len(names) >= 60
    assert set(c["group"] for c in cases) == {"walk", "layout", "sort", "sa", "framing", "deflate"}
    L = _lib.lib()
    missed = []
    for c in cases:
        assert be.check_case(c) is None, (c["name"], be.check_case(c))
        # the library's own record check agrees (host code only)
        ql = np.array([len(r) for r in c["reads"]], np.int32); tl = np.array([len(t) for t in c["targets"]], np.int32)
        al = np.ascontiguousarray(c["alns"]); cg = np.ascontiguousarray(c["cigars"])
        assert L.telr_debug_check_records(al.ctypes.data, len(al), cg.ctypes.data, len(cg), ql.ctypes.data, len(ql), tl.ctypes.data, len(tl), None) == 0, c["name"]
        s = be.stream_of(c)
        assert c["reach"] is not None, c["name"]
        miss = c["reach"](s, c)
        if miss:
            missed.append((c["name"], miss))
        # what every stream owes the format, whatever the case: the records chain to the last byte, NM is blen - mlen
        recs = br.parse_records(s.raw)
        assert len(recs) == len(s.recs) and [r[0] for r in recs] == s.offsets
        for r in s.recs:
            if r["idx"] is not None:
                a = c["alns"][r["idx"]]
                assert r["nm"] == a["blen"] - a["mlen"], (c["name"], r["idx"])
                assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", r["md"])
    assert not missed, missed


def test_long_cigar_placeholder(cases):
    c = next(c for c in cases if c["name"] == "layout_long_cigar")
    s = be.stream_of(c)
    for r, p in zip(s.recs, br.parse_records(s.raw)):
        a = c["alns"][r["idx"]]
        real = [int(x) for x in c["cigars"][int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]]
        t, order = tags_of(p[10])
        if r["n_ops"] > 65535:
            assert cigar_text(p[7]) == "%dS%dN" % (r["l_seq"], a["te"] - a["ts"]) and order[-1] == "CG"
            cg = t["CG"][1]
            assert len(cg) == r["n_ops"] and [x for x in cg if x & 15 != 4] == real and all(x & 15 == 4 for x in cg[:1] + cg[-1:] if x not in real[:1] + real[-1:])
        else:
            assert "CG" not in t and len(p[7]) == r["n_ops"] == 65535
