"""The definition of telr_bam_load (tests/bam_in_ref.py) held to zlib, to hand-derived records and to the project's own BAM encoder
(tests/bam_reference.py), on the CPU; the host twin of the device decoder under the address and undefined-behaviour sanitizers; and
the bindings of the new exports."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import bam_edges
import bam_in_ref as R
import bam_reference as br
from telr_amd import _lib
from telr_amd._abi import F_PRIMARY, F_SECONDARY, F_REV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFLATE = R.deflate_cases()
DEFLATE_ERR = R.deflate_error_cases()


@pytest.mark.parametrize("case", DEFLATE, ids=[c["name"] for c in DEFLATE])
def test_inflater_equals_zlib_and_reaches_its_edge(case):
    out, facts = R.inflate_member(case["comp"], len(case["raw"]))
    assert out == case["raw"] == zlib.decompress(case["comp"], -15)
    assert case["claim"](facts), (case["name"], facts)
    assert R.inflate_one(case["comp"], len(case["raw"]), zlib.crc32(case["raw"])) == case["raw"]


def test_deflate_cases_cover_the_list():
    f = {c["name"]: R.inflate_member(c["comp"])[1] for c in DEFLATE}
    assert set(b for x in f.values() for b in x["btypes"]) == {0, 1, 2}
    assert [len(c["raw"]) for c in DEFLATE if c["name"].startswith("out")] == [0, 1, 65536] and len(DEFLATE[0]["raw"]) == 65280
    assert f["memlevel1"]["blocks"] >= 8 and f["fib15"]["max_code"] == 15 and f["dist32768"]["max_dist"] == 32768
    assert max(x["max_dist"] for k, x in f.items() if k not in ("dist32768",)) <= 32506          # why the hand-written stream exists
    for c in DEFLATE:
        assert len(R.member(c["comp"], c["raw"])) <= 65536


@pytest.mark.parametrize("case", DEFLATE_ERR, ids=[c["name"] for c in DEFLATE_ERR])
def test_inflater_error_codes(case):
    with pytest.raises(R.InflateError) as e:
        R.inflate_one(case["comp"], case["isize"], case["crc"])
    assert e.value.status == case["status"]


def test_fixed_writer_round_trip():
    toks = [65, 66, 67, (3, 3), (258, 1), 0, 255, (4, 9), (258, 200), (257, 2)]
    assert zlib.decompress(R.fixed_deflate(toks), -15) == R.tokens_output(toks)


def test_host_twin_under_sanitizers(tmp_path):
    """tools/ubench/inflate_host.cpp = the device decoder's serial part compiled for the CPU with -fsanitize=address,undefined: every
    deflate case, every error case, and truncated and bit-flipped copies of the good ones"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "inflate_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "ubench", "inflate_host.cpp"), "-lz", "-o", exe])
    R.write_case_file(str(tmp_path / "cases.bin"))
    p = subprocess.run([exe, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "%d cases, 0 failed" % (len(DEFLATE) + len(DEFLATE_ERR)) in p.stdout


def test_framing():
    s = b"0123456789" * 10
    good = R.bgzf(s, [0, 0, 1, 2, 50, 50], extra=b"ZZ\x01\0q")
    raw, n, no_eof = R.inflate_file(good)
    assert raw == s and n == 8 and no_eof == 0
    assert R.inflate_file(good[:-28])[2] == 1
    for bad, blk in ((good[:-3], 7), (good + b"x" * 40, 8), (good[:30] + b"\1" + good[31:], 0)):
        with pytest.raises(R.BamInError) as e:
            R.inflate_file(bad)
        assert e.value.code == R.E_ARG and "block %d" % blk in e.value.text


def hand_file():
    head = R.bam_header(["r"], [1000])
    recs = [
        R.bam_record("a", 0, 0, 10, 40, R.ops_of("2S5=2X1I3M2D0I4N6M3S"), "ACGTACGTACGTACGTACGTAC", bytes(range(22)),
                     R.tag_int("NM", "C", 4) + R.tag_int("AS", "s", -5) + R.tag_int("cm", "c", 7) + R.tag_int("s1", "S", 50000) + R.tag_int("s2", "I", 3)),
        R.bam_record("a", 0x110, 0, 500, 0, R.ops_of("22M"), "", None),
        R.bam_record("b", 0x10, 0, 100, 3, R.ops_of("3H2S4M1H"), "ACGTAC", None),
        R.bam_record("c", 0x10, 0, 200, 9, R.ops_of("1S4M2S"), "ACGTNAC", bytes([1, 2, 3, 4, 5, 6, 7])),
        R.bam_record("d", 4, -1, -1, 0, (), "ACG", bytes([9, 9, 9])),
    ]
    return R.bgzf(head + b"".join(recs), [3, 40, 41])


def test_hand_derived_records():
    L = R.load(hand_file(), keep_qual=True)
    assert L.tnames == ["r"] and L.tlens == [1000]
    assert L.qnames == ["a", "c", "d"] and L.seqs == ["ACGTACGTACGTACGTACGTAC", "GTNACGT", "ACG"]
    assert L.quals == [bytes(range(22)), bytes([7, 6, 5, 4, 3, 2, 1]), bytes([9, 9, 9])]          # ("b" is not sequence-bearing: its 0xff does not count)
    a = L.alns
    assert len(a) == 3
    want = [dict(qid=0, tid=0, tlen=1000, qlen=22, qs=2, qe=19, ts=10, te=32, blen=23, mlen=19, dp_score=-5, cnt=7, score=50000, subsc=3,
                 mapq=40, flags=F_PRIMARY, parent=0, n_cigar=5, cigar_off=0, n_sub=0, n_ambi=0),
            dict(qid=0, tid=0, tlen=1000, qlen=22, qs=0, qe=22, ts=500, te=522, blen=22, mlen=22, dp_score=0, cnt=0, score=0, subsc=0,
                 mapq=0, flags=F_SECONDARY | F_REV, parent=0, n_cigar=1, cigar_off=5, n_sub=0, n_ambi=0),
            dict(qid=1, tid=0, tlen=1000, qlen=7, qs=2, qe=6, ts=200, te=204, blen=4, mlen=4, dp_score=0, cnt=0, score=0, subsc=0,
                 mapq=9, flags=F_PRIMARY | F_REV, parent=0, n_cigar=1, cigar_off=6, n_sub=0, n_ambi=0)]
    for i, w in enumerate(want):
        for k, v in w.items():
            assert int(a[i][k]) == v, (i, k, int(a[i][k]), v)
    assert [int(c) for c in L.cigars] == R.ops_of("7M1I3M6D6M") + R.ops_of("22M") + R.ops_of("4M")
    assert L.counters == dict(members=5, records=5, mapped=4, kept=3, reads=3, orphans=1, len_mismatch=0, no_cigar=0, no_eof=0)


def test_hand_derived_qualities():
    head = R.bam_header(["r"], [50])
    recs = [R.bam_record("f", 0, 0, 1, 1, R.ops_of("3M"), "ACG", bytes([1, 2, 3])), R.bam_record("r", 0x10, 0, 1, 1, R.ops_of("3M"), "ACG", bytes([4, 5, 6]))]
    L = R.load(R.bgzf(head + b"".join(recs)), keep_qual=True)
    assert L.quals == [bytes([1, 2, 3]), bytes([6, 5, 4])] and L.seqs == ["ACG", "CGT"]
    assert R.load(R.bgzf(head + b"".join(recs)), keep_qual=False).quals is None
    w2, wn = R.packed_words(["ACGTN", "T" * 65])
    assert len(w2) == (64 + 128) // 16 and len(wn) == 6 and int(w2[0]) == 0b11100100 and int(wn[0]) == 16 and int(w2[4]) == 0xffffffff and int(w2[8]) == 3


def test_record_and_error_cases_cover_the_list():
    cs = {c["name"]: c for c in R.record_cases()}
    L = R.load(cs["foreign_cut"]["data"], True)
    assert L.quals is not None and R.load(cs["foreign_one_qual_absent"]["data"], True).quals is None
    assert L.counters["no_eof"] == 0 and R.load(cs["foreign_no_eof_extra"]["data"], True).counters["no_eof"] == 1
    assert L.counters["orphans"] >= 1 and L.counters["len_mismatch"] >= 1 and L.counters["no_cigar"] >= 1 and L.counters["records"] <= 200
    assert max(int(x) for x in L.alns["n_cigar"]) > 65535
    assert set(len(s) for s in L.seqs) >= {1, 15, 16, 17, 63, 64, 65}
    assert any(int(a["flags"]) & 4 for a in L.alns) and any(int(a["flags"]) & 2 for a in L.alns)          # a supplementary and a secondary are kept
    assert sum(1 for m in R.hop(cs["foreign_cut"]["data"]) if m[2] == 1) >= 2 and sum(1 for m in R.hop(cs["foreign_cut"]["data"]) if m[2] == 0) >= 3
    for c in R.error_cases():
        with pytest.raises(R.BamInError) as e:
            R.load(c["data"])
        assert e.value.code == c["code"] and c["text"] in e.value.text, (c["name"], e.value.text)


# A file in which two reads share a QNAME cannot be inverted: the definition (like bam2fasta) makes ONE read of them.  Five layout /
# deflate cases of bam_edges name their reads that way on purpose (name-length edges); the inversion is stated on the others.
ALL_EDGE = bam_edges.cases(big=False)
EDGE = [c for c in ALL_EDGE if len(set(c["qnames"])) == len(c["qnames"])]


def test_inversion_covers_nearly_every_edge_case():
    assert len(EDGE) >= len(ALL_EDGE) - 5 and len(EDGE) >= 40


@pytest.mark.parametrize("case", EDGE, ids=[c["name"] for c in EDGE])
def test_definition_inverts_the_plain_encoder(case):
    """bam_reference.bam_stream of a bam_edges case, read back by the definition: the input records field for field -- modulo the read
    numbering (matched by name), `parent`, `n_sub` and `subsc` of secondaries, which the file does not hold"""
    c = case
    s = bam_edges.stream_of(c)
    L = R.load_stream(s.raw)
    assert L.counters["orphans"] == 0 and L.counters["len_mismatch"] == 0 and L.counters["no_cigar"] == 0
    assert L.tnames == list(c["tnames"]) and L.tlens == [len(t) for t in c["targets"]]
    qid_in = {n: i for i, n in enumerate(c["qnames"])}
    assert len(set(c["qnames"])) == len(c["qnames"])
    for q, n in enumerate(L.qnames):
        assert L.seqs[q] == br.norm(c["reads"][qid_in[n]])
    fields = ("tid", "tlen", "qlen", "qs", "qe", "ts", "te", "mlen", "blen", "score", "dp_score", "cnt", "mapq", "flags")

    def key(a, cig, qid):
        sec = bool(int(a["flags"]) & F_SECONDARY)
        return (qid,) + tuple(int(a[f]) for f in fields) + (0 if sec else int(a["subsc"]),) + tuple(int(x) for x in cig[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])])
    got = sorted(key(a, L.cigars, qid_in[L.qnames[int(a["qid"])]]) for a in L.alns)
    want = sorted(key(a, c["cigars"], int(a["qid"])) for a in c["alns"])
    assert got == want
    assert L.counters["kept"] == len(c["alns"]) == L.counters["mapped"]


NEW_EXPORTS = ["telr_bam_load", "telr_bam_in_free", "telr_bam_in_target_count", "telr_bam_in_target_names", "telr_bam_in_target_lens",
               "telr_bam_in_read_count", "telr_bam_in_read_names", "telr_bam_in_read_lens", "telr_bam_in_seqset", "telr_bam_in_result",
               "telr_bam_in_detach_seqset", "telr_bam_in_detach_result", "telr_bam_in_counters", "telr_bam_in_ascii", "telr_bam_in_phase_ms"]


def test_abi_binds_every_new_export():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "telr_hip.h")).read()
    for n in NEW_EXPORTS:
        assert n in _lib.EXPORTS and (n + "(") in header
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
    from telr_amd.aligner import Engine, BamInput
    assert callable(Engine.load_bam) and BamInput.COUNTERS == R.COUNTERS
    from telr_amd import telr_alignment
    assert callable(telr_alignment.bam_input)
