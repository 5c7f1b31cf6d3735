"""The definition of telr_reads_load in plain Python (tests/reads_in_ref.py) against hand-derived answers, against fasta.read_fasta on
the cases both accept, and against bam_in_ref.packed_words; and the shared per-record / per-word functions of
telr_amd/csrc/reads_text_core.h, compiled for the CPU with the sanitizers, against the definition.  No device."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_in_ref as B
import reads_in_ref as R
from telr_amd import _lib, fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()
TEXT_ERRORS = R.text_error_cases()


def test_hand_derived_fastq():
    p = R.parse(b"@a b\tc\r\nACGTN\r\n+a\r\n!~II@\r\n@\nacgu\n+\n+@!~", True)
    assert p.names == ["a", ""] and p.seqs == [b"ACGTN", b"acgu"] and p.quals == [bytes([0, 93, 40, 40, 31]), bytes([10, 31, 0, 93])]
    assert p.fastq == 1 and p.lines == 8
    assert R.parse(b"@a\nAC\n+\nII\r", True).seqs == [b"AC"] and R.parse(b"@a\nAC\n+\nII\r", True).quals == [bytes([40, 40])]
    assert R.parse(b"@a\tx\n\n+\n\n").names == ["a"] and R.parse(b"@a\n\n+\n\n").seqs == [b""]
    assert R.parse(b"") .names == [] and R.parse(b"").lines == 0


def test_hand_derived_fasta():
    p = R.parse(b">x 1\nAC\r\n\nGT\n>y\n>\tz\nNN", True)
    assert p.names == ["x", "y", ""] and p.seqs == [b"ACGT", b"", b"NN"] and p.quals is None and p.fastq == 0 and p.lines == 7
    assert R.parse(b">").names == [""] and R.parse(b">").seqs == [b""] and R.parse(b">\n").lines == 1
    assert R.parse(b">a\nA C\n").seqs == [b"A C"]          # a space inside a sequence is a base like any other: masked


def test_hand_derived_refusals():
    assert R.parse(b"ACGT\n") == (R.E_ARG, R.W + R.NO_KIND)
    assert R.parse(b"@a\nAC\n+\nII\n\n") == (R.E_ARG, R.W + "record 1: " + R.NO_AT)
    assert R.parse(b"@a\nAC\n+\nII\n@b\n") == (R.E_ARG, R.W + "record 1: " + R.SHORT)
    assert R.parse(b"@a\nAC\nGT\n+\nIIII\n") == (R.E_ARG, R.W + "record 0: " + R.NO_PLUS)
    assert R.parse(b"@a\nAC\n+\nI\n") == (R.E_ARG, R.W + "record 0: " + R.LEN)
    assert R.parse(b"@a\nAC\n+\nI \n", True) == (R.E_ARG, R.W + "record 0: " + R.QUAL) and R.parse(b"@a\nAC\n+\nI \n", False).seqs == [b"AC"]
    assert R.parse(b"@a\nAC\n+\nI\x7f\n", True)[0] == R.E_ARG


@pytest.mark.parametrize("e", TEXT_ERRORS, ids=[e["name"] for e in TEXT_ERRORS])
def test_text_error_cases(e):
    p = R.parse(e["data"], e["keep_qual"])
    if e["code"] == 0:
        assert not isinstance(p, tuple) and len(p.seqs) == 5
    else:
        assert p == (e["code"], R.W + e["text"])


def test_cases_cover_the_list():
    by = {c["name"]: c for c in CASES}
    lens = set(len(s) for s in R.parse(by["fq_lengths"]["text"]).seqs)
    assert lens == set(R.LENGTHS) and set(len(n) for n in R.parse(by["fq_names_0_17"]["text"]).names) == set(range(18))
    starts = set()
    t = by["fq_names_0_17"]["text"]
    p = 0
    for ln in t.split(b"\n")[:-1:1]:
        starts.add(p % 16); p += len(ln) + 1
    assert len(starts) == 16
    for n in R.COUNTS:
        assert len(R.parse(by["fq_count_%d" % n]["text"]).seqs) == n
    assert max(len(s) for s in R.parse(by["fq_long_70001"]["text"]).seqs) == 70001
    assert b"\r\n" in by["fq_crlf_mixed"]["text"] and by["fq_crlf_mixed"]["text"].count(b"\n") > by["fq_crlf_mixed"]["text"].count(b"\r\n")
    assert not by["fq_no_last_lf"]["text"].endswith(b"\n") and by["fq_last_lone_cr"]["text"].endswith(b"\r")
    for w in (1, 60, 64, 70):
        assert set(len(s) for s in R.parse(by["fa_width_%d" % w]["text"]).seqs) == set(R.LENGTHS)
    assert [len(s) for s in R.parse(by["fa_header_only"]["text"]).seqs] == [0, 12, 0, 4, 0]
    assert R.parse(by["fa_empty_lines"]["text"]).seqs == [b"ACGTAC", b"", b"TTTTGG"]
    names = set(e["name"] for e in TEXT_ERRORS) | set(e["name"] for e in R.file_error_cases())
    assert {"first_byte", "no_at_0", "no_at_mid", "no_at_last", "no_plus", "seq_longer", "seq_shorter", "trailing_1", "trailing_2", "trailing_3",
            "empty_line_mid", "trailing_empty_line", "qual_32", "qual_127", "bgzf_flipped_bit", "gzip_flipped_bit", "bgzf_wrong_crc", "gzip_wrong_crc",
            "bgzf_wrong_isize", "gzip_wrong_isize", "bgzf_truncated", "gzip_truncated"} <= names


STRAY = {"fq_alphabet", "fa_alphabet", "fq_names_0_17", "fa_one_line_lf", "fa_one_line"}          # white space inside a line, or a name that read_fasta cannot split


@pytest.mark.parametrize("c", [c for c in CASES if c["name"] not in STRAY and c["text"]], ids=lambda c: c["name"])
def test_definition_agrees_with_read_fasta(tmp_path, c):
    """the Python reader that the loader replaces accepts these files and reads the same names, bases and quality lines"""
    p = tmp_path / "x.fq.gz"
    p.write_bytes(gzip.compress(c["text"], 1))
    names, seqs, quals = fasta.read_fasta(str(p), with_qual=True)
    d = R.parse(c["text"], True)
    assert names == d.names and [s.encode("latin-1") for s in seqs] == d.seqs
    if d.fastq:
        assert [q.encode("latin-1") for q in quals] == [bytes(x + 33 for x in q) for q in d.quals]
    else:
        assert quals is None and d.quals is None


def test_norm_and_packed_words():
    assert R.norm(b"acgtuUNn*R \x80") == "ACGTTTNNNNNN"
    w2, wn = B.packed_words([R.norm(b"ACGTN"), R.norm(b"T" * 65)])
    assert len(w2) == (64 + 128) // 16 and int(w2[0]) == 0b0011100100 and int(wn[0]) == 16 and int(w2[4]) == 0xffffffff and int(w2[8]) == 3
    assert R.qual_layout([b"AC", b""], [b"\x01\x02", b""]) == b"\x01\x02" + bytes(62)


def test_containers():
    text = CASES[0]["text"]
    for kind in R.CONTAINERS:
        data = R.container(kind, text, [10, 10, 200])
        cont, got, members, no_eof = R.inflate_any(data)
        assert got == text and cont == R.want_container(kind, text) and no_eof == 0
        assert members == {"plain": 0, "gz6": 1, "gz0": 1, "gz3m": 3, "bgzf": 5}[kind]
    assert R.inflate_any(b"") == (R.PLAIN, b"", 0, 0) and R.inflate_any(B.EOF_MARKER) == (R.BGZF, b"", 1, 0)
    assert R.inflate_any(R.container("bgzf", text, eof=False))[3] == 1
    data, big = R.big_member_file()
    assert R.inflate_any(data) == (R.GZIP, big, 2, 0)
    for e in R.file_error_cases():
        with pytest.raises(R.ReadsInError) as x:
            R.load(e["data"])
        assert x.value.code == R.E_ARG and x.value.text.startswith(R.W)
        if e["container"] == R.BGZF:
            assert "block 1: " in x.value.text
        elif e["container"] == R.GZIP:
            assert x.value.text.startswith(R.W + "gzip: ")


def test_shared_functions_under_sanitizers(tmp_path):
    """tools/ubench/reads_text_host.cpp = the kernels' per-record and per-word functions compiled for the CPU with
    -fsanitize=address,undefined, run over every case and every text fault: the text in a block of exactly text + 64 bytes, the outputs in
    blocks of exactly the layout's size"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "reads_text_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "ubench", "reads_text_host.cpp"), "-o", exe])
    n = R.write_case_file(str(tmp_path / "cases.bin"))
    p = subprocess.run([exe, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert "%d cases, 0 failed" % n in p.stdout


NEW_EXPORTS = ["telr_reads_load", "telr_reads_in_free", "telr_reads_in_count", "telr_reads_in_names", "telr_reads_in_lens", "telr_reads_in_seqset",
               "telr_reads_in_detach_seqset", "telr_reads_in_counters", "telr_reads_in_chunk_info", "telr_reads_in_phase_ms"]


def test_abi_binds_every_new_export():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "telr_hip.h")).read()
    for n in NEW_EXPORTS:
        assert n in _lib.EXPORTS and (n + "(") in header
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
    from telr_amd.aligner import Engine, ReadsInput
    assert callable(Engine.load_reads) and ReadsInput.COUNTERS == R.COUNTERS and callable(fasta.load_reads)
