"""telr_reads_load on the device == its definition in plain Python (tests/reads_in_ref.py), for every case x container x chunk_bytes:
names, lengths, the set's 2-bit and mask words (against bam_in_ref.packed_words AND against Engine.seqset of the same reads), the Phred
bytes, has_qual and the counters -- integers and bytes, no tolerance; a second load gives the same bytes; a refused file gives the
definition's code and text at every chunk_bytes."""
import numpy as np
import pytest

import bam_in_ref as B
import reads_in_ref as R
from telr_amd._lib import TelrError

pytestmark = pytest.mark.gpu

CASES = R.cases()
TEXT_ERRORS = R.text_error_cases()
FILE_ERRORS = R.file_error_cases()
CHUNKS = (0, 1, 100, 65536)
_REF = {}


def definition(engine, c):
    """the definition's answer for a case, and what Engine.seqset makes of the same reads: computed once"""
    if c["name"] not in _REF:
        p = R.parse(c["text"], True)
        e2, en = B.packed_words([R.norm(s) for s in p.seqs])
        s = engine.seqset(list(p.seqs))
        if p.seqs:
            h2, hn = (x.cpu().numpy().view(np.uint32).copy() for x in s.packed())
        else:
            h2, hn = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        s.free()
        q = np.frombuffer(R.qual_layout(p.seqs, p.quals), np.uint8) if p.quals is not None else None
        _REF[c["name"]] = (p, e2, en, h2, hn, q)
    return _REF[c["name"]]


def load_and_check(engine, path, c, kind, chunk, members, no_eof=0):
    """-> the loaded set's bytes"""
    p, e2, en, h2, hn, q = definition(engine, c)
    ri = engine.load_reads(str(path), keep_qual=True, chunk_bytes=chunk)
    try:
        tag = "%s %s chunk_bytes %d" % (c["name"], kind, chunk)
        assert ri.qnames == p.names, tag
        np.testing.assert_array_equal(ri.read_set.len, [len(s) for s in p.seqs], err_msg=tag)
        if ri.read_set.n:
            w2, wn = (x.cpu().numpy().view(np.uint32) for x in ri.read_set.packed())
        else:
            w2, wn = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        np.testing.assert_array_equal(w2, e2, err_msg=tag); np.testing.assert_array_equal(wn, en, err_msg=tag)
        np.testing.assert_array_equal(w2, h2, err_msg=tag); np.testing.assert_array_equal(wn, hn, err_msg=tag)
        assert ri.read_set.has_qual == (q is not None), tag
        got_q = b""
        if q is not None:
            got = np.zeros(max(len(q), 1), np.uint8)
            assert engine.L.telr_debug_seqset_qual(ri.read_set.h, got.ctypes.data, len(q)) == len(q), tag
            np.testing.assert_array_equal(got[:len(q)], q, err_msg=tag)
            got_q = got[:len(q)].tobytes()
        want = dict(container=R.want_container(kind, c["text"]), fastq=p.fastq, members=members, text_bytes=len(c["text"]), lines=p.lines,
                    records=len(p.seqs), bases=sum(len(s) for s in p.seqs), no_eof=no_eof)
        assert ri.counters == want, tag
        assert ri.n_bases == want["bases"] and ri.container == ("plain", "gzip", "bgzf")[want["container"]]
        assert ri.kind == (None if not c["text"] else "fastq" if p.fastq else "fasta")
        assert ri.chunk_info["chunks"] >= 1 and ri.phase_ms["total"] > 0
        return w2.tobytes(), wn.tobytes(), got_q, tuple(ri.qnames)
    finally:
        ri.read_set.free(); ri.free()


@pytest.mark.parametrize("kind", R.CONTAINERS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case(engine, tmp_path, case, kind):
    c = case
    data = R.container(kind, c["text"], c["cuts"], eof=c["eof"])
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(data)
    members = {"plain": 0, "gz6": 1, "gz0": 1, "gz3m": 3}.get(kind)
    if kind == "bgzf":
        members = len(B.hop(data))
    no_eof = 1 if kind == "bgzf" and not c["eof"] else 0
    runs = [load_and_check(engine, path, c, kind, chunk, members, no_eof) for chunk in CHUNKS + c["chunks"]]
    runs.append(load_and_check(engine, path, c, kind, CHUNKS[0], members, no_eof))          # a second load at the first size
    assert all(r == runs[0] for r in runs)


def test_chunks_and_carry(engine, tmp_path):
    """chunk_bytes 1 puts every BGZF member into a chunk of its own; a record that spans chunks makes the carry grow beyond a slot's room"""
    by = {c["name"]: c for c in CASES}
    c = by["seam_fq_lf"]
    p = tmp_path / "a.gz"
    p.write_bytes(R.container("bgzf", c["text"], c["cuts"]))
    ri = engine.load_reads(str(p), chunk_bytes=1)
    isize = [m[2] for m in B.hop(p.read_bytes())]
    assert ri.chunk_info["chunks"] == len(engine.bam_chunk_plan(isize, 1)) >= sum(1 for x in isize if x) and ri.chunk_info["largest_carry"] > 0
    ri.read_set.free(); ri.free()
    c = by["fq_long_70001"]
    for kind, chunk in (("bgzf", 1), ("plain", 65536), ("gz6", 65536)):
        p.write_bytes(R.container(kind, c["text"], list(range(30000, len(c["text"]), 30000))))
        ri = engine.load_reads(str(p), keep_qual=True, chunk_bytes=chunk)
        assert ri.chunk_info["chunks"] >= 3 and ri.chunk_info["largest_carry"] > 65536 and ri.chunk_info["largest_buffer"] > ri.chunk_info["largest_carry"]
        assert ri.chunk_info["peak_transient_bytes"] >= 2 * ri.chunk_info["largest_buffer"]
        ri.read_set.free(); ri.free()


def test_empty_file_and_eof_marker_alone(engine, tmp_path):
    p = tmp_path / "e.gz"
    for data, cont, members in ((b"", 0, 0), (B.EOF_MARKER, 2, 1)):
        p.write_bytes(data)
        for chunk in CHUNKS:
            ri = engine.load_reads(str(p), keep_qual=True, chunk_bytes=chunk)
            assert ri.qnames == [] and ri.read_set.n == 0 and ri.kind is None and not ri.read_set.has_qual
            assert ri.counters == dict(container=cont, fastq=0, members=members, text_bytes=0, lines=0, records=0, bases=0, no_eof=0)
            ri.read_set.free(); ri.free()


def test_fasta_with_keep_qual_has_no_qualities(engine, tmp_path):
    p = tmp_path / "f.fa"
    p.write_bytes(b">a\nACGT\n")
    ri = engine.load_reads(str(p), keep_qual=True)
    assert not ri.read_set.has_qual and ri.kind == "fasta"
    ri.read_set.free(); ri.free()
    p.write_bytes(b"@a\nACGT\n+\nIIII\n")
    ri = engine.load_reads(str(p), keep_qual=False)
    assert not ri.read_set.has_qual and ri.kind == "fastq"
    ri.read_set.free(); ri.free()


def refused(engine, path, keep_qual, chunk):
    with pytest.raises(TelrError) as x:
        engine.load_reads(str(path), keep_qual=keep_qual, chunk_bytes=chunk)
    return x.value.code, engine.L.telr_last_error(engine.h).decode("latin-1")


@pytest.mark.parametrize("kind", R.CONTAINERS)
@pytest.mark.parametrize("e", TEXT_ERRORS, ids=[e["name"] for e in TEXT_ERRORS])
def test_text_fault(engine, tmp_path, e, kind):
    """one fault: the definition's code and text at every chunk_bytes, in every container"""
    path = tmp_path / "bad.fq.gz"
    path.write_bytes(R.container(kind, e["data"], [50, 333]))
    for chunk in CHUNKS + (37,):
        if e["code"] == 0:
            ri = engine.load_reads(str(path), keep_qual=e["keep_qual"], chunk_bytes=chunk)
            assert ri.read_set.n == 5 and not ri.read_set.has_qual
            ri.read_set.free(); ri.free()
            continue
        want = R.W + (R.NO_CONTAINER if kind == "plain" and e["text"] == R.NO_KIND else e["text"])
        assert refused(engine, path, e["keep_qual"], chunk) == (e["code"], want), (e["name"], kind, chunk)


@pytest.mark.parametrize("e", FILE_ERRORS, ids=[e["name"] for e in FILE_ERRORS])
def test_file_fault(engine, tmp_path, e):
    """a fault of the container: the definition's code and text (zlib's own: the code and the "gzip:" prefix), at every chunk_bytes"""
    path = tmp_path / "bad.gz"
    path.write_bytes(e["data"])
    with pytest.raises(R.ReadsInError) as x:
        R.load(e["data"])
    for chunk in CHUNKS:
        code, text = refused(engine, path, False, chunk)
        assert code == x.value.code
        if e["container"] == R.GZIP:
            assert text.startswith(R.W + "gzip: ")
        else:
            assert text == x.value.text


def test_member_above_65536_goes_the_gzip_way(engine, tmp_path):
    data, text = R.big_member_file()
    path = tmp_path / "big.gz"
    path.write_bytes(data)
    d = R.load(data, True)
    assert d.counters["container"] == R.GZIP
    for chunk in CHUNKS:
        ri = engine.load_reads(str(path), keep_qual=True, chunk_bytes=chunk)
        assert ri.counters == d.counters and ri.qnames == d.names and ri.container == "gzip"
        np.testing.assert_array_equal(ri.read_set.len, [len(s) for s in d.seqs])
        ri.read_set.free(); ri.free()


def test_refusals_of_the_call(engine, tmp_path):
    p = tmp_path / "x.fa"
    p.write_bytes(b">a\nAC\n")
    assert refused(engine, p, False, -1)[0] == R.E_ARG
    assert refused(engine, tmp_path / "missing.fq.gz", False, 0)[0] == -6
    from telr_amd import fasta
    assert fasta.load_reads(str(p), engine).qnames == ["a"]
    p.write_bytes(b"@a\nAC\n+\nII\n\n")
    assert fasta.load_reads(str(p), engine) is None                     # a grammar refusal: the caller's fallback
    with pytest.raises(TelrError):
        fasta.load_reads(str(tmp_path / "missing.fq.gz"), engine)     # anything else is raised
