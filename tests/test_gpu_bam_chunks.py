"""telr_bam_load_chunked on the device == the whole-file load == the definition (tests/bam_in_ref.py), field for field, at chunk sizes that
put a chunk seam at every place a load in chunks can go wrong (tests/bam_chunks_ref.py; tests/test_bam_chunks_ref.py holds the cases to
what they claim): the record cases, the seam cases, the error cases, the memory bound and the `telr` command."""
import os

import numpy as np
import pytest

import bam_in_ref as R
import bam_chunks_ref as K
from test_gpu_bam_in import loaded_equals
from telr_amd import aligner, telr
from telr_amd._lib import TelrError

pytestmark = pytest.mark.gpu

RECORD = R.record_cases()
SEAMS = K.seam_cases()
ERRORS = R.error_cases()
ONE_CHUNK = 1 << 40
_REF = {}


def definition(c):
    """the definition's answer for a case, computed once"""
    if c["name"] not in _REF:
        _REF[c["name"]] = R.load(c["data"], c["keep_qual"])
    return _REF[c["name"]]


def isizes(data):
    return [m[2] for m in R.hop(data)]


def two_chunk_bytes(isize):
    """the largest chunk_bytes that cuts these members into exactly two chunks"""
    sums = np.cumsum(isize)
    for c in sorted({int(s) - d for s in sums for d in (0, 1)}, reverse=True):
        if c >= 1 and len(K.plan(isize, c)) == 2:
            return c
    raise AssertionError("no chunk size gives two chunks")


def snapshot(engine, bi):
    """everything a load leaves, as bytes"""
    m = bi.map_result()
    out = [bi.tnames, [int(x) for x in bi.tlens], bi.qnames, bi.counters, m.alns.tobytes(), m.cigars.tobytes(), bi.read_set.len.tobytes(), bi.read_set.has_qual]
    if bi.read_set.n:
        w2, wn = bi.read_set.packed()
        out += [w2.cpu().numpy().tobytes(), wn.cpu().numpy().tobytes()]
    if bi.read_set.has_qual:
        tot = int(((bi.read_set.len.astype(np.int64) + 63) // 64 * 64).sum())
        q = np.zeros(tot, np.uint8)
        assert engine.L.telr_debug_seqset_qual(bi.read_set.h, q.ctypes.data, tot) == tot
        out.append(q.tobytes())
    return out


@pytest.fixture(scope="module")
def whole(engine, tmp_path_factory):
    """case name -> (path, snapshot of the whole-file load), loaded once"""
    d = tmp_path_factory.mktemp("bam_chunks")
    got = {}

    def of(case):
        if case["name"] not in got:
            p = d / (case["name"] + ".bam")
            p.write_bytes(case["data"])
            bi = engine.load_bam(str(p), keep_qual=case["keep_qual"])
            assert bi.chunk_info == dict(chunks=0, passes=0, largest_buffer=0, largest_carry=0)
            got[case["name"]] = (str(p), snapshot(engine, bi))
            bi.free()
        return got[case["name"]]
    return of


def load_and_compare(engine, whole, case, c):
    path, snap = whole(case)
    bi = engine.load_bam(path, keep_qual=case["keep_qual"], chunk_bytes=c)
    loaded_equals(engine, bi, definition(case))
    assert snapshot(engine, bi) == snap
    info = bi.chunk_info
    bi.free()
    isz = isizes(case["data"])
    first = K.plan(isz, c) + [len(isz)]
    assert info["chunks"] == len(first) - 1
    assert info["passes"] == (2 if definition(case).qnames or len(definition(case).alns) else 1)
    payload = max(sum(isz[a:b]) for a, b in zip(first, first[1:]))
    assert payload + info["largest_carry"] <= info["largest_buffer"] <= payload + info["largest_carry"] + 65536      # a slot: carry room + members
    return info


# ---- 1. chunk sizes over the record cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1", "65536", "two_chunks", "one_chunk"])
@pytest.mark.parametrize("case", RECORD, ids=[c["name"] for c in RECORD])
def test_record_case_in_chunks(engine, whole, case, size):
    isz = isizes(case["data"])
    c = {"1": 1, "65536": 65536, "two_chunks": two_chunk_bytes(isz), "one_chunk": sum(isz) + 1}[size]
    info = load_and_compare(engine, whole, case, c)
    if size == "two_chunks":
        assert info["chunks"] == 2
    if size == "one_chunk":
        assert info["chunks"] == 1 and info["largest_carry"] == 0
    if size == "1" and case["name"] == "foreign_cut":
        assert info["largest_carry"] > 3 * 40000                  # the CG record spans more than three members: the carry grew over them


# ---- 2. seam cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 65536])
@pytest.mark.parametrize("case", SEAMS, ids=[c["name"] for c in SEAMS])
def test_seam_case(engine, whole, case, c):
    info = load_and_compare(engine, whole, case, c)
    if c == 1 and case["seam"]:
        assert info["largest_carry"] >= case["seam"][1]            # the record's bytes before the seam were carried
    if case["name"] == "long_header":
        assert info["largest_carry"] > 65536                       # the header outgrew a chunk and a slot's first carry room
    if case["name"] == "one_ff_in_the_last_chunk":
        assert definition(case).quals is None


def test_same_bytes_on_two_chunked_runs(engine, whole):
    case = RECORD[0]
    path, snap = whole(case)
    for _ in range(2):
        bi = engine.load_bam(path, keep_qual=case["keep_qual"], chunk_bytes=1)
        assert snapshot(engine, bi) == snap
        bi.free()


def test_engine_chosen_sizes(engine, whole):
    """chunk_bytes 0: the engine's own size (one chunk for a small file); BAM_CHUNK_FIT: the whole-file load when the file fits"""
    case = RECORD[0]
    path, snap = whole(case)
    bi = engine.load_bam(path, keep_qual=case["keep_qual"], chunk_bytes=0)
    assert snapshot(engine, bi) == snap and bi.chunk_info["chunks"] == 1 and bi.chunk_info["passes"] == 2
    bi.free()
    bi = engine.load_bam(path, keep_qual=case["keep_qual"], chunk_bytes=aligner.BAM_CHUNK_FIT)
    assert snapshot(engine, bi) == snap and bi.chunk_info["chunks"] == 0
    bi.free()
    with pytest.raises(TelrError) as e:
        engine.load_bam(path, chunk_bytes=-2)
    assert e.value.code == R.E_ARG


# ---- 3. error cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, ONE_CHUNK])
@pytest.mark.parametrize("case", ERRORS, ids=[c["name"] for c in ERRORS])
def test_error_case_in_chunks(engine, whole, tmp_path, case, c):
    """one fault per file: the whole-file load's code and text; the same engine loads a good file in chunks afterwards"""
    p = tmp_path / "bad.bam"
    p.write_bytes(case["data"])
    with pytest.raises(TelrError) as w:
        engine.load_bam(str(p))
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(p), chunk_bytes=c)
    assert e.value.code == case["code"] and case["text"] in str(e.value), str(e.value)
    assert str(e.value) == str(w.value)
    with pytest.raises(R.BamInError) as d:
        R.load(case["data"])
    assert d.value.text in str(e.value)                          # the definition's own words
    good = RECORD[-2]
    path, snap = whole(good)
    bi = engine.load_bam(path, keep_qual=good["keep_qual"], chunk_bytes=c)
    assert snapshot(engine, bi) == snap
    bi.free()


def test_quality_above_93_in_the_second_pass(engine, tmp_path):
    head, recs = R.record_stream()
    bad = R.bam_record("q94", 0, 0, 5, 9, R.ops_of("10M"), "A" * 10, bytes([1, 2, 94, 3, 4, 5, 6, 7, 8, 9]))
    rs = recs[:7] + [bad] + recs[8:10]
    st = K.record_starts(head, rs)
    p = tmp_path / "q.bam"
    p.write_bytes(R.bgzf(head + b"".join(rs), [st[3], st[7] + 50, st[9]]))
    seen = []
    for c in (None, 1, ONE_CHUNK):
        with pytest.raises(TelrError) as e:
            engine.load_bam(str(p), keep_qual=True, chunk_bytes=c)
        assert e.value.code == R.E_ARG and "record 7: a base quality above 93" in str(e.value)
        seen.append(str(e.value))
    assert seen[0] == seen[1] == seen[2]
    bi = engine.load_bam(str(p), keep_qual=False, chunk_bytes=1)          # without the qualities the file is a good one
    assert bi.counters["records"] == len(rs)
    bi.free()


def test_empty_file_in_chunks(engine, tmp_path):
    p = tmp_path / "empty.bam"
    p.write_bytes(b"")
    with pytest.raises(TelrError) as w:
        engine.load_bam(str(p))
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(p), chunk_bytes=1)
    assert str(e.value) == str(w.value) and "header" in str(e.value)


@pytest.mark.parametrize("data", [b"", R.EOF_MARKER], ids=["zero_bytes", "eof_marker_alone"])
def test_no_member_with_a_byte(engine, tmp_path, data):
    """no chunk to inflate, or one of no bytes: the definition's header error, the same words on both entry points"""
    with pytest.raises(R.BamInError) as d:
        R.load(data)
    assert d.value.code == R.E_ARG and d.value.text == "header: magic runs past the stream"
    p = tmp_path / "none.bam"
    p.write_bytes(data)
    seen = []
    for c in (None, 1):
        with pytest.raises(TelrError) as e:
            engine.load_bam(str(p), chunk_bytes=c)
        assert e.value.code == d.value.code and d.value.text in str(e.value), str(e.value)
        seen.append(str(e.value))
    assert seen[0] == seen[1]


def test_one_chunk_second_pass_reuses_its_slot(engine, whole):
    """one chunk, something kept, qualities on: the second pass reads the chunk where the first left it, on every way to one chunk; a
    load in two slots right behind it on the same engine sees nothing of that slot's state"""
    case = RECORD[0]
    ref = definition(case)
    assert case["keep_qual"] and ref.quals is not None and len(ref.alns)
    path, snap = whole(case)
    for c in (None, sum(isizes(case["data"])) + 1, 0, 1):
        bi = engine.load_bam(path, keep_qual=True, chunk_bytes=c)
        loaded_equals(engine, bi, ref)
        assert snapshot(engine, bi) == snap
        info = bi.chunk_info
        bi.free()
        if c is None:
            assert info == dict(chunks=0, passes=0, largest_buffer=0, largest_carry=0)
        elif c != 1:
            assert info["chunks"] == 1 and info["passes"] == 2 and info["largest_carry"] == 0
        else:
            assert info["chunks"] > 2 and info["passes"] == 2


# ---- 4. memory bound ----------------------------------------------------------------------------------------------------------------
def test_chunk_buffer_does_not_grow_with_the_file(engine, tmp_path):
    c = 65536
    infos = []
    for copies in (K.FILLER_COPIES, 2 * K.FILLER_COPIES):
        data = K.filler_file(copies)
        isz = isizes(data)
        assert len(isz) >= 64
        p = tmp_path / ("fill%d.bam" % copies)
        p.write_bytes(data)
        bi = engine.load_bam(str(p), chunk_bytes=c)
        ref = engine.load_bam(str(p))
        assert snapshot(engine, bi) == snapshot(engine, ref)
        assert bi.counters["records"] == 40 * copies and bi.counters["reads"] == 40 * 26
        info = bi.chunk_info
        bi.free(); ref.free()
        assert info["chunks"] == len(K.plan(isz, c)) >= len(isz) - 1          # (the EOF marker joins the last chunk)
        assert info["largest_buffer"] <= c + info["largest_carry"] + 65536
        infos.append(info)
    assert infos[1]["chunks"] > infos[0]["chunks"]
    assert infos[1]["largest_buffer"] == infos[0]["largest_buffer"]          # twice the file, the same longest record: the same buffer


# ---- 5. the command -----------------------------------------------------------------------------------------------------------------
def test_command_outputs_do_not_depend_on_the_chunking(engine, data_dir, tmp_path, monkeypatch):
    def argv(reads, out, *extra):
        return ["-i", reads, "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out), "--aligner", "minimap2", "-x", "pacbio",
                "--polish", "poa"] + list(extra)
    made = telr.run(telr.get_args(argv(data_dir + "/reads.fasta", tmp_path / "reads", "-k")), engine=engine)          # the bundled BAM, as test_gpu_telr_cli.py makes it
    bam = made["files"]["bam"]
    loads = []
    load_bam = aligner.Engine.load_bam

    def watched(self, path, keep_qual=False, chunk_bytes=None):
        bi = load_bam(self, path, keep_qual=keep_qual, chunk_bytes=chunk_bytes)
        loads.append((chunk_bytes, bi.chunk_info["chunks"]))
        return bi
    monkeypatch.setattr(aligner.Engine, "load_bam", watched)
    a = telr.run(telr.get_args(argv(bam, tmp_path / "whole")), engine=engine)
    b = telr.run(telr.get_args(argv(bam, tmp_path / "chunked", "--bam_chunk_mb", "1")), engine=engine)
    assert loads[0] == (aligner.BAM_CHUNK_FIT, 0)                 # the default: the small file fits, the whole-file load
    assert loads[1][0] == 1 << 20 and loads[1][1] >= 1            # N > 0 always chunks
    # the VCF but its date and the path of the run's own copy of the reference, which lies in the output directory
    body = lambda p: [l for l in open(p).read().splitlines() if not l.startswith(("##fileDate", "##reference"))]
    assert body(a["files"]["vcf"]) == body(b["files"]["vcf"]) and sum(1 for l in body(a["files"]["vcf"]) if not l.startswith("#")) == 1
    for k in ("bed", "json"):
        assert open(a["files"][k], "rb").read() == open(b["files"][k], "rb").read() and os.path.getsize(a["files"][k]) > 0
    assert a["counts"] == b["counts"] and a["counts"]["calls"] == 1
    with pytest.raises(SystemExit):
        telr.get_args(argv(bam, tmp_path / "x", "--bam_chunk_mb", "-1"))
