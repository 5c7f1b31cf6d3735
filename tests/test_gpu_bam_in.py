"""telr_bam_load on the device == its definition in plain Python (tests/bam_in_ref.py): the inflated stream byte for byte, then records,
CIGAR words, packed words, qualities, names, counters and reads() -- integers and bytes, no tolerance.  Then the round trip through
this project's own device writer on the bundled reads, and the stage-1 consumers on the loaded result."""
import ctypes as C

import numpy as np
import pytest

import bam_in_ref as R
import inscall_ref as iref
import draft_ref as dref
from telr_amd._abi import ALN_DTYPE, MF_KEEP_CIGARS, F_SECONDARY
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

DEFLATE = R.deflate_cases()
RECORD = R.record_cases()
ERRORS = R.error_cases()
_REF = {}


def definition(c):
    """the definition's answer for a record case, computed once"""
    if c["name"] not in _REF:
        _REF[c["name"]] = R.load(c["data"], c["keep_qual"])
    return _REF[c["name"]]


def inflate_on_device(engine, path, n):
    out = np.zeros(n + 1, np.uint8)
    m = C.c_int64(-1)
    rc = engine.L.telr_debug_bgzf_inflate(engine.h, str(path).encode(), out.ctypes.data, len(out), C.byref(m))
    return rc, int(m.value), out


@pytest.mark.parametrize("case", DEFLATE, ids=[c["name"] for c in DEFLATE])
def test_deflate_case(engine, tmp_path, case):
    """one member per case (+ an empty first member and the EOF marker): the device's bytes are zlib's"""
    p = tmp_path / "m.gz"
    p.write_bytes(R.member(R.deflate_raw(b""), b"") + R.member(case["comp"], case["raw"]) + R.EOF_MARKER)
    rc, n, out = inflate_on_device(engine, p, len(case["raw"]))
    assert rc == 0, engine.L.telr_last_error(engine.h).decode()
    assert n == len(case["raw"]) and out[:n].tobytes() == case["raw"]


def test_deflate_cases_in_one_file(engine, tmp_path):
    """every case as a member of one file: each lands at its scanned offset"""
    p = tmp_path / "all.gz"
    p.write_bytes(b"".join(R.member(c["comp"], c["raw"]) for c in DEFLATE))
    want = b"".join(c["raw"] for c in DEFLATE)
    rc, n, out = inflate_on_device(engine, p, len(want))
    assert rc == 0 and n == len(want) and out[:n].tobytes() == want


def loaded_equals(engine, bi, L):
    assert bi.tnames == L.tnames and [int(x) for x in bi.tlens] == L.tlens
    assert bi.qnames == L.qnames
    assert bi.counters == L.counters
    m = bi.map_result()
    assert m.alns.dtype == ALN_DTYPE and len(m.alns) == len(L.alns)
    for f in ALN_DTYPE.names:
        np.testing.assert_array_equal(m.alns[f], L.alns[f], err_msg=f)
    np.testing.assert_array_equal(m.cigars, L.cigars)
    twin = np.zeros(len(L.cigars) + 1, np.uint32)
    assert engine.L.telr_debug_result_twin(bi.result, twin.ctypes.data, len(twin)) == len(L.cigars)          # resident on the device, complete
    np.testing.assert_array_equal(twin[:len(L.cigars)], L.cigars)
    np.testing.assert_array_equal(bi.read_set.len, [len(s) for s in L.seqs])
    e2, en = R.packed_words(L.seqs)
    if bi.read_set.n:
        w2, wn = bi.read_set.packed()
        np.testing.assert_array_equal(w2.cpu().numpy().view(np.uint32), e2)
        np.testing.assert_array_equal(wn.cpu().numpy().view(np.uint32), en)
    buf, off, ln = bi.reads()
    assert [buf[int(o):int(o) + int(l)].tobytes().decode() for o, l in zip(off, ln)] == L.seqs
    assert bi.read_set.has_qual == (L.quals is not None)
    if L.quals is not None:
        tot = sum((len(s) + 63) // 64 * 64 for s in L.seqs)
        q = np.zeros(tot, np.uint8)
        assert engine.L.telr_debug_seqset_qual(bi.read_set.h, q.ctypes.data, tot) == tot
        want, b = np.zeros(tot, np.uint8), 0
        for x in L.quals:
            want[b:b + len(x)] = np.frombuffer(x, np.uint8); b += (len(x) + 63) // 64 * 64
        np.testing.assert_array_equal(q, want)


@pytest.mark.parametrize("case", RECORD, ids=[c["name"] for c in RECORD])
def test_record_case(engine, tmp_path, case):
    p = tmp_path / "in.bam"
    p.write_bytes(case["data"])
    bi = engine.load_bam(str(p), keep_qual=case["keep_qual"])
    loaded_equals(engine, bi, definition(case))
    fa = tmp_path / "r.fasta"
    bi.write_fasta(str(fa))
    names, seqs = read_fasta(str(fa))
    assert list(names) == bi.qnames and list(seqs) == definition(case).seqs
    bi.check_targets(bi.tnames, bi.tlens)
    with pytest.raises(ValueError):
        bi.check_targets(bi.tnames[::-1] + ["x"], list(bi.tlens) + [1])
    bi.free()


def test_same_bytes_on_two_runs(engine, tmp_path):
    c = RECORD[0]
    p = tmp_path / "in.bam"
    p.write_bytes(c["data"])
    runs = []
    for _ in range(2):
        bi = engine.load_bam(str(p), keep_qual=True)
        m = bi.map_result()
        w2, wn = bi.read_set.packed()
        runs.append((m.alns.tobytes(), m.cigars.tobytes(), w2.cpu().numpy().tobytes(), wn.cpu().numpy().tobytes(), bi.reads()[0].tobytes(), bi.counters))
        bi.free()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("case", ERRORS, ids=[c["name"] for c in ERRORS])
def test_error_case(engine, tmp_path, case):
    """the code and the text; the same engine loads a good file afterwards"""
    p = tmp_path / "bad.bam"
    p.write_bytes(case["data"])
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(p))
    assert e.value.code == case["code"] and case["text"] in str(e.value), str(e.value)
    with pytest.raises(R.BamInError) as d:
        R.load(case["data"])
    assert d.value.text in str(e.value)                          # the definition's own words
    good = tmp_path / "good.bam"
    good.write_bytes(RECORD[-1]["data"])
    bi = engine.load_bam(str(good))
    assert bi.counters == definition(RECORD[-1]).counters
    bi.free()


def test_unreadable_file(engine, tmp_path):
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(tmp_path / "absent.bam"))
    assert e.value.code == R.E_IO
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(tmp_path))
    assert e.value.code == R.E_IO


@pytest.fixture(scope="module")
def bundled(engine, data_dir):
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-pb")
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    ix = engine.index(ts, io)
    rng = np.random.RandomState(4)
    qual = ["".join(chr(33 + int(v)) for v in rng.randint(0, 60, len(s))) for s in qs]
    qset, qset_q = engine.seqset(qs), engine.seqset(qs, qual=qual)
    r = ix.map_raw(qset, mo)
    yield dict(ix=ix, r=r, tn=tn, ts=ts, qn=list(qn), qs=list(qs), qset=qset, qset_q=qset_q, qual=qual)
    ix.free_raw(r)


def _key(a, cig, name):
    sec = bool(int(a["flags"]) & F_SECONDARY)
    fields = ("tid", "tlen", "qlen", "qs", "qe", "ts", "te", "mlen", "blen", "score", "dp_score", "cnt", "mapq", "flags")
    return (name,) + tuple(int(a[f]) for f in fields) + (0 if sec else int(a["subsc"]),) + \
        tuple(int(x) for x in cig[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])])


@pytest.mark.parametrize("level,keep_qual", [(0, False), (0, True), (1, False), (1, True)])
def test_round_trip_through_the_device_writer(engine, bundled, tmp_path, level, keep_qual):
    """map -> write_bam_device -> load_bam: records and reads equal the originals through the name permutation (`parent`, `n_sub` and
    the `subsc` of secondaries are not in the file)"""
    b = bundled
    p = str(tmp_path / "rt.bam")
    b["ix"].write_bam_device(b["r"], b["qset_q"] if keep_qual else b["qset"], b["qn"], b["tn"], p, level=level)
    bi = engine.load_bam(p, keep_qual=True)
    assert bi.tnames == list(b["tn"]) and [int(x) for x in bi.tlens] == [len(t) for t in b["ts"]]
    bi.check_targets(b["tn"], [len(t) for t in b["ts"]])
    assert sorted(bi.qnames) == sorted(b["qn"])
    orig = b["ix"].result_arrays(b["r"])
    c = bi.counters
    assert (c["orphans"], c["len_mismatch"], c["no_cigar"], c["no_eof"]) == (0, 0, 0, 0) and c["kept"] == len(orig.alns) == c["mapped"] and c["reads"] == len(b["qn"])
    qid_in = {n: i for i, n in enumerate(b["qn"])}
    buf, off, ln = bi.reads()
    for q, n in enumerate(bi.qnames):
        s = b["qs"][qid_in[n]].upper()
        assert buf[int(off[q]):int(off[q]) + int(ln[q])].tobytes().decode() == "".join(ch if ch in "ACGT" else "N" for ch in s)
    m = bi.map_result()
    assert sorted(_key(a, m.cigars, bi.qnames[int(a["qid"])]) for a in m.alns) == sorted(_key(a, orig.cigars, b["qn"][int(a["qid"])]) for a in orig.alns)
    assert np.all(np.diff(m.alns["qid"]) >= 0)
    assert bi.read_set.has_qual == keep_qual
    if keep_qual:
        tot = int(((bi.read_set.len.astype(np.int64) + 63) // 64 * 64).sum())
        q = np.zeros(tot, np.uint8)
        assert engine.L.telr_debug_seqset_qual(bi.read_set.h, q.ctypes.data, tot) == tot
        base = 0
        for k, n in enumerate(bi.qnames):
            want = np.frombuffer(b["qual"][qid_in[n]].encode(), np.uint8) - 33
            np.testing.assert_array_equal(q[base:base + len(want)], want)
            base += (len(want) + 63) // 64 * 64
    bi.free()


def test_downstream_on_the_loaded_result(engine, bundled, tmp_path):
    """call_insertions / genotype_insertions on the loaded result: the same calls and the same supporter and reference NAME sets as on
    the original result (the known chr2L call with 13 reads); draft_contigs on the loaded result and set == tests/draft_ref.py on the
    loaded arrays"""
    b = bundled
    p = str(tmp_path / "ds.bam")
    b["ix"].write_bam_device(b["r"], b["qset"], b["qn"], b["tn"], p, level=1)
    bi = engine.load_bam(p)
    ic0 = b["ix"].call_insertions(b["r"]); g0 = b["ix"].genotype_insertions(b["r"], ic0)
    ic1 = b["ix"].call_insertions(bi.result); g1 = b["ix"].genotype_insertions(bi.result, ic1)
    assert len(ic0.calls) == len(ic1.calls) == 1 and int(ic0.calls[0]["support"]) == 13
    for f in ("tid", "pos", "len", "support", "n_sized"):
        np.testing.assert_array_equal(ic0.calls[f], ic1.calls[f], err_msg=f)
    for f in ("ref", "ambig", "alt", "gt"):
        np.testing.assert_array_equal(g0.gt[f], g1.gt[f], err_msg=f)
    for k in range(len(ic0.calls)):
        assert {b["qn"][q] for q in ic0.reads_of(k)} == {bi.qnames[q] for q in ic1.reads_of(k)}
        assert {b["qn"][q] for q in g0.ref_reads_of(k)} == {bi.qnames[q] for q in g1.ref_reads_of(k)}
    d, s = b["ix"].draft_contigs(bi.result, ic1, bi.read_set)
    m = bi.map_result()
    buf, off, ln = bi.reads()
    seqs = [buf[int(o):int(o) + int(l)].tobytes().decode() for o, l in zip(off, ln)]
    sigs, calls = iref.call_insertions(m.alns, m.cigars)
    wd, wseq = dref.drafts(m.alns, m.cigars, calls, sigs, seqs)
    assert len(d) == len(wd) == 1 and int(d[0]["sig"]) >= 0
    for f in dref.DRAFT_FIELDS:
        assert int(d[0][f]) == int(wd[0][f]), f
    e2, en = R.packed_words(wseq)
    w2, wn = s.packed()
    np.testing.assert_array_equal(w2.cpu().numpy().view(np.uint32), e2)
    np.testing.assert_array_equal(wn.cpu().numpy().view(np.uint32), en)
    s.free(); bi.free()


def test_bam_input_mirrors_the_bam_branch_of_parse_input(engine, bundled, tmp_path):
    from telr_amd import telr_alignment
    b = bundled
    p = str(tmp_path / "in.bam")
    b["ix"].write_bam_device(b["r"], b["qset"], b["qn"], b["tn"], p, level=1)
    bi = telr_alignment.bam_input(p, str(tmp_path), "s", engine, index=b["ix"])
    names, seqs = read_fasta(str(tmp_path / "s.telr.fasta"))
    assert list(names) == bi.qnames and len(seqs) == len(b["qs"])
    bi.free()
