"""telr_seqset_join and telr_bridge_contigs on the device == their definitions in plain Python (tests/bridge_ref.py): the joined set's
packed words and mask words word for word what the packer makes of the expected strings, padding included; the bridge records field for
field.  The inputs are those of tests/bridge_cases.py, where every case asserts the edge it claims (tests/test_bridge_ref.py).  The last
tests run a planted insertion that no read spans through draft_loci, run_loci and the `telr` command."""
import ctypes as C

import numpy as np
import pytest

import bridge_cases as cases
import bridge_ref as bref
import draft_cases
import draft_ref as dref
import packed_np
from inscall_cases import pack
from telr_amd import locus_pipeline, telr, telr_assembly, telr_sv
from telr_amd._abi import BridgeOpt, DraftOpt, InsOpt, MF_KEEP_CIGARS, TELR_E_ARG, BRIDGE_DTYPE
from telr_amd._lib import TelrError
from telr_amd.aligner import Engine
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

BRIDGE = cases.bridge_cases()


def words(s):
    w2, wn = s.packed()
    return w2.cpu().numpy().view(np.uint32).copy(), wn.cpu().numpy().view(np.uint32).copy()


# ---- join ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parent(engine):
    seqs = cases.join_parent()
    s = engine.seqset(seqs)
    yield seqs, s
    s.free()


def test_join_equals_the_packed_strings(parent):
    """piece lengths 0 .. 65, a second piece at every residue mod 32, 1 to 3 pieces, three inside one word, rc on either piece, N at a
    seam, repeats, overlaps, sequences without pieces: one call, word for word including the padding"""
    seqs, pset = parent
    off, idx, start, ln, rc, names = cases.join_cases(seqs)
    want = bref.join(seqs, off, idx, start, ln, rc)
    got = pset.join(off, idx, start, ln, rc)
    e_len, e2, en = packed_np.pack(want)
    w2, wn = words(got)
    np.testing.assert_array_equal(got.len, e_len)
    np.testing.assert_array_equal(w2, e2)
    np.testing.assert_array_equal(wn, en)
    assert got.n == len(names) and not got.has_qual
    # the text of the set is the strings (telr_seqset_extract on the joined set)
    text = got.extract(np.arange(got.n), np.zeros(got.n, np.int32), got.len)
    assert [t.decode() for t in text] == want
    again = pset.join(off, idx, start, ln, rc)
    a2, an = words(again)
    assert a2.tobytes() == w2.tobytes() and an.tobytes() == wn.tobytes()          # the same bytes on two runs
    # rc None = all forward
    fwd = pset.join(off, idx, start, ln)
    f_len, f2, fn = packed_np.pack(bref.join(seqs, off, idx, start, ln))
    g2, gn = words(fwd)
    np.testing.assert_array_equal(g2, f2); np.testing.assert_array_equal(gn, fn)
    for s in (got, again, fwd):
        s.free()


def test_join_empty_sets(parent):
    seqs, pset = parent
    s = pset.join([0], [], [], [])
    assert s.n == 0 and len(words(s)[0]) == 0
    s.free()
    s = pset.join([0, 0, 0], [], [], [])                 # two sequences without pieces
    assert s.n == 2 and s.len.tolist() == [0, 0] and len(words(s)[0]) == 0
    s.free()
    h = C.c_void_p()
    assert pset.eng.L.telr_seqset_join(pset.eng.h, pset.h, 0, None, None, None, None, None, C.byref(h)) == 0 and h.value
    assert pset.eng.L.telr_seqset_count(h) == 0
    pset.eng.L.telr_seqset_free(h)


def test_join_refused_arguments_leave_no_set(parent):
    seqs, pset = parent
    L, eh = pset.eng.L, pset.eng.h
    i32, i64 = (lambda v: np.array(v, np.int32)), (lambda v: np.array(v, np.int64))

    def refused(text, off, idx, start, ln, n_out=None, rc=None, code=TELR_E_ARG, null=()):
        off, idx, start, ln = i64(off), i32(idx), i32(start), i32(ln)
        h = C.c_void_p()
        ptr = lambda name, a: None if name in null else a.ctypes.data
        got = L.telr_seqset_join(eh, pset.h, len(off) - 1 if n_out is None else n_out, ptr("off", off), ptr("idx", idx), ptr("start", start), ptr("len", ln),
                                 None if rc is None else np.array(rc, np.uint8).ctypes.data, C.byref(h))
        msg = L.telr_last_error(eh)
        assert got == code and not h.value, (text, got)
        assert b"telr_seqset_join" in msg and text in msg, msg

    refused(b"negative n_out", [0], [], [], [], n_out=-1)
    refused(b"null piece_off", [0, 1], [0], [0], [1], null=("off",))
    refused(b"does not start at 0", [1, 1], [0], [0], [1])
    refused(b"piece_off decreases", [0, 2, 1], [0, 0], [0, 0], [1, 1])
    refused(b"null idx, start or len", [0, 1], [0], [0], [1], null=("idx",))
    refused(b"null idx, start or len", [0, 1], [0], [0], [1], null=("len",))
    refused(b"idx outside the set", [0, 1], [len(seqs)], [0], [1])
    refused(b"idx outside the set", [0, 1], [-1], [0], [1])
    refused(b"negative start", [0, 1], [0], [-1], [1])
    refused(b"negative len", [0, 1], [0], [0], [-1])
    refused(b"start + len beyond the sequence", [0, 2], [0, 2], [0, 60], [len(seqs[0]), 5])
    h = C.c_void_p()
    assert L.telr_seqset_join(eh, None, 0, None, None, None, None, None, C.byref(h)) == TELR_E_ARG and not h.value
    assert L.telr_seqset_join(eh, pset.h, 0, None, None, None, None, None, None) == TELR_E_ARG
    with pytest.raises(ValueError):
        pset.join([0, 2], [0], [0], [1])
    with pytest.raises(ValueError):
        pset.join([0, 1], [0], [0], [1], rc=[0, 1])
    with pytest.raises(TelrError) as e:
        pset.join([0, 1], [9], [0], [1])
    assert e.value.code == TELR_E_ARG


# ---- bridge -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ix(engine):
    """the step only needs the number of targets: two short ones"""
    io, _ = preset("map-ont")
    return engine.index(["ACGT" * 64, "TTGCA" * 64], io)


def engine_bridges(engine, ix, data, opt, want=None, read_set=None):
    alns, cig, sigs, calls, reads = data
    qs = read_set if read_set is not None else engine.seqset(reads)
    r = ix.result_from_arrays(alns, cig)
    try:
        return ix.bridge_contigs(r, cases.as_ic(calls, sigs), qs, BridgeOpt.default(**opt), want)
    finally:
        ix.free_raw(r)
        if read_set is None:
            qs.free()


def assert_equal_to_ref(got, want):
    assert got.dtype == BRIDGE_DTYPE and len(got) == len(want)
    for f in bref.BRIDGE_FIELDS:
        np.testing.assert_array_equal(got[f], np.array([x[f] for x in want], np.int64), err_msg=f)


@pytest.mark.parametrize("case", BRIDGE, ids=[c["name"] for c in BRIDGE])
def test_bridge_case(engine, ix, case):
    alns, cig, sigs, calls, reads = case["data"]
    want, seqs = bref.bridges(alns, cig, calls, sigs, reads, case["opt"], case["want"])
    case["expect"](want, seqs)
    got = engine_bridges(engine, ix, case["data"], case["opt"], case["want"])
    assert_equal_to_ref(got, want)


def test_noisy_pairs_and_their_contigs(engine, ix):
    """200 seeded pairs of reads with 10 % errors on seeded strands: the records field for field, and the contigs of the bridged calls
    through SeqSet.join word for word.  How many are bridged is printed, not asserted."""
    data, opt = cases.noisy_pairs()
    alns, cig, sigs, calls, reads = data
    want, seqs = bref.bridges(alns, cig, calls, sigs, reads, opt)
    qs = engine.seqset(reads)
    runs = [engine_bridges(engine, ix, data, opt, read_set=qs) for _ in range(2)]
    assert_equal_to_ref(runs[0], want)
    assert runs[0].tobytes() == runs[1].tobytes()                                  # the same bytes on two runs
    have = runs[0][runs[0]["sig_l"] >= 0]
    print("bridged %d of %d, votes %d .. %d" % (len(have), len(want), have["votes"].min() if len(have) else 0, have["votes"].max() if len(have) else 0))
    off = np.arange(len(have) + 1, dtype=np.int64) * 2
    inter = lambda a, b: np.stack([have[a], have[b]], 1).ravel()
    cset = qs.join(off, inter("qid_l", "qid_r"), inter("start_l", "start_r"), inter("len_l", "len_r"), inter("rc_l", "rc_r"))
    e_len, e2, en = packed_np.pack([s for s in seqs if s is not None])
    w2, wn = words(cset)
    np.testing.assert_array_equal(cset.len, e_len)
    np.testing.assert_array_equal(w2, e2)
    np.testing.assert_array_equal(wn, en)
    cset.free(); qs.free()


def test_same_bytes_on_two_runs(engine, ix):
    picks = [c for c in BRIDGE if c["name"] in ("table_full", "pairs_tied", "cut_wide_enough", "V_several_chunks", "window_duplicate")]
    assert len(picks) == 5
    runs = [b"".join(engine_bridges(engine, ix, c["data"], c["opt"], c["want"]).tobytes() for c in picks) for _ in range(2)]
    assert runs[0] == runs[1]


def engine_drafts(engine, ix, data, opt):
    """-> (draft records, lengths, 2-bit words, mask words of the output set) of Index.draft_contigs on a bridge-style data tuple"""
    alns, cig, sigs, calls, reads = data
    qs = engine.seqset(reads)
    r = ix.result_from_arrays(alns, cig)
    try:
        d, s = ix.draft_contigs(r, cases.as_ic(calls, sigs), qs, DraftOpt.default(**opt))
        out = (d, s.len.copy()) + words(s)
        s.free()
        return out
    finally:
        ix.free_raw(r); qs.free()


def test_sized_and_clip_signatures_in_one_window(engine, ix):
    """one call, a sized signature between two clips: the one span kernel counts the clips for the bridge and the sized one for the
    drafter, and only the kind mask keeps them apart -- either step equals its own definition"""
    c = next(c for c in BRIDGE if c["name"] == "sized_among_clips")
    alns, cig, sigs, calls, reads = c["data"]
    assert [s["kind"] for s in sigs] == [2, 0, 2] and len(calls) == 1
    want, _ = bref.bridges(alns, cig, calls, sigs, reads, c["opt"])
    assert want[0]["sig_l"] == 0 and want[0]["sig_r"] == 2 and want[0]["n_left"] == 1 and want[0]["n_right"] == 1
    assert_equal_to_ref(engine_bridges(engine, ix, c["data"], c["opt"]), want)
    wd, wseq = dref.drafts(alns, cig, calls, sigs, reads, draft_cases.SMALL)
    assert wd[0]["sig"] == 1 and wd[0]["n_candidates"] == 1 and wd[0]["qid"] == 2 and len(wseq) == 1
    d, lens, w2, wn = engine_drafts(engine, ix, c["data"], draft_cases.SMALL)
    for f in dref.DRAFT_FIELDS:
        np.testing.assert_array_equal(d[f], np.array([x[f] for x in wd], np.int64), err_msg=f)
    e_len, e2, en = packed_np.pack(wseq)
    np.testing.assert_array_equal(lens, e_len); np.testing.assert_array_equal(w2, e2); np.testing.assert_array_equal(wn, en)


def test_draft_and_bridge_share_their_input_buffers(engine, ix):
    """telr_draft_contigs and telr_bridge_contigs keep their input in the same context buffers.  On ONE engine: the drafter on two records
    and one call, the bridge on its hand case of the most records, the drafter on 70 records (more than a wave), the bridge on its hand
    case of the fewest, the first drafter call again -- inputs grow and shrink through the same buffers, and both kind masks go through
    the one span kernel back to back.  Every result equals, byte for byte, that of the same call on a fresh engine."""
    recs = [draft_cases.ins_rec(0, 1000, 60), draft_cases.ins_rec(1, 1003, 62)]      # the input of test_gpu_draft.py::test_argument_errors
    alns, cig = pack(recs)
    two = (alns, cig, draft_cases.sigs_of(alns, cig), [draft_cases.call(0, 1000, 60, [0, 1])], draft_cases.random_reads(recs))
    recs, calls = draft_cases.many_candidates()
    alns, cig = pack(recs)
    many = (alns, cig, draft_cases.sigs_of(alns, cig), calls, draft_cases.random_reads(recs, calls))
    big = max(BRIDGE, key=lambda c: len(c["data"][0]))
    small = min(BRIDGE, key=lambda c: len(c["data"][0]))
    assert len(big["data"][0]) >= 14 and len(small["data"][0]) == 2 and len(many[0]) == 70
    draft = lambda e, i, data: b"".join(np.ascontiguousarray(x).tobytes() for x in engine_drafts(e, i, data, draft_cases.SMALL))
    bridge = lambda e, i, c: engine_bridges(e, i, c["data"], c["opt"], c["want"]).tobytes()
    steps = [(draft, two), (bridge, big), (draft, many), (bridge, small), (draft, two)]
    got = [f(engine, ix, x) for f, x in steps]
    assert got[0] == got[4] and len(got[0]) > 0 and len(got[2]) > 0
    io, _ = preset("map-ont")
    for k, (f, x) in enumerate(steps[:4]):
        fresh = Engine(0)
        fix = fresh.index(["ACGT" * 64, "TTGCA" * 64], io)
        try:
            assert f(fresh, fix, x) == got[k], "step %d" % k
        finally:
            fix.free(); fresh.close()


def test_zero_calls_and_zero_signatures(engine, ix):
    c = next(c for c in BRIDGE if c["name"] == "pairs_tied")
    alns, cig, sigs, calls, reads = c["data"]
    for cc, ss in (([], sigs), ([], []), (calls, [])):
        got = engine_bridges(engine, ix, (alns, cig, ss, cc, reads), c["opt"])
        assert len(got) == len(cc) and (got["sig_l"] == -1).all() and (got["sig_r"] == -1).all() and not got["n_left"].any() and not got["votes"].any()


def test_argument_errors(engine, ix):
    c = next(c for c in BRIDGE if c["name"] == "pairs_tied")
    alns, cig, sigs, calls, reads = c["data"]

    def refused(text, alns=alns, calls=calls, sigs=sigs, opt=None, reads=reads, want=None, err=TelrError):
        with pytest.raises(err) as e:
            engine_bridges(engine, ix, (alns, cig, sigs, calls, reads), dict(cases.SMALL, **(opt or {})), want)
        if err is TelrError and e.value.code is not None:
            assert e.value.code == TELR_E_ARG
            msg = engine.L.telr_last_error(engine.h)
            assert b"telr_bridge_contigs" in msg and text in msg, msg

    for f in ("flank", "min_flank", "reach", "max_len"):
        refused(b"negative option", opt={f: -1} if f != "flank" else dict(flank=-1, min_flank=-2))
    refused(b"min_flank > flank", opt=dict(flank=10, min_flank=11))
    for k in (10, 16):
        refused(b"k outside", opt=dict(k=k))
    refused(b"window outside", opt=dict(window=12))
    refused(b"window outside", opt=dict(window=4097))
    for p in (0, 9):
        refused(b"pairs outside", opt=dict(pairs=p))
    refused(b"min_votes below 1", opt=dict(min_votes=0))
    # what telr_draft_contigs refuses
    refused(b"not strictly ascending", calls=[calls[0], calls[0]])
    refused(b"tid", calls=[dict(calls[0], tid=2)])
    refused(b"tid", sigs=[dict(sigs[0], tid=-1)] + sigs[1:])
    refused(b"rec outside", sigs=[dict(sigs[0], rec=len(alns))] + sigs[1:])
    refused(b"qid outside", sigs=[dict(sigs[0], qid=len(reads))] + sigs[1:])
    refused(b"qid is not", sigs=[dict(sigs[0], qid=1)] + sigs[1:])
    refused(b"signatures not ascending", sigs=[dict(sigs[0], pos=sigs[0]["pos"] + 1)] + sigs[1:])
    refused(b"read id outside", calls=[dict(calls[0], reads=[0, 1, 2, 3, 4])])
    a2 = alns.copy(); a2["te"] = 100
    refused(b"coordinates", alns=a2)
    refused(b"qlen is not the length", reads=[reads[0] + "A"] + reads[1:])
    refused(b"one want flag per call", want=[1, 0])
    # the C entry itself: NULL arguments, and NULL options = the defaults
    qs = engine.seqset(reads)
    r = ix.result_from_arrays(alns, cig)
    try:
        ic = cases.as_ic(calls, sigs)
        h = C.c_void_p()
        L = engine.L
        args = (1, ic.calls.ctypes.data, ic.read_off.ctypes.data, ic.reads.ctypes.data, len(ic.sigs), ic.sigs.ctypes.data)
        assert L.telr_bridge_contigs(engine.h, r, 0, *args, qs.h, None, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_bridge_contigs(engine.h, None, 2, *args, qs.h, None, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_bridge_contigs(engine.h, r, 2, *args, None, None, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_bridge_contigs(engine.h, r, 2, *args, qs.h, None, None, None) == TELR_E_ARG
        assert not h.value
        assert L.telr_bridge_contigs(engine.h, r, 2, *args, qs.h, None, None, C.byref(h)) == 0
        # the default min_flank of 500 refuses the flanks of 30: no candidate on either side
        assert L.telr_bridges_count(h) == 1
        got = np.frombuffer((C.c_char * 64).from_address(L.telr_bridges_data(h)), BRIDGE_DTYPE)[0]
        assert (got["sig_l"], got["sig_r"], got["n_left"], got["n_right"]) == (-1, -1, 0, 0)
        L.telr_bridge_contigs_free(h)
    finally:
        ix.free_raw(r); qs.free()
    o = BridgeOpt()
    engine.L.telr_bridge_opt_default(C.byref(o))
    assert {k: getattr(o, k) for k in bref.DEFAULTS} == bref.DEFAULTS
    with pytest.raises(TypeError):
        BridgeOpt.default(nope=1)


# ---- an insertion that no read spans: draft_loci, run_loci, the command ---------------------------------------------------------------
@pytest.fixture(scope="module")
def spanless(engine, tmp_path_factory):
    f = cases.spanless_fixture()
    d = tmp_path_factory.mktemp("spanless")
    (d / "ref.fasta").write_text(">chrT\n%s\n" % f["chrom"])
    (d / "lib.fasta").write_text(">famL\n%s\n" % f["fam"])
    (d / "reads.fasta").write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(f["names"], f["reads"])))
    return f, d


def test_spanless_through_draft_loci_and_run_loci(engine, spanless):
    """the device against the checker over the engine's own records, then the truth: the bridged contig holds the family, polishing with
    POA keeps it annotated as famL, and the liftover puts it inside the range of the cluster's signature positions"""
    f, _ = spanless
    io, mo = preset("map-ont")
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    fix = engine.index([f["chrom"]], io)
    qset = engine.seqset(f["reads"])
    r = fix.map_raw(qset, mo)
    try:
        assert len(fix.call_insertions(r).calls) == 0                             # today's caller: the cluster has no sized signature
        opt = InsOpt.default(min_sized=0)
        ic = fix.call_insertions(r, opt)
        assert len(ic.calls) == 1 and int(ic.calls[0]["rep"]) == -1
        res = fix.result_arrays(r)
        sigs = [{k: int(s[k]) for k in s.dtype.names} for s in ic.sigs]
        calls = [dict({k: int(c[k]) for k in c.dtype.names}, reads=ic.reads_of(0).tolist()) for c in ic.calls]
        want, wseq = bref.bridges(res.alns, res.cigars, calls, sigs, f["reads"])
        got = fix.bridge_contigs(r, ic, qset)
        assert_equal_to_ref(got, want)
        assert got["sig_l"][0] >= 0
        pos = [int(s["pos"]) for s in ic.sigs]
        rows = telr_sv.call_insertions(fix, r, ["chrT"], f["names"], qset, opt=opt, sample="s", genotype=True)
        assert len(rows) == 1 and rows[0][7] == "N" and rows[0][3] == "0"
        # without bridge: what it does today -- the call is skipped
        loci, cset, skipped = telr_assembly.draft_loci(fix, r, ic, rows, qset, qset, {"chrT": 0})
        assert loci == [] and cset.n == 0 and skipped == [telr_sv.locus_name(rows[0])]
        cset.free()
        loci, cset, skipped = telr_assembly.draft_loci(fix, r, ic, rows, qset, qset, {"chrT": 0}, bridge=True)
        assert skipped == [] and len(loci) == 1 and cset.n == 1
        l = loci[0]
        assert l["contig"] == wseq[0] and l["bridged"] is True and l["ins_len"] == int(got["ins_len"][0])
        assert l["alt"] == l["contig"][int(got["ins_off"][0]):int(got["ins_off"][0]) + l["ins_len"]]
        sl, sr = sigs[int(got["sig_l"][0])], sigs[int(got["sig_r"][0])]
        assert l["contig"] == f["hap"][sl["pos"] - 2000:sr["pos"] + 2000 + len(f["fam"])] and f["fam"] in l["alt"]          # the truth, letter for letter
        io10, _ = preset("asm10")
        ix10 = engine.index(fix.targets, io10)
        out = locus_pipeline.run_loci(engine, ix10, ["chrT"], lambda ch: f["chrom"], loci, ["famL"], [f["fam"]], presets="ont", read_set=qset,
                                      polish="poa", contig_set=cset)
        print(out["annotation"], [x["report"] for x in out["liftover"]], out["af"])
        assert len(out["annotation"]) == 1 and out["annotation"][0][0] == l["name"] and out["annotation"][0][3] == "famL"
        assert len(out["liftover"]) == 1
        rep = out["liftover"][0]["report"]
        assert (rep["type"], rep["family"], rep["chrom"]) == ("non-reference", "famL", "chrT")
        assert min(pos) <= rep["start"] <= rep["end"] <= max(pos) + 1
        cset.free(); ix10.free()
    finally:
        fix.free_raw(r); qset.free(); fix.free()


def vcf_body(path):
    return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("#")]


def test_telr_with_and_without_bridge(engine, spanless, tmp_path, capsys):
    f, d = spanless
    base = ["-i", str(d / "reads.fasta"), "-r", str(d / "ref.fasta"), "-l", str(d / "lib.fasta"), "--aligner", "minimap2", "-x", "ont", "--polish", "poa"]
    plain = telr.run(telr.get_args(base + ["-o", str(tmp_path / "plain")]), engine=engine)
    assert "TELR found no non-reference TE insertions" in capsys.readouterr().err          # today's behaviour
    assert plain["final"] == [] and plain["counts"]["calls"] == 0 and "calls_bridged" not in plain["counts"]
    assert vcf_body(plain["files"]["vcf"]) == []
    out = telr.run(telr.get_args(base + ["-o", str(tmp_path / "bridge"), "--bridge", "-k"]), engine=engine)
    err = capsys.readouterr().err
    print(err, out["counts"], [{k: v for k, v in x.items() if k != "te_sequence"} for x in out["final"]])
    assert "1 of them bridges of two reads" in err
    assert out["counts"]["calls"] == 1 and out["counts"]["calls_bridged"] == 1 and out["counts"]["calls_without_draft"] == 0
    body = vcf_body(out["files"]["vcf"])
    assert len(body) == 1 and body[0][0] == "chrT" and "FAMILY=famL" in body[0][7]
    # the cluster's signature positions: every clip is at the planted position or the few bases an alignment runs on by chance
    assert f["pos"] - 20 <= int(body[0][1]) <= f["pos"] + 21
    assert len(out["final"]) == 1 and out["final"][0]["family"] == "famL" and out["final"][0]["chrom"] == "chrT"
    table = telr_sv.read_locus_table(out["files"]["locus_table"])
    assert len(table) == 1 and int(table[0][3]) >= len(f["fam"]) and f["fam"] in table[0][7]


def test_bundled_reads_same_vcf_with_and_without_bridge(engine, data_dir, tmp_path):
    """the bundled reads' one call has sized reads and a draft: --bridge changes nothing in the VCF body"""
    def run(out, *extra):
        argv = ["-i", data_dir + "/reads.fasta", "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out),
                "--aligner", "minimap2", "-x", "pacbio", "--polish", "poa"] + list(extra)
        return telr.run(telr.get_args(argv), engine=engine)
    a, b = run(tmp_path / "a"), run(tmp_path / "b", "--bridge")
    assert len(vcf_body(a["files"]["vcf"])) == 1 and vcf_body(a["files"]["vcf"]) == vcf_body(b["files"]["vcf"])
    print(a["counts"], b["counts"])
    assert b["counts"]["calls_bridged"] == 0 and "calls_bridged" not in a["counts"]
