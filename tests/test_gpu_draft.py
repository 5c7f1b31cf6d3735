"""telr_draft_contigs on the device == its definition in plain Python (tests/draft_ref.py): the draft records array for array, the output
set's packed words and mask words word for word what the packer makes of the expected strings, padding included.  Records are built by
hand and wrapped with result_from_arrays, so every edge is exact; the last tests run the step behind a real map call (the bundled reads)."""
import ctypes as C
import types

import numpy as np
import pytest

import draft_cases as cases
import draft_ref as dref
import inscall_ref as iref
import packed_np
from inscall_cases import pack
from telr_amd import locus_pipeline, telr_assembly, telr_sv
from telr_amd._abi import DraftOpt, MF_KEEP_CIGARS, TELR_E_ARG, INS_CALL_DTYPE, INS_SIG_DTYPE, DRAFT_DTYPE
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()


@pytest.fixture(scope="module")
def ix(engine):
    """the step only needs the number of targets: two short ones"""
    io, _ = preset("map-ont")
    return engine.index(["ACGT" * 64, "TTGCA" * 64], io)


def as_ic(calls, sigs):
    """checker-style calls and signatures -> what Index.draft_contigs takes"""
    a = np.zeros(len(calls), INS_CALL_DTYPE)
    for k, c in enumerate(calls):
        for f in ("tid", "pos", "len", "support", "n_sized", "rep"):
            a[k][f] = c[f]
    s = np.zeros(len(sigs), INS_SIG_DTYPE)
    for k, x in enumerate(sigs):
        for f in iref.SIG_FIELDS:
            s[k][f] = x[f]
    off = np.zeros(len(calls) + 1, np.int64)
    off[1:] = np.cumsum([len(c["reads"]) for c in calls])
    return types.SimpleNamespace(calls=a, sigs=s, read_off=off, reads=np.array([q for c in calls for q in c["reads"]], np.int32))


def engine_drafts(engine, ix, alns, cig, ic, reads, opt, read_set=None):
    """-> (draft records, lengths, 2-bit words, mask words of the output set)"""
    qs = read_set if read_set is not None else engine.seqset(reads)
    r = ix.result_from_arrays(alns, cig)
    try:
        d, s = ix.draft_contigs(r, ic, qs, DraftOpt.default(**opt))
        w2, wn = s.packed()
        out = d, s.len.copy(), w2.cpu().numpy().view(np.uint32).copy(), wn.cpu().numpy().view(np.uint32).copy()
        s.free()
        return out
    finally:
        ix.free_raw(r)
        if read_set is None:
            qs.free()


def assert_equal_to_ref(got, want, seqs):
    d, lens, w2, wn = got
    assert d.dtype == DRAFT_DTYPE and len(d) == len(want)
    for f in dref.DRAFT_FIELDS:
        np.testing.assert_array_equal(d[f], np.array([x[f] for x in want], np.int64), err_msg=f)
    e_len, e2, en = packed_np.pack(seqs)
    np.testing.assert_array_equal(lens, e_len)
    np.testing.assert_array_equal(w2, e2)
    np.testing.assert_array_equal(wn, en)


def check(engine, ix, recs, calls, sigs, opt, reads=None):
    alns, cig = pack(recs)
    sigs = sigs if sigs is not None else cases.sigs_of(alns, cig)
    reads = reads if reads is not None else cases.random_reads(recs, calls)
    want, seqs = dref.drafts(alns, cig, calls, sigs, reads, opt)
    assert_equal_to_ref(engine_drafts(engine, ix, alns, cig, as_ic(calls, sigs), reads, opt), want, seqs)
    return alns, cig, sigs, want, seqs


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(engine, ix, case):
    _, recs, calls, sigs, opt, hand = case
    _, _, _, want, _ = check(engine, ix, recs, calls, sigs, opt)
    assert [{k: d[k] for k in dref.DRAFT_FIELDS} for d in want] == hand          # (and the checker's answer is the hand-derived one)


def test_walk_edges(engine, ix):
    """CIGARs of 1 .. 129 words and one of more than 100,000, xL / xR in the first word, the last word and on either side of every
    64-word step seam, splits in either record order: every case claims its edge, and the claim is checked on the records"""
    recs, calls, claims = cases.walk_cases()
    alns, cig, sigs, want, _ = check(engine, ix, recs, calls, None, cases.WALK_OPT)
    assert max(int(a["n_cigar"]) for a in alns) > 100000
    assert set(int(a["n_cigar"]) for a in alns) >= {1, 63, 64, 65, 128, 129}
    orders = set()
    for d, (name, cl, cr) in zip(want, claims):
        assert d["sig"] >= 0, name
        s = sigs[d["sig"]]
        a = alns[s["rec"]]
        b = a if s["kind"] == 0 else alns[s["mate"]]
        if s["kind"] == 1:
            orders.add(s["rec"] < s["mate"])
        rpos = s["pos"] if s["kind"] == 0 else int(b["ts"])
        xL, xR = max(int(a["ts"]), s["pos"] - cases.F), min(int(b["te"]), rpos + cases.F)
        assert cases.claim_holds(cl, cases.op_places(a, cig, xL), int(a["n_cigar"])), (name, "xL")
        assert cases.claim_holds(cr, cases.op_places(b, cig, xR), int(b["n_cigar"])), (name, "xR")
    assert orders == {True, False}
    assert any(d["rc"] for d in want)


def test_piece_edges(engine, ix):
    """the extraction: start offsets 0, 1, 15, 16, 31 (mod 32) and base 0, lengths 1 .. 65, pieces that end on their read's last base, the
    last read of the set, forward and rc, an N on both ends of every rc piece; 154 calls are more than two waves of the selection"""
    recs, calls, sigs, reads, claims = cases.piece_cases()
    _, _, _, want, seqs = check(engine, ix, recs, calls, sigs, cases.PIECE_OPT, reads)
    assert len(want) > 150 and all(d["sig"] >= 0 for d in want)
    seen = set()
    for d, c, s in zip(want, claims, seqs):
        assert (d["start"], d["len"], d["rc"]) == (c["start"], c["len"], c["rc"])
        assert (d["start"] + d["len"] == len(reads[d["qid"]])) == c["ends_on_last_base"]
        if d["rc"]:
            assert s[0] == "N" and s[-1] == "N"
        seen.add((d["start"] % 32 if d["start"] else "zero", d["len"], d["rc"], c["ends_on_last_base"]))
    for off in ("zero", 0, 1, 15, 16, 31):
        for ln in (1, 15, 16, 17, 63, 64, 65):
            for rc in (0, 1):
                assert (off, ln, rc, False) in seen and (off == "zero" or (off, ln, rc, True) in seen)
    assert want[-1]["qid"] == len(reads) - 1 and want[-1]["start"] + want[-1]["len"] == len(reads[-1])      # the last read, to its last base


def test_more_candidates_than_a_wave(engine, ix):
    recs, calls = cases.many_candidates()
    _, _, _, want, _ = check(engine, ix, recs, calls, None, cases.SMALL)
    assert want[0]["n_valid"] == 70 > 64 and want[0]["qid"] == 69


def test_no_draft_at_all_and_zero_calls(engine, ix):
    recs, calls, claims = cases.walk_cases()
    keep = [k for k, c in enumerate(claims) if c[0].endswith("first_last") or c[0] == "3_words_ts_te"]      # (one record per call up to there)
    recs, calls = [recs[k] for k in keep], [calls[k] for k in keep]
    assert len(calls) == 6 and all(r["qid"] == c["reads"][0] for r, c in zip(recs, calls))
    alns, cig = pack(recs)
    sigs = cases.sigs_of(alns, cig)
    reads = cases.random_reads(recs)
    # these records end less than 1,900 bases from their insertion: no candidate is valid
    want, seqs = dref.drafts(alns, cig, calls, sigs, reads, dict(min_flank=1900))
    assert all(d["sig"] == -1 and d["n_candidates"] for d in want) and seqs == []
    got = engine_drafts(engine, ix, alns, cig, as_ic(calls, sigs), reads, dict(min_flank=1900))
    assert_equal_to_ref(got, want, seqs)
    assert len(got[1]) == 0 and len(got[2]) == 0 and len(got[3]) == 0
    # zero calls, with and without signatures; calls without signatures
    for c, s in (([], sigs), ([], []), (calls, [])):
        got = engine_drafts(engine, ix, alns, cig, as_ic(c, s), reads, {})
        assert len(got[0]) == len(c) and (got[0]["sig"] == -1).all() and (got[0]["set_index"] == -1).all() and len(got[2]) == 0


def test_same_bytes_on_every_run(engine, ix):
    recs, calls, sigs, reads, _ = cases.piece_cases()
    w_recs, w_calls, _ = cases.walk_cases()
    runs = []
    for _ in range(3):
        alns, cig = pack(recs)
        a = engine_drafts(engine, ix, alns, cig, as_ic(calls, sigs), reads, cases.PIECE_OPT)
        alns, cig = pack(w_recs)
        b = engine_drafts(engine, ix, alns, cig, as_ic(w_calls, cases.sigs_of(alns, cig)), cases.random_reads(w_recs), cases.WALK_OPT)
        runs.append(b"".join(x.tobytes() for x in a + b))
    assert runs[0] == runs[1] == runs[2]


def test_argument_errors(engine, ix):
    recs = [cases.ins_rec(0, 1000, 60), cases.ins_rec(1, 1003, 62)]
    alns, cig = pack(recs)
    sigs = cases.sigs_of(alns, cig)
    reads = cases.random_reads(recs)
    one = [cases.call(0, 1000, 60, [0, 1])]

    def refused(text, alns=alns, calls=one, sigs=sigs, opt=None, reads=reads, ic=None):
        with pytest.raises(TelrError) as e:
            engine_drafts(engine, ix, alns, cig, ic if ic is not None else as_ic(calls, sigs), reads, opt or {})
        assert e.value.code == TELR_E_ARG
        msg = engine.L.telr_last_error(engine.h)
        assert b"telr_draft_contigs" in msg and text in msg, msg

    for f in ("flank", "min_flank", "reach", "max_len", "reserved0", "reserved1", "reserved2", "reserved3"):
        refused(b"negative option", opt={f: -1} if f != "flank" else dict(flank=-1, min_flank=-2))
    refused(b"min_flank > flank", opt=dict(flank=10, min_flank=11))
    refused(b"not strictly ascending", calls=[cases.call(0, 1000, 60, [0]), cases.call(0, 1000, 60, [1])])
    refused(b"not strictly ascending", calls=[cases.call(1, 10, 60, [0]), cases.call(0, 999, 60, [1])])
    for tid in (2, -1):                                  # the index has two targets
        refused(b"tid", calls=[cases.call(tid, 1000, 60, [0])])
        refused(b"tid", sigs=[dict(sigs[0], tid=tid)] + sigs[1:])
    refused(b"rec outside", sigs=[dict(sigs[0], rec=2)] + sigs[1:])
    refused(b"rec outside", sigs=[dict(sigs[0], rec=-1)] + sigs[1:])
    refused(b"mate outside", sigs=[dict(sigs[0], kind=1, mate=2)] + sigs[1:])
    refused(b"mate outside", sigs=[dict(sigs[0], kind=1, mate=-1)] + sigs[1:])
    refused(b"qid outside", sigs=[dict(sigs[0], qid=2)] + sigs[1:])
    refused(b"qid is not", sigs=[dict(sigs[0], qid=1)] + sigs[1:])
    refused(b"signatures not ascending", sigs=sigs[::-1])
    for rd in ([1, 0], [1, 1]):
        ic = as_ic(one, sigs)
        ic.reads = np.array(rd, np.int32)
        refused(b"read list not ascending", ic=ic)
    refused(b"read id outside", calls=[cases.call(0, 1000, 60, [0, 2])])
    # records that telr_call_insertions refuses
    a2 = alns.copy(); a2["tid"] = 2
    refused(b"tid", alns=a2)
    a2 = alns.copy(); a2["te"] = 100
    refused(b"coordinates", alns=a2)
    # a read set whose count or lengths disagree with the records
    refused(b"qid outside the read set", reads=reads[:1], calls=[cases.call(0, 1000, 60, [0])])
    refused(b"qlen is not the length", reads=[reads[0], reads[1] + "A"])
    # the C entry itself: NULL arguments, and NULL options = the defaults
    qs = engine.seqset(reads)
    r = ix.result_from_arrays(alns, cig)
    try:
        ic = as_ic(one, sigs)
        h, hs = C.c_void_p(), C.c_void_p()
        L = engine.L
        args = (1, ic.calls.ctypes.data, ic.read_off.ctypes.data, ic.reads.ctypes.data, len(ic.sigs), ic.sigs.ctypes.data)
        assert L.telr_draft_contigs(engine.h, r, 0, *args, qs.h, None, C.byref(h), C.byref(hs)) == TELR_E_ARG
        assert L.telr_draft_contigs(engine.h, None, 2, *args, qs.h, None, C.byref(h), C.byref(hs)) == TELR_E_ARG
        assert L.telr_draft_contigs(engine.h, r, 2, *args, None, None, C.byref(h), C.byref(hs)) == TELR_E_ARG
        assert L.telr_draft_contigs(engine.h, r, 2, *args, qs.h, None, C.byref(h), C.byref(hs)) == 0
        # the default min_flank of 500 refuses the flanks of 20: a call without a draft, an empty set
        assert L.telr_drafts_count(h) == 1 and L.telr_seqset_count(hs) == 0
        got = np.frombuffer((C.c_char * 32).from_address(L.telr_drafts_data(h)), DRAFT_DTYPE)[0]
        assert (got["sig"], got["set_index"], got["len"]) == (-1, -1, 0)
        L.telr_draft_contigs_free(h); L.telr_seqset_free(hs)
    finally:
        ix.free_raw(r); qs.free()
    o = DraftOpt()
    engine.L.telr_draft_opt_default(C.byref(o))
    assert {k: getattr(o, k) for k in dref.DEFAULTS} == dref.DEFAULTS and (o.reserved0, o.reserved1, o.reserved2, o.reserved3) == (0, 0, 0, 0)
    with pytest.raises(TypeError):
        DraftOpt.default(nope=1)


# ---- behind a real map call ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(engine, data_dir):
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-pb")
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    fix = engine.index(ts, io)
    qset = engine.seqset(qs)
    r = fix.map_raw(qset, mo)
    yield dict(ix=fix, r=r, tn=tn, ts=ts, qn=qn, qs=qs, qset=qset, io=io)
    fix.free_raw(r)


def test_resident_cigars_and_uploaded_cigars_give_the_same(engine, bundled):
    b = bundled
    res = b["ix"].result_arrays(b["r"])
    twin = np.zeros(len(res.cigars) + 1, np.uint32)
    assert engine.L.telr_debug_result_twin(b["r"], twin.ctypes.data, len(twin)) == len(res.cigars)      # the result did keep its device copy
    ic = b["ix"].call_insertions(b["r"])
    d1, s1 = b["ix"].draft_contigs(b["r"], ic, b["qset"])
    r2 = b["ix"].result_from_arrays(res.alns, res.cigars)
    try:
        d2, s2 = b["ix"].draft_contigs(r2, ic, b["qset"])
    finally:
        b["ix"].free_raw(r2)
    assert len(d1) == 1 and d1["sig"][0] >= 0 and d1.tobytes() == d2.tobytes()
    for x, y in zip(s1.packed(), s2.packed()):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    s1.free(); s2.free()


def test_contig_set_in_one_call_and_in_two_halves(engine, bundled, monkeypatch):
    """polish_consensus(..., contig_set=...) indexes the resident drafts instead of the strings: the polished contigs equal those of the call
    without it, as ONE call (TELR_POLISH_HALVES=1) and as the two halves that 64 loci and more run as (each half a device subset of the set,
    the second on the worker context).  The loci differ in their reads, so a set taken in the wrong order would show."""
    b = bundled
    ic = b["ix"].call_insertions(b["r"])
    d, cset = b["ix"].draft_contigs(b["r"], ic, b["qset"])
    sup = ic.reads_of(0)
    assert len(sup) >= 12 and cset.n == 1
    n = 66
    draft = telr_assembly.draft_loci(b["ix"], b["r"], ic, [[b["tn"][0], str(int(ic.calls[0]["pos"])), str(int(ic.calls[0]["pos"]) + 1)] + [""] * 11],
                                     b["qset"], b["qs"], {b["tn"][0]: 0})[0][0]["contig"]
    # odd loci hold the draft cut short by 300 bases: a set in another order than the strings would polish another sequence
    both = engine.seqset([draft, draft[:-300]])
    cs = both.subset(np.arange(n, dtype=np.int32) % 2)
    contigs = [draft if k % 2 == 0 else draft[:-300] for k in range(n)]
    reads = [np.roll(sup, k)[:6].astype(np.int32) for k in range(n)]
    names = ["c%d" % k for k in range(n)]
    kw = dict(presets="pacbio", read_set=b["qset"], method="pileup")
    monkeypatch.setenv("TELR_POLISH_HALVES", "1")
    plain = telr_assembly.polish_consensus(engine, names, contigs, reads, **kw)
    one = telr_assembly.polish_consensus(engine, names, contigs, reads, contig_set=cs, **kw)
    monkeypatch.delenv("TELR_POLISH_HALVES")
    t = {}
    two = telr_assembly.polish_consensus(engine, names, contigs, reads, contig_set=cs, timings=t, **kw)
    assert "second_half_s" in t                      # the two-halves path ran
    assert len(plain) == len(one) == len(two) == n
    for k in range(n):
        assert plain[k] == one[k] == two[k], "locus %d" % k
    assert sum(x != y for x, y in zip(plain, contigs)) >= 60 and len(set(plain)) > 2        # polishing did something, and not the same thing everywhere
    # a set of another size is refused before anything is polished
    with pytest.raises(ValueError):
        locus_pipeline.run_loci(engine, None, [], None, [dict(name="a_1_2", contig=draft, alt="A", read_idx=sup)], [], [], read_set=b["qset"],
                                polish="pileup", contig_set=both)
    for x in (both, cs, cset):
        x.free()


def test_bundled_reads_end_to_end(engine, bundled, data_dir, tmp_path):
    """engine drafts == the checker over the oracle's records; draft_loci -> run_loci -> write_outputs.  Without polishing the bundle on the
    engine gives what the oracle-backend run of tests/test_draft_ref.py gives (annotation, liftover, AF: `unlifted`, no row).  With
    polish="poa" and the resident contig set it runs through the consensus kernels, which have no CPU counterpart, so it can NOT equal the
    oracle-backend run -- and does not: the polished draft lifts over.  SURVEY 4's known answer is asserted on it: one non-reference
    `jockey`, minus strand, inside 33,006-33,029, the AF, and the VCF / BED rows."""
    from oracle import binding as ob
    import test_draft_ref as cpu
    b = bundled
    _, mo = preset("map-pb")
    want = ob.OracleIndex(b["ts"], b["io"]).map(b["qs"], mo)
    sigs, calls = iref.call_insertions(want["alns"], want["cigars"])
    wd, wseq = dref.drafts(want["alns"], want["cigars"], calls, sigs, b["qs"])
    ic = b["ix"].call_insertions(b["r"])
    d, s = b["ix"].draft_contigs(b["r"], ic, b["qset"])
    w2, wn = s.packed()
    assert_equal_to_ref((d, s.len, w2.cpu().numpy().view(np.uint32), wn.cpu().numpy().view(np.uint32)), wd, wseq)
    s.free()
    assert {k: wd[0][k] for k in cpu.BUNDLED["map-pb"]} == cpu.BUNDLED["map-pb"]
    rows = telr_sv.call_insertions(b["ix"], b["r"], b["tn"], b["qn"], b["qs"], sample="s", genotype=True)
    loci, cset, skipped = telr_assembly.draft_loci(b["ix"], b["r"], ic, rows, b["qset"], b["qs"], {b["tn"][0]: 0})
    assert skipped == [] and len(loci) == 1 and cset.n == 1 and loci[0]["contig"] == wseq[0] and loci[0]["alt"] == rows[0][7]
    assert loci[0]["read_idx"].tolist() == list(range(18))
    ln, lib = read_fasta(data_dir + "/library.fasta")
    io10, _ = preset("asm10")
    ix10 = engine.index(b["ts"], io10)
    args = (engine, ix10, b["tn"], lambda ch: b["ts"][0], loci, ln, lib)
    o_locus, o_res = cpu.oracle_bundle(dict(b, **{"map-pb": want}), data_dir)
    assert o_locus["contig"] == loci[0]["contig"] and o_locus["alt"] == loci[0]["alt"]
    plain = locus_pipeline.run_loci(*args, presets="pacbio", read_set=b["qset"], contig_set=cset)
    again = locus_pipeline.run_loci(*args, presets="pacbio", read_set=b["qset"])
    for k in ("annotation", "liftover", "af"):
        assert plain[k] == o_res[k], k
        assert plain[k] == again[k], k
    # polished on the device from the resident set (measured on an MI355X: annotation at contig bases 2,018-6,531, the liftover at
    # chr2L:33,019-33,025 with a 6-base TSD, AF 0.74).  The asserted bounds are not those figures: the coordinate range is that of the
    # signatures (33,006-33,029); the AF lies between 13 supporters of 18 window reads (0.72, every other read counted as
    # reference) and 13 of the 16 reads the genotyper counts (0.81), with 0.1 either side for the S6 step's own coverage arithmetic.
    res = locus_pipeline.run_loci(*args, presets="pacbio", read_set=b["qset"], polish="poa", contig_set=cset)
    print(res["annotation"], [x["report"] for x in res["liftover"]], res["af"])
    name = loci[0]["name"]
    assert len(res["annotation"]) == 1 and res["annotation"][0][0] == name and res["annotation"][0][3:6] == ["jockey", ".", "-"]
    assert len(res["liftover"]) == 1
    rep = res["liftover"][0]["report"]
    assert (rep["type"], rep["family"], rep["chrom"], rep["strand"]) == ("non-reference", "jockey", "chr2L", "-")
    assert 33006 <= rep["start"] <= rep["end"] <= 33029
    assert list(res["af"]) == [name] and 13 / 18 - 0.1 <= res["af"][name]["freq"] <= 13 / 16 + 0.1
    assert res["contigs"][name] != loci[0]["contig"] and abs(len(res["contigs"][name]) - len(loci[0]["contig"])) < 0.1 * len(loci[0]["contig"])
    ref_fa = tmp_path / "ref.fa"
    ref_fa.write_text(">%s\n%s\n" % (b["tn"][0], b["ts"][0]))
    loci_out = [dict(l, contig=res["contigs"][l["name"]]) for l in loci]
    final, _ = locus_pipeline.write_outputs(res, loci_out, str(tmp_path), "s", str(ref_fa), sv_info=telr_sv.sv_info(rows), today="DATE")
    assert len(final) == 1
    f = final[0]
    assert (f["type"], f["chrom"], f["start"], f["end"], f["family"], f["strand"]) == ("non-reference", "chr2L", rep["start"], rep["end"], "jockey", "-")
    assert (f["genotype"], f["num_ref_reads"], f["num_sv_reads"]) == ("1/1", "3", "13") and f["allele_frequency"] == res["af"][name]["freq"]
    body = [l.split("\t") for l in (tmp_path / "s.telr.vcf").read_text().splitlines() if not l.startswith("#")]
    assert len(body) == 1 and body[0][0] == "chr2L" and 33006 <= int(body[0][1]) <= 33030 and body[0][-2] == "GT:DR:DV"
    bed = [l.split("\t") for l in (tmp_path / "s.telr.bed").read_text().splitlines()]
    assert len(bed) == 1 and (bed[0][0], int(bed[0][1]), int(bed[0][2]), bed[0][3], bed[0][5]) == ("chr2L", rep["start"], rep["end"], "jockey", "-")
    cset.free()
