"""telr_call_at_sites on the device == its definition in plain Python (tests/sitecall_ref.py), array for array: the calls, one per site,
the kept signatures, the offsets and the read-id lists.  Records are built by hand and wrapped with result_from_arrays, so every edge
is exact; then the bundled reads mapped by the engine, telr_sv.genotype_sites with DESIGN.md 5.19's table, and `telr --sites`."""
import ctypes as C
import os

import numpy as np
import pytest

import genotype_ref as gref
import inscall_cases as icases
import inscall_ref as iref
import sitecall_cases as cases
import sitecall_ref as sref
from telr_amd import telr, telr_sv
from telr_amd._abi import InsOpt, SiteOpt, MF_KEEP_CIGARS, TELR_E_ARG, TELR_E_RANGE, INS_SIG_DTYPE, INS_CALL_DTYPE
from telr_amd._lib import TelrError
from telr_amd.aligner import Engine
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()
REFUSALS = cases.refusals()
TARGETS = ["ACGT" * 64, "TTGCA" * 64, "GGCAT" * 64]          # the entry only needs their number
SITES = [(0, 20000, 0), (0, 33022, 4562), (0, 33100, 0), (0, 37990, 0)]


@pytest.fixture(scope="module")
def ix(engine):
    io, _ = preset("map-ont")
    assert len(TARGETS) == cases.N_TARGETS
    return engine.index(TARGETS, io)


@pytest.fixture(scope="module")
def generated():
    """the generated case, packed, with the checker's answer: made once, shared, left unchanged"""
    recs, sites, opt, sopt = cases.generated()
    alns, cig = icases.pack(recs)
    kept, calls = sref.call_at_sites(alns, cig, sites, opt, sopt)
    return dict(alns=alns, cig=cig, sites=sites, opt=opt, sopt=sopt, kept=kept, calls=calls)


def engine_sites(ix, alns, cig, sites, opt, sopt):
    r = ix.result_from_arrays(alns, cig)
    try:
        return ix.call_at_sites(r, sites, InsOpt.default(**opt), SiteOpt.default(**sopt))
    finally:
        ix.free_raw(r)


def assert_equal_to_ref(ic, kept, calls):
    assert ic.sigs.dtype == INS_SIG_DTYPE and ic.calls.dtype == INS_CALL_DTYPE
    assert len(ic.sigs) == len(kept)
    for f in iref.SIG_FIELDS:
        np.testing.assert_array_equal(ic.sigs[f], np.array([s[f] for s in kept], np.int64), err_msg="kept signature " + f)
    assert len(ic.calls) == len(calls)
    for f in iref.CALL_FIELDS:
        np.testing.assert_array_equal(ic.calls[f], np.array([c[f] for c in calls], np.int64), err_msg="call " + f)
    off = np.zeros(len(calls) + 1, np.int64)
    off[1:] = np.cumsum([len(c["reads"]) for c in calls])
    np.testing.assert_array_equal(ic.read_off, off)
    np.testing.assert_array_equal(ic.reads, np.array([q for c in calls for q in c["reads"]], np.int64))


def blob(ic):
    return ic.sigs.tobytes() + ic.calls.tobytes() + ic.read_off.tobytes() + ic.reads.tobytes()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(ix, case):
    _, recs, sites, opt, sopt, want_kept, want_calls = case
    alns, cig = icases.pack(recs)
    kept, calls = sref.call_at_sites(alns, cig, sites, opt, sopt)
    assert [(s["pos"], s["qid"], s["kind"], s["len"]) for s in kept] == want_kept and calls == want_calls      # the checker's answer is the hand-derived one
    assert_equal_to_ref(engine_sites(ix, alns, cig, sites, opt, sopt), kept, calls)


def test_generated_case(ix, generated):
    g = generated
    assert len(g["kept"]) > 4096 and len(g["calls"]) == 700
    assert_equal_to_ref(engine_sites(ix, g["alns"], g["cig"], g["sites"], g["opt"], g["sopt"]), g["kept"], g["calls"])
    # without the length test, and with one site only (n_sites - 1 has no bits)
    for sites, sopt in ((g["sites"], dict(reach=50)), (g["sites"][40:41], g["sopt"]), (g["sites"][:257], dict(reach=0))):
        kept, calls = sref.call_at_sites(g["alns"], g["cig"], sites, g["opt"], sopt)
        assert_equal_to_ref(engine_sites(ix, g["alns"], g["cig"], sites, g["opt"], sopt), kept, calls)


def test_same_output_on_every_run(ix, generated):
    g = generated
    a = engine_sites(ix, g["alns"], g["cig"], g["sites"], g["opt"], g["sopt"])
    b = engine_sites(ix, g["alns"], g["cig"], g["sites"], g["opt"], g["sopt"])
    assert blob(a) == blob(b) and len(a.sigs) > 4096


def test_growing_and_shrinking_inputs_equal_fresh_engines(engine, ix, generated):
    """small, large, small, nothing kept, large with few sites, small again through one context's buffers: each equals the call on a fresh engine"""
    g = generated
    small = next(c for c in HAND if c[0] == "equidistant_and_close_sites")
    none = next(c for c in HAND if c[0] == "nothing_kept")
    s_in = icases.pack(small[1]) + (small[2], small[3], small[4])
    n_in = icases.pack(none[1]) + (none[2], none[3], none[4])
    big = (g["alns"], g["cig"], g["sites"], g["opt"], g["sopt"])
    few = (g["alns"], g["cig"], g["sites"][100:103], g["opt"], g["sopt"])
    steps = [s_in, big, s_in, n_in, few, s_in]
    got = [blob(engine_sites(ix, *x)) for x in steps]
    assert got[0] == got[2] == got[5]
    io, _ = preset("map-ont")
    for k in (0, 1, 3, 4):
        fresh = Engine(0)
        fix = fresh.index(TARGETS, io)
        try:
            assert blob(engine_sites(fix, *steps[k])) == got[k], "step %d" % k
        finally:
            fix.free(); fresh.close()


def test_discovery_is_untouched_by_a_site_call(ix, generated):
    g = generated
    r = ix.result_from_arrays(g["alns"], g["cig"])
    try:
        opt = InsOpt.default(min_support=3)
        before = ix.call_insertions(r, opt)
        at = ix.call_at_sites(r, g["sites"], None, SiteOpt.default(**g["sopt"]))
        after = ix.call_insertions(r, opt)
    finally:
        ix.free_raw(r)
    assert len(before.calls) > 10 and len(at.calls) == 700
    assert blob(before) == blob(after)
    sigs, calls = iref.call_insertions(g["alns"], g["cig"], dict(min_support=3))
    assert len(before.sigs) == len(sigs) and before.calls["pos"].tolist() == [c["pos"] for c in calls]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal(engine, ix, case):
    name, recs, sites, opt, sopt, n_sites, code = case
    alns, cig = icases.pack(recs)
    r = ix.result_from_arrays(alns, cig)
    try:
        if n_sites is None:
            with pytest.raises(TelrError) as e:
                ix.call_at_sites(r, sites, InsOpt.default(**opt), SiteOpt.default(**sopt))
            assert e.value.code == code
        else:       # a count that is not the array's: the raw entry.  Refused by the count alone: the array is not read
            s = np.ascontiguousarray(np.array(sites if sites is not None else [(0, 0, 0)], np.int32).reshape(-1, 3))
            h = C.c_void_p()
            assert engine.L.telr_call_at_sites(engine.h, r, cases.N_TARGETS, None, s.ctypes.data if sites is not None else None, n_sites, None, C.byref(h)) == code
            assert not h.value
        assert b"telr_call_at_sites" in engine.L.telr_last_error(engine.h)
    finally:
        ix.free_raw(r)


def test_null_arguments_and_defaults(engine, ix):
    r = ix.result_from_arrays(*icases.pack([icases.simple(0, 1000, 60)]))
    s = np.array([(0, 1000, 0)], np.int32)
    try:
        h = C.c_void_p()
        L = engine.L
        assert L.telr_call_at_sites(engine.h, None, 3, None, s.ctypes.data, 1, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_call_at_sites(engine.h, r, 0, None, s.ctypes.data, 1, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_call_at_sites(engine.h, r, 3, None, s.ctypes.data, 1, None, None) == TELR_E_ARG
        assert L.telr_call_at_sites(engine.h, r, 3, None, s.ctypes.data, 1, None, C.byref(h)) == 0          # NULL options = the defaults
        assert L.telr_ins_calls_count(h) == 1 and L.telr_ins_calls_sig_count(h) == 1
        L.telr_ins_calls_free(h)
        assert L.telr_call_at_sites(engine.h, r, 3, None, None, 0, None, C.byref(h)) == 0                     # no sites: no array needed
        assert L.telr_ins_calls_count(h) == 0 and L.telr_ins_calls_sig_count(h) == 0
        L.telr_ins_calls_free(h)
    finally:
        ix.free_raw(r)
    o = SiteOpt(7, 7, 7, 7)
    engine.L.telr_site_opt_default(C.byref(o))
    assert (o.reach, o.len_pct, o.reserved0, o.reserved1) == (50, 0, 0, 0) == tuple(getattr(SiteOpt.default(), k) for k, _ in SiteOpt._fields_)
    assert TELR_E_ARG == sref.E_ARG and TELR_E_RANGE == sref.E_RANGE


# ---- behind a real map call ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(engine, data_dir):
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    out = {}
    for name in ("map-pb", "ngmlr-pacbio", "map-ont"):
        io, mo = preset(name)
        mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
        fix = engine.index(ts, io)
        out[name] = dict(ix=fix, r=fix.map_raw(qs, mo), tn=tn, qn=qn)
    yield out
    for b in out.values():
        b["ix"].free_raw(b["r"])


@pytest.mark.parametrize("name", ("map-pb", "ngmlr-pacbio", "map-ont"))
@pytest.mark.parametrize("len_pct", (0, 2))
def test_bundled_reads_equal_the_checker_and_genotype(bundled, name, len_pct):
    b = bundled[name]
    res = b["ix"].result_arrays(b["r"])
    sopt = dict(len_pct=len_pct)
    kept, calls = sref.call_at_sites(res.alns, res.cigars, SITES, None, sopt)
    ic = b["ix"].call_at_sites(b["r"], SITES, None, SiteOpt.default(**sopt))
    assert_equal_to_ref(ic, kept, calls)
    assert calls[1]["support"] >= 10 and calls[0]["support"] == 0
    # the site result is what the genotyper takes, unchanged
    ig = b["ix"].genotype_insertions(b["r"], ic)
    want = gref.genotype(res.alns, res.cigars, calls)
    for f in gref.GT_FIELDS:
        np.testing.assert_array_equal(ig.gt[f], np.array([g[f] for g in want], np.int64), err_msg=f)
    for k, g in enumerate(want):
        assert ig.ref_reads_of(k).tolist() == g["ref_reads"] and ig.ambig_reads_of(k).tolist() == g["ambig_reads"]
    assert ig.gt["gt"][0] == 2 and want[0]["alt"] + want[0]["ref"] == 0          # the empty genotype stays the genotyper's 2


# preset: (support, n_sized, len, gt, af at 33,022), (ref, ambig at 33,100): DESIGN.md 5.19
TABLE = {"map-pb": ((13, 6, 4562), (9, 1)), "ngmlr-pacbio": ((13, 6, 4564), (10, 0)), "map-ont": ((12, 5, 4586), (8, 1))}


@pytest.mark.parametrize("name", ("map-pb", "ngmlr-pacbio", "map-ont"))
def test_genotype_sites_gives_the_tables_texts(bundled, name):
    b = bundled[name]
    rows = telr_sv.genotype_sites(b["ix"], b["r"], b["tn"], b["qn"], SITES)
    (sup, nsz, ln), (ref100, amb100) = TABLE[name]
    assert [tuple(r) for r in rows] == [telr_sv.SITE_FIELDS] * 4
    assert [(r["chrom"], r["pos"], r["site_len"]) for r in rows] == [("chr2L", p, l) for _, p, l in SITES]
    print(name, [{k: v for k, v in r.items() if k != "reads"} for r in rows])
    assert (rows[0]["support"], rows[0]["ref"], rows[0]["ambig"], rows[0]["gt_text"], rows[0]["af_text"], rows[0]["reads"]) == (0, 0, 0, "./.", "nan", [])
    assert (rows[1]["support"], rows[1]["n_sized"], rows[1]["len"], rows[1]["ref"], rows[1]["ambig"]) == (sup, nsz, ln, 3, 1)
    assert (rows[1]["gt_text"], rows[1]["af_text"]) == ("1/1", "%.6f" % (sup / (sup + 3))) and len(rows[1]["reads"]) == sup
    assert rows[1]["reads"] == sorted(rows[1]["reads"], key=b["qn"].index) and set(rows[1]["reads"]) <= set(b["qn"])
    assert (rows[2]["support"], rows[2]["ref"], rows[2]["ambig"], rows[2]["gt_text"], rows[2]["af_text"]) == (0, ref100, amb100, "0/0", "0.000000")
    assert (rows[3]["support"], rows[3]["n_sized"], rows[3]["len"], rows[3]["ref"], rows[3]["gt_text"], rows[3]["af_text"]) == (6, 0, 0, 0, "1/1", "1.000000")
    if name == "map-ont":
        r2 = telr_sv.genotype_sites(b["ix"], b["r"], b["tn"], b["qn"], np.array(SITES, np.int32), site_opt=SiteOpt.default(len_pct=2))
        assert (r2[1]["support"], r2[1]["n_sized"], r2[1]["ambig"], r2[1]["gt_text"]) == (10, 3, 3, "0/1")


# ---- the command -----------------------------------------------------------------------------------------------------------------
MM2 = ("--aligner", "minimap2", "-x", "pacbio")


def argv_for(data_dir, reads, out, *extra):
    return ["-i", reads, "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out)] + list(extra)


def data_lines(path):
    return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("#")]


@pytest.fixture(scope="module")
def normal_run(engine, data_dir, tmp_path_factory):
    """a run without --sites, intermediate files kept: its VCF and its BAM are the inputs below"""
    out = tmp_path_factory.mktemp("telr_normal")
    return telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", out, *MM2, "-k")), engine=engine), out


def test_a_run_without_sites_writes_what_it_wrote(normal_run):
    res, out = normal_run
    assert set(res["files"]) == {"vcf", "bed", "json", "expanded.json", "te.fasta", "contig.fasta", "locus_table", "bam"}
    assert set(res["counts"]) == {"reads", "records", "calls", "calls_without_draft", "loci_annotated", "loci_lifted", "loci_written"} and "sites" not in res
    assert set(res["seconds"]) == {"inputs", "index", "reads", "calls", "drafts", "index10", "loci", "outputs"}
    assert sorted(p.name for p in out.iterdir()) == sorted(["intermediate_files"] + ["reads.telr." + k for k in ("vcf", "bed", "json", "expanded.json", "te.fasta", "contig.fasta")])
    assert len(data_lines(res["files"]["vcf"])) == 1


def test_sites_from_the_vcf_of_a_normal_run(engine, data_dir, normal_run, tmp_path, capfd):
    res, _ = normal_run
    got = telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", tmp_path, *MM2, "--sites", res["files"]["vcf"], "--polish", "poa", "--bridge",
                                          "--sample", "B")), engine=engine)
    err = capfd.readouterr().err
    assert err.count("no effect with --sites") == 1 and "--polish, --bridge have no effect" in err and "[telr] sites" in err
    assert (got["counts"]["sites"], got["counts"]["sites_supported"], got["counts"]["reads"], got["counts"]["calls"]) == (1, 1, 18, 0)
    assert set(got["seconds"]) == {"inputs", "index", "reads", "sites", "outputs"} and got["final"] == []
    assert sorted(p.name for p in tmp_path.iterdir()) == ["B.telr.sites.tsv", "B.telr.sites.vcf"]
    src, dst = data_lines(res["files"]["vcf"]), data_lines(got["files"]["sites_vcf"])
    assert len(dst) == 1 and dst[0][:8] == src[0][:8] and dst[0][8:] == ["GT:DR:DV", "1/1:3:13"]
    head = [l for l in open(got["files"]["sites_vcf"]).read().splitlines() if l.startswith("#")]
    assert head[:-1] == [l for l in open(res["files"]["vcf"]).read().splitlines() if l.startswith("##")] and head[-1].split("\t")[-1] == "B"
    row = got["sites"][0]
    assert (row["gt_text"], row["support"], row["ref"], row["pos"]) == ("1/1", 13, 3, int(src[0][1]) - 1) and row["site_len"] == len(src[0][4])
    tsv = data_lines(got["files"]["sites_tsv"])
    assert len(tsv) == 1 and len(tsv[0]) == 1 + len(telr_sv.SITE_FIELDS) and tsv[0][:3] == [src[0][2], "chr2L", str(row["pos"])]


def test_sites_from_a_tsv_on_both_routes(engine, data_dir, normal_run, tmp_path):
    res, _ = normal_run
    tsv = tmp_path / "four.tsv"
    tsv.write_text("".join("chr2L\t%d\t%d\n" % (p, l) for _, p, l in SITES))
    a = telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", tmp_path / "a", *MM2, "--sites", str(tsv))), engine=engine)
    assert (a["counts"]["sites"], a["counts"]["sites_supported"]) == (4, 2) and "sites_vcf" not in a["files"]
    assert [(r["support"], r["ref"], r["gt_text"]) for r in a["sites"]] == [(0, 0, "./."), (13, 3, "1/1"), (0, 9, "0/0"), (6, 0, "1/1")]
    lines = data_lines(a["files"]["sites_tsv"])
    assert [l[7:11] for l in lines] == [[str(r["ref"]), str(r["ambig"]), r["gt_text"], r["af_text"]] for r in a["sites"]] and lines[0][-1] == "."
    assert not (tmp_path / "a" / "intermediate_files").exists()
    # the BAM route on the BAM the normal run kept: the same counts (the read numbering may differ, the counts do not)
    b = telr.run(telr.get_args(argv_for(data_dir, res["files"]["bam"], tmp_path / "b", *MM2, "--sites", str(tsv))), engine=engine)
    assert b["counts"] == a["counts"]
    assert [{k: v for k, v in r.items() if k != "reads"} for r in b["sites"]] == [{k: v for k, v in r.items() if k != "reads"} for r in a["sites"]]
    assert [sorted(r["reads"]) for r in b["sites"]] == [sorted(r["reads"]) for r in a["sites"]]


def test_a_bad_site_list_ends_the_run_before_mapping(engine, data_dir, tmp_path):
    tsv = tmp_path / "bad.tsv"
    tsv.write_text("chrX\t5\n")
    with pytest.raises(ValueError, match="chrX"):
        telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", tmp_path / "o", *MM2, "--sites", str(tsv))), engine=engine)
