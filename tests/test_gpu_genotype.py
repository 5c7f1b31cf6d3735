"""telr_genotype_insertions on the device == its definition in plain Python (tests/genotype_ref.py), array for array: the per-call
counts and GT and both read lists.  Records and calls are built by hand and wrapped with result_from_arrays, so every edge is exact;
the last tests run the step behind a real map call and the caller (the bundled reads)."""
import ctypes as C
import types

import numpy as np
import pytest

import genotype_cases as cases
import genotype_ref as gref
import inscall_ref as iref
from telr_amd import locus_pipeline, telr_sv
from telr_amd._abi import GenoOpt, MF_KEEP_CIGARS, TELR_E_ARG, TELR_E_RANGE, ALN_DTYPE, INS_CALL_DTYPE, GENO_DTYPE
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()
EDGES = cases.gpu_cases()


@pytest.fixture(scope="module")
def ix(engine):
    """the step only needs the number of targets: two short ones"""
    io, _ = preset("map-ont")
    return engine.index(["ACGT" * 64, "TTGCA" * 64], io)


def as_ic(calls):
    """checker-style calls -> what Index.genotype_insertions takes"""
    a = np.zeros(len(calls), INS_CALL_DTYPE)
    for k, c in enumerate(calls):
        for f in ("tid", "pos", "len", "support", "n_sized", "rep"):
            a[k][f] = c[f]
    off = np.zeros(len(calls) + 1, np.int64)
    off[1:] = np.cumsum([len(c["reads"]) for c in calls])
    reads = np.array([q for c in calls for q in c["reads"]], np.int32)
    return types.SimpleNamespace(calls=a, read_off=off, reads=reads)


def engine_geno(ix, alns, cig, calls, opt):
    """calls: checker-style dicts, or the arrays themselves"""
    r = ix.result_from_arrays(alns, cig)
    try:
        return ix.genotype_insertions(r, calls if isinstance(calls, types.SimpleNamespace) else as_ic(calls), GenoOpt.default(**opt))
    finally:
        ix.free_raw(r)


def assert_equal_to_ref(ig, want):
    assert ig.gt.dtype == GENO_DTYPE and len(ig.gt) == len(want)
    for f in gref.GT_FIELDS:
        np.testing.assert_array_equal(ig.gt[f], np.array([g[f] for g in want], np.int64), err_msg=f)
    assert len(ig.ref_off) == len(ig.ambig_off) == len(want) + 1 and ig.ref_off[0] == 0 and ig.ambig_off[0] == 0
    for k, g in enumerate(want):
        assert ig.ref_reads_of(k).tolist() == g["ref_reads"], "reference reads of call %d" % k
        assert ig.ambig_reads_of(k).tolist() == g["ambig_reads"], "ambiguous reads of call %d" % k
    assert int(ig.ref_off[-1]) == len(ig.ref_reads) and int(ig.ambig_off[-1]) == len(ig.ambig_reads)


def check(ix, recs, calls, opt, exact=False):
    """exact: also at max_window_indel = every window indel the checker met (the three smallest and the three largest) and one below it, so that the
    device's sum is held to the base, not only to one side of the case's threshold"""
    alns, cig = cases.pack(recs)
    want = gref.genotype(alns, cig, calls, opt)
    assert_equal_to_ref(engine_geno(ix, alns, cig, calls, opt), want)
    if exact:
        seen = sorted(set(w for g in want for ws in g["indels"].values() for w in ws))
        assert seen
        for w in sorted(set(seen[:3] + seen[-3:])):
            for t in (w, w - 1):
                if t >= 0:
                    o = dict(opt, max_window_indel=t)
                    assert_equal_to_ref(engine_geno(ix, alns, cig, calls, o), gref.genotype(alns, cig, calls, o))
    return want


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(ix, case):
    _, recs, calls, opt, hand = case
    want = check(ix, recs, calls, opt)
    assert [{k: g[k] for k in hand[0]} for g in want] == hand          # (and the checker's answer is the hand-derived one)


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_edge_case(ix, case):
    name, recs, calls, opt = case
    want = check(ix, recs, calls, opt, exact=name.startswith("ops_") or name == "inside_long_del")
    assert sum(g["ref"] + g["ambig"] for g in want) > 0
    if name == "span_4100":
        assert sum(1 for g in want if 0 in g["ref_reads"]) == 4100 > 4096
    if name == "reads_2100":
        assert want[0]["ref"] + want[0]["ambig"] > 2048 and want[0]["ambig"] > 0 and want[0]["ref"] > 0
    if name == "ops_100k":
        assert len(recs[0]["cig"]) > 100000 and all(0 in g["indels"] for g in want)
    if name == "inside_long_del":
        assert want[0]["indels"][0] == [100]


def test_many_pairs(ix):
    recs, calls, opt = cases.many_pairs()
    want = check(ix, recs, calls, opt)
    assert sum(len(ws) for g in want for ws in g["indels"].values()) > 65536
    assert any(g["ambig"] for g in want)


def test_zero_calls_and_calls_without_spanning_records(ix):
    alns, cig = cases.pack([cases.flat(0, 900, 1100)])
    ig = engine_geno(ix, alns, cig, [], {})
    assert len(ig.gt) == 0 and ig.ref_off.tolist() == [0] and ig.ambig_off.tolist() == [0] and len(ig.ref_reads) == 0 and len(ig.ambig_reads) == 0
    calls = [cases.call(0, 5000, cases.SUP), cases.call(1, 1000, [7])]
    for recs in ([cases.flat(0, 900, 1100)], [], [cases.flat(0, 4000, 6000, mapq=3)]):
        alns, cig = cases.pack(recs)
        ig = engine_geno(ix, alns, cig, calls, {})
        assert_equal_to_ref(ig, gref.genotype(alns, cig, calls))
        assert ig.gt["ref"].tolist() == [0, 0] and ig.gt["ambig"].tolist() == [0, 0] and ig.gt["alt"].tolist() == [3, 1] and ig.gt["gt"].tolist() == [2, 2]
        assert ig.ref_off.tolist() == [0, 0, 0] and ig.ambig_off.tolist() == [0, 0, 0]


def test_same_output_on_every_run(ix):
    recs, calls, opt = cases.many_pairs()
    alns, cig = cases.pack(recs)
    a = engine_geno(ix, alns, cig, calls, opt)
    b = engine_geno(ix, alns, cig, calls, opt)
    for f in ("gt", "ref_off", "ref_reads", "ambig_off", "ambig_reads"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


def test_argument_errors(ix, engine):
    alns, cig = cases.pack([cases.flat(0, 900, 1100)])
    one = [cases.call(0, 1000, cases.SUP)]

    def refused(alns, cig, calls, opt, text):
        with pytest.raises(TelrError) as e:
            engine_geno(ix, alns, cig, calls, opt)
        assert e.value.code == TELR_E_ARG
        msg = engine.L.telr_last_error(engine.h)
        assert b"telr_genotype_insertions" in msg and text in msg, msg

    for bad in (dict(flank=-1), dict(min_mapq=-1), dict(max_window_indel=-1), dict(het_pct=-1), dict(hom_pct=-1, het_pct=-2), dict(reserved0=-1),
                dict(reserved1=-1), dict(reserved2=-1)):
        refused(alns, cig, one, bad, b"negative option")
    refused(alns, cig, one, dict(het_pct=81), b"het_pct > hom_pct")
    refused(alns, cig, one, dict(hom_pct=101), b"above 100")
    refused(alns, cig, one, dict(het_pct=101, hom_pct=101), b"above 100")
    # calls not strictly ascending: equal, descending position, descending target
    refused(alns, cig, [cases.call(0, 1000, [1]), cases.call(0, 1000, [2])], {}, b"not strictly ascending")
    refused(alns, cig, [cases.call(0, 1000, [1]), cases.call(0, 999, [2])], {}, b"not strictly ascending")
    refused(alns, cig, [cases.call(1, 10, [1]), cases.call(0, 999, [2])], {}, b"not strictly ascending")
    for tid in (2, -1):                                  # the index has two targets
        refused(alns, cig, [cases.call(tid, 1000, [1])], {}, b"tid")
    # a read list that is not ascending, or not distinct (as_ic would sort it: built here)
    for reads in ([5, 4], [4, 4]):
        ic = as_ic(one)
        ic.read_off = np.array([0, 2], np.int64); ic.reads = np.array(reads, np.int32)
        refused(alns, cig, ic, {}, b"read list not ascending")
    # records that telr_call_insertions refuses
    a2 = alns.copy(); a2["tid"] = 2
    refused(a2, cig, one, {}, b"tid")
    a2 = alns.copy(); a2["te"] = 100
    refused(a2, cig, one, {}, b"coordinates")
    # (a CIGAR range outside the array cannot be wrapped: result_from_arrays refuses it first)
    # the C entry itself: NULL arguments, and NULL options = the defaults
    r = ix.result_from_arrays(alns, cig)
    try:
        ic = as_ic(one)
        h = C.c_void_p()
        args = (1, ic.calls.ctypes.data, ic.read_off.ctypes.data, ic.reads.ctypes.data)
        assert engine.L.telr_genotype_insertions(engine.h, r, 0, *args, None, C.byref(h)) == TELR_E_ARG
        assert engine.L.telr_genotype_insertions(engine.h, None, 2, *args, None, C.byref(h)) == TELR_E_ARG
        assert engine.L.telr_genotype_insertions(engine.h, r, 2, 1, None, None, None, None, C.byref(h)) == TELR_E_ARG
        assert engine.L.telr_genotype_insertions(engine.h, r, 2, *args, None, C.byref(h)) == 0
        assert engine.L.telr_ins_geno_count(h) == 1
        got = np.frombuffer((C.c_char * 16).from_address(engine.L.telr_ins_geno_gt(h)), GENO_DTYPE)[0]
        assert (got["ref"], got["ambig"], got["alt"], got["gt"]) == (1, 0, 3, 1)
        engine.L.telr_ins_geno_free(h)
    finally:
        ix.free_raw(r)
    o = GenoOpt()
    engine.L.telr_geno_opt_default(C.byref(o))
    assert {k: getattr(o, k) for k in gref.DEFAULTS} == gref.DEFAULTS and (o.reserved0, o.reserved1, o.reserved2) == (0, 0, 0)


def test_null_options_are_the_defaults(ix):
    """a window indel of 20 is clean and one of 21 is not, a mapq of 19 is out: the documented defaults, through the Python default"""
    recs = [cases.with_ins(0, 900, 1100, 1000, 20), cases.with_ins(1, 900, 1100, 1000, 21), cases.flat(2, 900, 1100, mapq=19), cases.flat(3, 951, 1100)]
    alns, cig = cases.pack(recs)
    r = ix.result_from_arrays(alns, cig)
    try:
        ig = ix.genotype_insertions(r, as_ic([cases.call(0, 1000, cases.SUP)]))
    finally:
        ix.free_raw(r)
    assert ig.ref_reads.tolist() == [0] and ig.ambig_reads.tolist() == [1]


def test_too_many_pairs_is_a_range_error(ix, engine):
    """50,000 records that each span 50,000 calls: 2.5e9 pairs, found by the count pass; nothing is allocated for them"""
    n = 50000
    alns = np.zeros(n, ALN_DTYPE)
    alns["qid"] = np.arange(n); alns["qlen"] = 100; alns["qe"] = 100; alns["te"] = 1 << 30; alns["tlen"] = 1 << 30; alns["mapq"] = 60
    ic = types.SimpleNamespace(calls=np.zeros(n, INS_CALL_DTYPE), read_off=np.zeros(n + 1, np.int64), reads=np.zeros(0, np.int32))
    ic.calls["pos"] = 1000 + 10 * np.arange(n)
    r = ix.result_from_arrays(alns, np.zeros(0, np.uint32))
    try:
        with pytest.raises(TelrError) as e:
            ix.genotype_insertions(r, ic)
    finally:
        ix.free_raw(r)
    assert e.value.code == TELR_E_RANGE and b"telr_genotype_insertions" in engine.L.telr_last_error(engine.h)


# ---- behind a real map call ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(engine, data_dir):
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-pb")
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    fix = engine.index(ts, io)
    r = fix.map_raw(qs, mo)
    yield dict(ix=fix, r=r, tn=tn, ts=ts, qn=qn, qs=qs, io=io)
    fix.free_raw(r)


def test_resident_cigars_and_uploaded_cigars_give_the_same(engine, bundled):
    b = bundled
    res = b["ix"].result_arrays(b["r"])
    twin = np.zeros(len(res.cigars) + 1, np.uint32)
    assert engine.L.telr_debug_result_twin(b["r"], twin.ctypes.data, len(twin)) == len(res.cigars)      # the result did keep its device copy
    ic = b["ix"].call_insertions(b["r"])
    a = b["ix"].genotype_insertions(b["r"], ic)
    r2 = b["ix"].result_from_arrays(res.alns, res.cigars)
    try:
        c = b["ix"].genotype_insertions(r2, ic)
    finally:
        b["ix"].free_raw(r2)
    assert len(a.gt) == 1 and a.gt["ref"][0] > 0
    for f in ("gt", "ref_off", "ref_reads", "ambig_off", "ambig_reads"):
        assert getattr(a, f).tobytes() == getattr(c, f).tobytes()


def test_bundled_reads_end_to_end(engine, bundled, tmp_path):
    from oracle import binding as ob
    b = bundled
    _, mo = preset("map-pb")
    want = ob.OracleIndex(b["ts"], b["io"]).map(b["qs"], mo)
    _, calls = iref.call_insertions(want["alns"], want["cigars"])
    g = gref.genotype(want["alns"], want["cigars"], calls)
    ic = b["ix"].call_insertions(b["r"])
    ig = b["ix"].genotype_insertions(b["r"], ic)
    assert_equal_to_ref(ig, g)
    assert g[0]["ref_reads"] == [1, 5, 12] and g[0]["ambig_reads"] == [6] and (g[0]["alt"], g[0]["gt"]) == (13, 2)
    args = (b["ix"], b["r"], b["tn"], b["qn"], b["qs"])
    rows = telr_sv.call_insertions(*args, sample="s", genotype=True)
    assert len(rows) == 1 and (rows[0][5], rows[0][10], rows[0][11]) == ("0.812500", "1/1", "3")
    assert telr_sv.call_insertions(*args, sample="s", genotype=GenoOpt.default()) == rows
    # without the keyword, and with None, the rows are what they were: the three placeholders, everything else as with genotype=True
    plain = telr_sv.call_insertions(*args, sample="s")
    assert plain == telr_sv.call_insertions(*args, sample="s", genotype=None)
    assert (plain[0][5], plain[0][10], plain[0][11]) == ("nan", "./.", "NA")
    assert [v for i, v in enumerate(plain[0]) if i not in (5, 10, 11)] == [v for i, v in enumerate(rows[0]) if i not in (5, 10, 11)]
    # a stricter window turns the three reference reads (4-7 indel bases) ambiguous: AF 13 / 13
    strict = telr_sv.call_insertions(*args, sample="s", genotype=GenoOpt.default(max_window_indel=3))
    assert (strict[0][5], strict[0][10], strict[0][11]) == ("1.000000", "1/1", "0")
    # the rows still merge, and sv_info feeds write_outputs: GT:DR:DV of the VCF is the genotype's
    assert telr_sv.merge_rows(rows)[0][10:13] == ["1/1", "3", "13"]
    info = telr_sv.sv_info(rows)
    name = telr_sv.locus_name(rows[0])
    assert info == {name: ("1/1", "3", "13")}
    contig = "ACGT" * 50
    rep = dict(type="non-reference", chrom=rows[0][0], start=int(rows[0][1]), end=int(rows[0][2]), family="jockey", strand="+", TSD_length=None,
               TSD_sequence=None, gap=0)
    from telr_amd.telr_output import EXPANDED_KEYS, COV_KEYS
    rep.update({k: None for k in EXPANDED_KEYS[-10:]})
    res = dict(annotation=[[name, 50, 150, "jockey", ".", "+"]], liftover=[dict(report=rep, genome1_coord="%s:50-150" % name)],
               af={name: dict({k: 1.0 for k in COV_KEYS}, freq=0.8125)})
    ref_fa = tmp_path / "ref.fa"
    ref_fa.write_text(">%s\n%s\n" % (b["tn"][0], "ACGT" * 15))
    final, _ = locus_pipeline.write_outputs(res, [dict(name=name, contig=contig, reads=list(range(13)), alt=rows[0][7])], str(tmp_path), "s", str(ref_fa),
                                            sv_info=info, today="DATE")
    assert len(final) == 1 and (final[0]["genotype"], final[0]["num_ref_reads"], final[0]["num_sv_reads"]) == ("1/1", "3", "13")
    body = [l for l in (tmp_path / "s.telr.vcf").read_text().splitlines() if not l.startswith("#")]
    assert len(body) == 1 and body[0].endswith("\tGT:DR:DV\t1/1:13:3")
