"""telr_call_insertions on the device == its definition in plain Python (tests/inscall_ref.py), array for array: the signatures in
key order, the call fields, the read-id lists.  Records are built by hand and wrapped with result_from_arrays, so every edge is
exact; three tests run the caller behind a real map call (the bundled reads, the stage-1 dataset of test_gpu_stage1_to_loci.py)."""
import ctypes as C

import numpy as np
import pytest

import inscall_cases as cases
import inscall_ref as ref
from telr_amd import synth, telr_assembly, telr_sv
from telr_amd._abi import InsOpt, MF_KEEP_CIGARS, TELR_E_ARG, F_REV, INS_SIG_DTYPE
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()
EDGES = cases.gpu_cases()


@pytest.fixture(scope="module")
def ix(engine):
    """the caller only needs the number of targets: two short ones"""
    io, _ = preset("map-ont")
    return engine.index(["ACGT" * 64, "TTGCA" * 64], io)


def engine_calls(ix, alns, cig, opt):
    r = ix.result_from_arrays(alns, cig)
    try:
        return ix.call_insertions(r, InsOpt.default(**opt))
    finally:
        ix.free_raw(r)


def assert_equal_to_ref(ic, sigs, calls):
    assert len(ic.sigs) == len(sigs)
    for f in ref.SIG_FIELDS:
        np.testing.assert_array_equal(ic.sigs[f], np.array([s[f] for s in sigs], np.int64), err_msg="signature " + f)
    assert len(ic.calls) == len(calls)
    for f in ref.CALL_FIELDS:
        np.testing.assert_array_equal(ic.calls[f], np.array([c[f] for c in calls], np.int64), err_msg="call " + f)
    assert len(ic.read_off) == len(calls) + 1 and ic.read_off[0] == 0
    for k, c in enumerate(calls):
        assert ic.reads_of(k).tolist() == c["reads"]
    assert int(ic.read_off[-1]) == len(ic.reads)


def check(ix, recs, opt):
    alns, cig = cases.pack(recs)
    sigs, calls = ref.call_insertions(alns, cig, opt)
    ic = engine_calls(ix, alns, cig, opt)
    assert_equal_to_ref(ic, sigs, calls)
    return ic, sigs, calls


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(ix, case):
    _, recs, opt, want_sigs, want_calls = case
    ic, sigs, calls = check(ix, recs, opt)
    assert sigs == want_sigs and calls == want_calls          # (and the checker's answer is the hand-derived one)


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_edge_case(ix, case):
    name, recs, opt = case
    ic, sigs, calls = check(ix, recs, opt)
    if name != "reads_interleaved":
        assert len(sigs) > 0
    if name == "ops_100k":
        assert max(len(r["cig"]) for r in recs) > 100000 and len(sigs) > 8000
    if name == "clusters_150":
        assert len(calls) > 64
    if name == "nine_records":
        assert sum(1 for s in sigs if s["kind"] == 1) == 8 + 7      # 72 ordered pairs looked at, those at most two records apart qualify


def test_many_signatures(ix):
    recs, opt = cases.many_signatures()
    ic, sigs, calls = check(ix, recs, opt)
    assert len(sigs) > 65536 and len(calls) > 4096


def test_empty_result_and_no_eligible_record(ix):
    alns, cig = cases.pack([])
    ic = engine_calls(ix, alns, cig, {})
    assert len(ic.calls) == 0 and len(ic.sigs) == 0 and ic.read_off.tolist() == [0]
    alns, cig = cases.pack([cases.simple(0, 100, 60, mapq=3), cases.simple(1, 100, 60, flags=2)])
    ic = engine_calls(ix, alns, cig, dict(min_support=1))
    assert len(ic.calls) == 0 and len(ic.sigs) == 0
    # eligible records without any signature
    alns, cig = cases.pack([cases.simple(0, 100, 20)])
    ic = engine_calls(ix, alns, cig, dict(min_support=1))
    assert len(ic.calls) == 0 and len(ic.sigs) == 0


def test_same_output_on_every_run(ix):
    recs, opt = cases.many_signatures()
    alns, cig = cases.pack(recs[:3000])
    a = engine_calls(ix, alns, cig, opt)
    b = engine_calls(ix, alns, cig, opt)
    assert a.sigs.tobytes() == b.sigs.tobytes() and a.calls.tobytes() == b.calls.tobytes() and a.reads.tobytes() == b.reads.tobytes()


def test_argument_errors(ix, engine):
    alns, cig = cases.pack([cases.simple(0, 100, 60)])
    for bad in (dict(min_len=-1), dict(min_mapq=-1), dict(min_clip=-1), dict(max_ref_gap=-1), dict(cluster_dist=-1), dict(min_support=-1),
                dict(min_sized=-1), dict(min_support=2, min_sized=3)):
        with pytest.raises(TelrError) as e:
            engine_calls(ix, alns, cig, bad)
        assert e.value.code == TELR_E_ARG
        assert b"telr_call_insertions" in engine.L.telr_last_error(engine.h)
    for tid in (2, -1):                                  # the index has two targets
        alns, cig = cases.pack([cases.simple(0, 100, 60, tid=tid)])
        with pytest.raises(TelrError) as e:
            engine_calls(ix, alns, cig, {})
        assert e.value.code == TELR_E_ARG and b"tid" in engine.L.telr_last_error(engine.h)
    r = ix.result_from_arrays(*cases.pack([cases.simple(0, 100, 60)]))
    try:
        h = C.c_void_p()
        assert engine.L.telr_call_insertions(engine.h, r, 0, None, C.byref(h)) == TELR_E_ARG
        assert engine.L.telr_call_insertions(engine.h, None, 1, None, C.byref(h)) == TELR_E_ARG
        assert engine.L.telr_call_insertions(engine.h, r, 1, None, C.byref(h)) == 0          # NULL options = the defaults
        assert engine.L.telr_ins_calls_sig_count(h) == 1 and engine.L.telr_ins_calls_count(h) == 0
        engine.L.telr_ins_calls_free(h)
    finally:
        ix.free_raw(r)
    o = InsOpt()
    engine.L.telr_ins_opt_default(C.byref(o))
    assert {k: getattr(o, k) for k in ref.DEFAULTS} == ref.DEFAULTS


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
    a = b["ix"].call_insertions(b["r"])
    r2 = b["ix"].result_from_arrays(res.alns, res.cigars)
    try:
        c = b["ix"].call_insertions(r2)
    finally:
        b["ix"].free_raw(r2)
    assert len(a.calls) == 1
    assert a.sigs.tobytes() == c.sigs.tobytes() and a.calls.tobytes() == c.calls.tobytes()
    assert a.reads.tobytes() == c.reads.tobytes() and a.read_off.tolist() == c.read_off.tolist()


def test_bundled_reads_end_to_end(engine, bundled, data_dir):
    from oracle import binding as ob
    b = bundled
    _, mo = preset("map-pb")
    want = ob.OracleIndex(b["ts"], b["io"]).map(b["qs"], mo)
    sigs, calls = ref.call_insertions(want["alns"], want["cigars"])
    ic = b["ix"].call_insertions(b["r"])
    assert_equal_to_ref(ic, sigs, calls)
    assert len(calls) == 1 and 33006 <= calls[0]["pos"] <= 33029
    rows = telr_sv.call_insertions(b["ix"], b["r"], b["tn"], b["qn"], b["qs"], sample="s")
    assert len(rows) == 1 and len(rows[0]) == len(telr_sv.COLUMNS)
    row = rows[0]
    c = calls[0]
    assert row[:5] == [b["tn"][0], str(c["pos"]), str(c["pos"] + 1), str(c["len"]), str(c["support"])]
    assert row[6] == "s.INS.0" and row[9] == "PASS" and row[12] == str(c["support"])
    assert row[8].split(",") == [b["qn"][q] for q in c["reads"]]
    s = sigs[c["rep"]]
    assert len(row[7]) == s["seg_len"] >= c["len"] - 200
    # the rows go on unchanged: the merge of nearby calls, and the window reads of the locus hold the call's reads
    assert telr_sv.merge_rows(rows) == rows
    assert telr_sv.merge_rows(rows + [list(rows[0])])[0][12] == str(c["support"])
    wr = telr_assembly.window_reads(b["ix"].result_arrays(b["r"]).alns, {b["tn"][0]: 0}, rows)
    assert set(c["reads"]) <= set(wr[0].tolist())
    # the ALT sequence is the element: mapped against the TE library it hits `jockey`, on the minus strand
    ln, lib = read_fasta(data_dir + "/library.fasta")
    io, mo = preset("map-pb")
    hits = engine.index(lib, io).map([row[7]], mo).alns
    hits = hits[(hits["flags"] & 2) == 0]
    print("library hits of the ALT sequence:", [(ln[h["tid"]], int(h["qs"]), int(h["qe"]), bool(h["flags"] & F_REV)) for h in hits])
    assert len(hits) == 1 and "jockey" in ln[hits[0]["tid"]].lower() and hits[0]["flags"] & F_REV


def test_stage1_dataset_equals_the_checker(engine):
    """the 200 spiked sites of test_gpu_stage1_to_loci.py at min_support 3 (recall and false calls are printed: DESIGN.md 5.10 quotes them)"""
    d = synth.make_stage1_dataset(seed=20261002, read_seed=20261002 + 1000)
    io, mo = preset("map-ont")
    six = engine.index([bytes(d["ref"]).decode()], io)
    r = six.map_raw(engine.seqset(d["reads"]), mo)
    try:
        res = six.result_arrays(r)
        opt = dict(min_support=3)
        ic = six.call_insertions(r, InsOpt.default(**opt))
    finally:
        six.free_raw(r)
    # the checker walks every op of every record it is given; a record without an I of min_len gives no intra signature whatever
    # else its CIGAR holds, so those records (found with one vectorised pass) are handed over without ops -- tens of millions fewer
    alns, cig = res.alns.copy(), res.cigars
    long_i = np.flatnonzero(((cig & 15) == 1) & ((cig >> 4) >= ref.DEFAULTS["min_len"]))
    nc = alns["n_cigar"].astype(np.int64)
    op_rec = np.full(len(cig), -1, np.int64)              # the record that owns an op (ops of dropped chains: none)
    op_rec[np.repeat(alns["cigar_off"] - (np.cumsum(nc) - nc), nc) + np.arange(int(nc.sum()))] = np.repeat(np.arange(len(alns)), nc)
    has = np.zeros(len(alns), bool)
    has[op_rec[long_i][op_rec[long_i] >= 0]] = True
    alns["n_cigar"][~has] = 0
    sigs, calls = ref.call_insertions(alns, cig, opt)
    assert_equal_to_ref(ic, sigs, calls)
    sites = np.array(sorted(p for p, *_ in d["insertions"]))
    cp = np.array([c["pos"] for c in calls])
    near = np.abs(cp[:, None] - sites[None, :]).min(axis=1) if len(cp) else np.zeros(0)
    found = sum(1 for s in sites if len(cp) and np.abs(cp - s).min() <= 60)
    print("stage-1 dataset: %d signatures, %d calls; %d of %d spiked sites have a call within 60 bases; %d calls lie farther than 60 bases from every site"
          % (len(sigs), len(calls), found, len(sites), int((near > 60).sum())))
    assert len(calls) > 0
