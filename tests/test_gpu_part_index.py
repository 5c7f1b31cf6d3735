"""The multi-part index on the device: telr_merge_parts == its definition in plain Python (tests/part_merge_ref.py) bit
for bit on every case of tests/part_merge_cases.py, from parts with and without a resident CIGAR copy; every host check is refused with
its code and leaves `out` alone; two runs give the same bytes.  Engine end to end: a PartIndex of 1, 2 and 4 parts against the
definition applied to the engine's own per-part results and against the unsplit Index, the merged result's resident CIGAR copy, the
BAM written through it, and the `telr` command with --index_part_bases."""
import ctypes as C
import gzip

import numpy as np
import pytest

import part_merge_cases as pc
import part_merge_ref as ref
from telr_amd import aligner, synth, telr
from telr_amd._abi import ALN_DTYPE, MF_CIGAR, MF_KEEP_CIGARS, MF_PER_TARGET, TELR_E_ARG, TELR_E_RANGE
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu


# ---- telr_merge_parts on hand-built parts -----------------------------------------------------------------------------------------------
def raw_parts(engine, c, resident):
    """one raw result per part of case c: telr_result_from_arrays (no device copy: the merge uploads the words) or, resident, the words
    handed over on the device (the copy a map call with TELR_MF_KEEP_CIGARS leaves)"""
    import torch
    L = engine.L
    raws = []
    for alns, cig in c["parts"]:
        a = np.ascontiguousarray(alns, dtype=ALN_DTYPE); w = np.ascontiguousarray(cig, dtype=np.uint32)
        r = C.c_void_p()
        if resident:
            t = torch.from_numpy(w.view(np.int32).copy()).to("cuda:0")
            torch.cuda.synchronize()
            rc = L.telr_result_from_device_cigars(engine.h, a.ctypes.data, len(a), C.c_void_p(t.data_ptr() if len(w) else 0), len(w), C.byref(r))
        else:
            rc = L.telr_result_from_arrays(engine.h, a.ctypes.data, len(a), w.ctypes.data, len(w), C.byref(r))
        assert rc == 0
        raws.append(r)
    return raws


def merge_call(engine, raws, tid_maps, n_queries, mo):
    """telr_merge_parts through ctypes -> (code, out handle, sentinel kept)"""
    n = len(raws)
    ra = (C.c_void_p * max(1, n))(*[r.value for r in raws])
    maps = [np.ascontiguousarray(m, dtype=np.int32) for m in tid_maps]
    ma = (C.c_void_p * max(1, n))(*[m.ctypes.data for m in maps])
    nt = np.ascontiguousarray([len(m) for m in maps] + [0], dtype=np.int32)
    out = C.c_void_p(0xdead0)
    rc = engine.L.telr_merge_parts(engine.h, n, ra, ma, nt.ctypes.data, n_queries, C.byref(mo), C.byref(out))
    return rc, out


def arrays(engine, r):
    L = engine.L
    return (aligner._np_from(L.telr_result_alns(r), L.telr_result_count(r), ALN_DTYPE),
            aligner._np_from(L.telr_result_cigars(r), L.telr_result_cigar_count(r), np.uint32))


def device_copy(engine, r):
    n = int(engine.L.telr_result_cigar_count(r))
    buf = np.zeros(max(n, 1), np.uint32)
    got = engine.L.telr_debug_result_twin(r, buf.ctypes.data, len(buf))
    return got, buf[:n]


def run_case(engine, c, resident):
    mo = pc.options(**c["opt"])
    raws = raw_parts(engine, c, resident)
    try:
        rc, out = merge_call(engine, raws, c["tid_maps"], c["n_queries"], mo)
        assert rc == 0, engine.L.telr_last_error(engine.h)
        try:
            alns, cig = arrays(engine, out)
            twin_n, twin = device_copy(engine, out)
        finally:
            engine.L.telr_result_free(out)
    finally:
        for r in raws:
            engine.L.telr_result_free(r)
    return alns, cig, twin_n, twin


@pytest.fixture(scope="module")
def expected():
    """the definition on every case, computed once"""
    return {c["name"]: ref.merge(c["parts"], c["tid_maps"], c["n_queries"], pc.options(**c["opt"])) for c in pc.CASES}


@pytest.mark.parametrize("resident", [False, True], ids=["uploaded", "resident"])
@pytest.mark.parametrize("c", pc.CASES, ids=[c["name"] for c in pc.CASES])
def test_merge_equals_the_definition(engine, expected, c, resident):
    want_a, want_c = expected[c["name"]]
    alns, cig, twin_n, twin = run_case(engine, c, resident)
    assert len(alns) == len(want_a)
    for f in ALN_DTYPE.names:
        np.testing.assert_array_equal(alns[f], want_a[f], err_msg=f)
    np.testing.assert_array_equal(cig, want_c)
    assert alns.tobytes() == want_a.tobytes()
    assert twin_n == len(want_c) and np.array_equal(twin, want_c)             # the resident copy is complete
    if c["expect"] is not None:
        assert pc.signature(c, alns) == c["expect"]


def test_two_runs_give_the_same_bytes(engine):
    c = next(x for x in pc.EDGE if x["name"].startswith("pools of 0 1 2 63 64 65 130, three parts"))
    a1, c1, _, t1 = run_case(engine, c, True)
    a2, c2, _, t2 = run_case(engine, c, True)
    assert a1.tobytes() == a2.tobytes() and c1.tobytes() == c2.tobytes() and t1.tobytes() == t2.tobytes() and len(a1) > 130


# (a CIGAR range outside the part's words cannot reach the merge through the C ABI: telr_result_from_arrays and telr_result_from_device_cigars
# refuse such records themselves, as the first assertion shows; the merge's own check of it is pinned on the host, tools/part_plan_check.cpp)
REFUSED = [("qid", 0, 1, "qid"), ("qid", 0, -1, "qid"), ("tid", 0, 2, "tid"), ("tid", 0, -1, "tid"), ("parent", 0, 1, "parent"), ("parent", 0, -1, "parent"),
           ("flags", 0, 3, "class"), ("flags", 0, 8, "class"), ("flags", 0, 7, "class")]


def test_a_cigar_range_outside_the_words_is_refused_before_the_merge(engine):
    a, w = pc.HAND[0]["parts"][0]
    for field, value in (("n_cigar", 99), ("n_cigar", -1), ("cigar_off", -1)):
        b = a.copy(); b[field][0] = value
        r = C.c_void_p(0xdead0)
        assert engine.L.telr_result_from_arrays(engine.h, b.ctypes.data, len(b), w.ctypes.data, len(w), C.byref(r)) == TELR_E_ARG and r.value == 0xdead0


@pytest.mark.parametrize("field,k,value,text", REFUSED, ids=["%s=%d" % (r[0], r[2]) for r in REFUSED])
def test_host_checks_refuse_and_leave_out_alone(engine, field, k, value, text):
    c = pc.HAND[0]
    a, w = c["parts"][0]
    a = a.copy(); a[field][k] = value
    bad = dict(c, parts=[(a, w), c["parts"][1]])
    raws = raw_parts(engine, bad, False)
    try:
        rc, out = merge_call(engine, raws, c["tid_maps"], 1, pc.options())
        assert rc == TELR_E_ARG and out.value == 0xdead0
        assert text in engine.L.telr_last_error(engine.h).decode()
    finally:
        for r in raws:
            engine.L.telr_result_free(r)


def test_other_refusals(engine):
    c = pc.HAND[-1]                                           # five queries, two parts
    raws = raw_parts(engine, c, False)
    try:
        mo = pc.options()
        rc, out = merge_call(engine, raws, c["tid_maps"], 3, mo)                  # qid 3 with three queries
        assert rc == TELR_E_ARG and out.value == 0xdead0
        mo.flags |= MF_PER_TARGET
        rc, out = merge_call(engine, raws, c["tid_maps"], 5, mo)
        assert rc == TELR_E_ARG and out.value == 0xdead0 and "PER_TARGET" in engine.L.telr_last_error(engine.h).decode()
        mo = pc.options()
        rc, out = merge_call(engine, raws, [c["tid_maps"][0], c["tid_maps"][1][:0]], 5, mo)      # part 1 without targets
        assert rc == TELR_E_ARG and out.value == 0xdead0
        assert engine.L.telr_merge_parts(engine.h, 2, None, None, None, 5, C.byref(mo), C.byref(out)) == TELR_E_ARG and out.value == 0xdead0
        assert engine.L.telr_merge_parts(engine.h, -1, None, None, None, 5, C.byref(mo), C.byref(out)) == TELR_E_ARG
        assert engine.L.telr_merge_parts(engine.h, 0, None, None, None, 5, None, C.byref(out)) == TELR_E_ARG
        assert engine.L.telr_merge_parts(engine.h, 0, None, None, None, 5, C.byref(mo), None) == TELR_E_ARG
        # records not ordered by qid
        a, w = c["parts"][0]
        swapped = dict(c, parts=[(a[::-1].copy(), w), c["parts"][1]])
        r2 = raw_parts(engine, swapped, False)
        try:
            rc, out = merge_call(engine, r2, c["tid_maps"], 5, mo)
            assert rc == TELR_E_ARG and out.value == 0xdead0 and "ordered" in engine.L.telr_last_error(engine.h).decode()
        finally:
            for r in r2:
                engine.L.telr_result_free(r)
    finally:
        for r in raws:
            engine.L.telr_result_free(r)
    assert TELR_E_RANGE == -4                                 # (2^31 - 16 pooled records: pinned on the host, tools/part_plan_check.cpp)


# ---- the engine end to end --------------------------------------------------------------------------------------------------------------
PRESETS = ("map-ont", "ngmlr-ont")


@pytest.fixture(scope="module")
def genomes(engine):
    """(repeats) -> targets, reads, the resident read set"""
    out = {}
    for repeats in (False, True):
        targets, reads = pc.genome(repeats)
        out[repeats] = (targets, reads, engine.seqset(reads))
    return out


def map_opt(name):
    io, mo = preset(name)
    mo = mo.copy(); mo.flags |= MF_CIGAR
    return io, mo


@pytest.fixture(scope="module")
def unsplit(engine, genomes):
    out = {}
    for repeats, (targets, reads, qset) in genomes.items():
        for name in PRESETS:
            io, mo = map_opt(name)
            ix = engine.index(targets, io)
            out[(repeats, name)] = ix.map(qset, mo)
            ix.free()
    return out


@pytest.mark.parametrize("name", PRESETS)
@pytest.mark.parametrize("n_parts", [2, 4])
@pytest.mark.parametrize("repeats", [False, True], ids=["unique", "repeats"])
def test_part_index_against_the_definition_and_the_unsplit_index(engine, genomes, unsplit, repeats, n_parts, name):
    targets, reads, qset = genomes[repeats]
    io, mo = map_opt(name)
    pix = engine.index_parts(targets, io, max_part_bases=pc.max_part_bases(pc.CUTS[n_parts]))
    try:
        assert pix.n_parts == n_parts and [int(x) for x in pix.part_of] == pc.CUTS[n_parts] and pix.targets.n == 4
        r = pix.map_raw(qset, mo)
        try:
            alns, cig = arrays(engine, r)
            twin_n, twin = device_copy(engine, r)
        finally:
            pix.free_raw(r)
        # the definition on the engine's own per-part results
        parts = []
        for ix in pix.parts:
            res = ix.map(qset, mo)
            parts.append((res.alns, res.cigars))
        want_a, want_c = ref.merge(parts, pix.tid_maps, len(reads), mo)
        assert alns.tobytes() == want_a.tobytes() and np.array_equal(cig, want_c)
        assert twin_n == len(cig) and np.array_equal(twin, cig)
        whole = unsplit[(repeats, name)]
        print("%s, %d parts, repeats %s: %d records unsplit, %d merged (%d secondary)" % (name, n_parts, repeats, len(whole.alns), len(alns),
                                                                                          int(((alns["flags"] & 2) != 0).sum())))
        if not repeats:
            assert len(alns) >= 80 and ref.records_equal(alns, cig, whole.alns, whole.cigars)
        else:
            a = whole.alns[(whole.alns["flags"] & 1) != 0]; b = alns[(alns["flags"] & 1) != 0]
            assert len(a) == len(b) > 0 and np.array_equal(a["qid"], b["qid"])
            for f in pc.PRIMARY_FIELDS:
                np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    finally:
        pix.free()


@pytest.mark.parametrize("name", PRESETS)
def test_a_one_part_index_equals_the_index(engine, genomes, unsplit, name):
    targets, reads, qset = genomes[False]
    io, mo = map_opt(name)
    pix = engine.index_parts(targets, io)
    try:
        assert pix.n_parts == 1
        res = pix.map(qset, mo)
        whole = unsplit[(False, name)]
        assert ref.records_equal(res.alns, res.cigars, whole.alns, whole.cigars)
        with pytest.raises(TelrError) as e:
            pix.map_raw(qset, mo, qtarget=np.zeros(len(reads), np.int32))
        assert e.value.code == TELR_E_ARG
        mp = mo.copy(); mp.flags |= MF_PER_TARGET
        with pytest.raises(TelrError) as e:
            pix.map_raw(qset, mp)
        assert e.value.code == TELR_E_ARG
        for fn in (pix.write_bam_slice, pix.consensus):
            with pytest.raises(TelrError, match="not for a multi-part index"):
                fn(None, None)
    finally:
        pix.free()


def insertion_genome():
    """two 30-kb targets, and reads of a sample that carries a 600-base insertion in the second: the caller has work, on global target 1"""
    rng = np.random.default_rng(11)
    g = [synth.random_seq(rng, 30000), synth.random_seq(rng, 30000)]
    ins = synth.random_seq(rng, 600)
    sample = [g[0], np.concatenate([g[1][:15000], ins, g[1][15000:]])]
    reads = []
    for k in range(16):
        s = 9000 + 250 * k
        reads.append(synth.mutate(rng, sample[1][s:s + 8000], 0.01, 0.005, 0.005))
    reads += [synth.mutate(rng, g[0][2000 * k:2000 * k + 5000], 0.01, 0.005, 0.005) for k in range(6)]
    return [bytes(t).decode() for t in g], [bytes(r).decode() for r in reads]


def test_calls_on_the_merged_result_and_on_its_records_rebuilt(engine):
    targets, reads = insertion_genome()
    io, mo = map_opt("map-ont")
    qset = engine.seqset(reads)
    pix = engine.index_parts(targets, io, max_part_bases=ref.extent_next(0, 30000) + 1)
    try:
        assert pix.n_parts == 2
        r = pix.map_raw(qset, mo)
        try:
            alns, cig = arrays(engine, r)
            twin_n, twin = device_copy(engine, r)
            assert twin_n == len(cig) > 0 and np.array_equal(twin, cig)
            ic = pix.call_insertions(r)
            rebuilt = pix.result_from_arrays(alns, cig)
            try:
                ic2 = pix.call_insertions(rebuilt)
                gt, gt2 = pix.genotype_insertions(r, ic), pix.genotype_insertions(rebuilt, ic2)
            finally:
                pix.free_raw(rebuilt)
        finally:
            pix.free_raw(r)
        assert len(ic.calls) == 1 and int(ic.calls["tid"][0]) == 1 and abs(int(ic.calls["pos"][0]) - 15000) <= 50
        assert ic.calls.tobytes() == ic2.calls.tobytes() and ic.sigs.tobytes() == ic2.sigs.tobytes() and np.array_equal(ic.reads, ic2.reads)
        assert gt.gt.tobytes() == gt2.gt.tobytes()
    finally:
        pix.free()


# ---- the BAM ----------------------------------------------------------------------------------------------------------------------------
def test_bam_through_a_part_index_equals_the_index_s(engine, genomes, tmp_path):
    targets, reads, qset = genomes[False]
    io, mo = map_opt("map-ont")
    mo.flags |= MF_KEEP_CIGARS
    qn = ["read%d" % i for i in range(len(reads))]; tn = ["chr%d" % i for i in range(len(targets))]
    streams = []
    for k, make in enumerate((lambda: engine.index(targets, io), lambda: engine.index_parts(targets, io, max_part_bases=pc.max_part_bases(pc.CUTS[2])))):
        ix = make()
        try:
            r = ix.map_raw(qset, mo)
            try:
                path = str(tmp_path / ("%d.bam" % k))
                ix.write_bam_device(r, qset, qn, tn, path)
                streams.append(gzip.decompress(open(path, "rb").read()))
            finally:
                ix.free_raw(r)
        finally:
            ix.free()
    assert len(streams[0]) > 100000 and streams[0] == streams[1]


# ---- the command ------------------------------------------------------------------------------------------------------------------------
MM2 = ("--aligner", "minimap2", "-x", "pacbio", "--polish", "poa")


@pytest.fixture(scope="module")
def decoy_reference(data_dir, tmp_path_factory):
    """ref_38kb plus one random 10-kb decoy target, and the --index_part_bases that puts the two into two parts"""
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    decoy = bytes(synth.random_seq(np.random.default_rng(5), 10000)).decode()
    path = tmp_path_factory.mktemp("decoy") / "ref_decoy.fasta"
    path.write_text(">%s\n%s\n>decoy\n%s\n" % (tn[0], ts[0], decoy))
    return str(path), ref.extent_next(0, len(ts[0])) + 1


def count_index_parts(monkeypatch):
    calls = []
    orig = aligner.Engine.index_parts
    monkeypatch.setattr(aligner.Engine, "index_parts", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    return calls


def known_row(out):
    f = out["final"][0]
    body = [l.split("\t") for l in open(out["files"]["vcf"]).read().splitlines() if not l.startswith("#")]
    return (len(out["final"]), f["type"], f["chrom"], f["family"], f["strand"], f["start"], f["end"], body[0][-1].split(":")[0])


def test_command_with_and_without_index_parts(engine, data_dir, decoy_reference, tmp_path, monkeypatch, capsys):
    path, part_bases = decoy_reference
    calls = count_index_parts(monkeypatch)
    argv = ["-i", data_dir + "/reads.fasta", "-r", path, "-l", data_dir + "/library.fasta"]
    one = telr.run(telr.get_args(argv + ["-o", str(tmp_path / "one")] + list(MM2)), engine=engine)
    err_one = capsys.readouterr().err
    assert calls == [] and "stage-1 index (map-pb), 1 part " in err_one
    two = telr.run(telr.get_args(argv + ["-o", str(tmp_path / "two"), "--index_part_bases", str(part_bases)] + list(MM2)), engine=engine)
    err_two = capsys.readouterr().err
    assert len(calls) == 2                                    # the stage-1 index and the asm10 index
    assert "stage-1 index (map-pb), 2 parts" in err_two and "asm10 index of the reference, 2 parts" in err_two
    print(known_row(one), known_row(two))
    assert known_row(one) == (1, "non-reference", "chr2L", "jockey", "-", 33019, 33025, "1/1")
    assert known_row(two) == known_row(one)
    assert one["counts"]["reads"] == two["counts"]["reads"] == 18


def test_command_on_the_plain_reference_never_builds_parts(engine, data_dir, tmp_path, monkeypatch):
    calls = count_index_parts(monkeypatch)
    out = telr.run(telr.get_args(["-i", data_dir + "/reads.fasta", "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(tmp_path)] + list(MM2)),
                   engine=engine)
    assert calls == [] and out["counts"]["loci_written"] == 1
