"""telr_merge_sites on the device == its definition in plain Python (tests/cohort_ref.py), array for array: the sites in final order, the
two offset arrays, the member and the sample lists, and their dtypes -- on every hand case of tests/cohort_cases.py and on the generated
cohort at min_samples 1 and 2; then the refusals, repeatability, the order of the input, one context's buffers across sizes, the
neighbours on the same context (telr_call_insertions before and after, telr_call_at_sites on the merged list), and the two commands."""
import ctypes as C

import numpy as np
import pytest

import cohort_cases as cases
import cohort_ref as cref
import inscall_cases as icases
from telr_amd import telr_cohort, telr_sv
from telr_amd._abi import CohortOpt, InsOpt, COHORT_ENTRY_DTYPE, COHORT_SITE_DTYPE, TELR_E_ARG, TELR_E_RANGE
from telr_amd._lib import TelrError
from telr_amd.aligner import Engine
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()
REFUSALS = cases.refusals()
TARGETS = ["ACGT" * 64, "TTGCA" * 64, "GGCAT" * 64]          # the site entries only need their number


@pytest.fixture(scope="module")
def generated():
    """the generated cohort with the checker's answers: made once, shared, left unchanged"""
    e = cases.generated()
    return dict(entries=e, one=cref.merge(e), two=cref.merge(e, dict(min_samples=2)))


def assert_equal_to_ref(got, want):
    A = cref.arrays(want)
    assert got.sites.dtype == COHORT_SITE_DTYPE and len(got.sites) == len(want["sites"])
    for f in cref.SITE_FIELDS:
        np.testing.assert_array_equal(got.sites[f], A[f], err_msg="site " + f)
    for name, dt in (("member_off", np.int64), ("members", np.int32), ("sample_off", np.int64), ("samples", np.int32)):
        assert getattr(got, name).dtype == dt, name
        np.testing.assert_array_equal(getattr(got, name), A[name], err_msg=name)
    for k in range(min(len(want["sites"]), 3)):
        assert got.members_of(k).tolist() == want["members"][k] and got.samples_of(k).tolist() == want["samples"][k]
    assert got.site_list().dtype == np.int32 and [tuple(x) for x in got.site_list().tolist()] == cref.site_list(want)


def blob(r):
    return r.sites.tobytes() + r.member_off.tobytes() + r.members.tobytes() + r.sample_off.tobytes() + r.samples.tobytes()


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_case(engine, case):
    want = cref.merge(case["entries"], case["opt"])
    assert want["sites"] == case["sites"] and want["members"] == case["members"] and want["samples"] == case["samples"]      # the checker's answer is the hand-derived one
    assert_equal_to_ref(engine.merge_sites(case["entries"], cases.N_TARGETS, CohortOpt.default(**case["opt"])), want)


@pytest.mark.parametrize("min_samples", (1, 2))
def test_generated_case(engine, generated, min_samples):
    want = generated["one" if min_samples == 1 else "two"]
    assert len(want["sites"]) > 256
    assert_equal_to_ref(engine.merge_sites(generated["entries"], 3, CohortOpt.default(min_samples=min_samples)), want)


def test_nothing_survives_the_filter(engine, generated):
    got = engine.merge_sites(generated["entries"], 3, CohortOpt.default(min_samples=41))          # 40 samples
    assert len(got.sites) == 0 and got.member_off.tolist() == [0] and got.sample_off.tolist() == [0] and len(got.members) == len(got.samples) == 0
    assert cref.merge(generated["entries"], dict(min_samples=41))["sites"] == []


def test_entries_as_a_structured_array_and_other_options(engine, generated):
    e = np.array(generated["entries"], np.int32).view(COHORT_ENTRY_DTYPE).reshape(-1)
    for opt in (dict(dist=0), dict(dist=1000, min_samples=3)):
        assert_equal_to_ref(engine.merge_sites(e, 3, CohortOpt.default(**opt)), cref.merge(generated["entries"], opt))


def test_same_output_on_every_run(engine, generated):
    a, b = engine.merge_sites(generated["entries"], 3), engine.merge_sites(generated["entries"], 3)
    assert blob(a) == blob(b) and len(a.sites) > 256


def test_input_order_does_not_matter(engine, generated):
    """the same entries shuffled: the same sites (rep names the same kind of entry), the same members once mapped back"""
    E = generated["entries"]
    perm = np.random.default_rng(7).permutation(len(E)).tolist()
    a, b = engine.merge_sites(E, 3), engine.merge_sites([E[i] for i in perm], 3)
    for f in cref.SITE_FIELDS:
        if f != "rep":
            np.testing.assert_array_equal(a.sites[f], b.sites[f], err_msg=f)
    assert [E[i] for i in a.sites["rep"].tolist()] == [E[perm[i]] for i in b.sites["rep"].tolist()]
    np.testing.assert_array_equal(a.member_off, b.member_off)
    assert [E[i] for i in a.members.tolist()] == [E[perm[i]] for i in b.members.tolist()]          # entry for entry, in key order
    assert sorted(perm[i] for i in b.members.tolist()) == sorted(a.members.tolist())
    assert a.samples.tobytes() == b.samples.tobytes() and a.sample_off.tobytes() == b.sample_off.tobytes()


def test_growing_and_shrinking_inputs_equal_fresh_engines(engine, generated):
    """small, large, small, nothing kept, one cluster of 2,049, small again through one context's buffers: each equals the call on a fresh engine"""
    by_name = {c["name"]: c for c in HAND}
    small, big1 = by_name["shadowed_between"], by_name["one_cluster_2049"]
    steps = [(small["entries"], {}), (generated["entries"], {}), (small["entries"], {}), (generated["entries"], dict(min_samples=41)), (big1["entries"], {}),
             (small["entries"], {})]
    got = [blob(engine.merge_sites(e, 3, CohortOpt.default(**o))) for e, o in steps]
    assert got[0] == got[2] == got[5]
    for k in (0, 1, 4):
        fresh = Engine(0)
        try:
            assert blob(fresh.merge_sites(steps[k][0], 3, CohortOpt.default(**steps[k][1]))) == got[k], "step %d" % k
        finally:
            fresh.close()


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(engine, case):
    name, entries, n, n_targets, opt, code = case
    assert cref.refusal(entries, len(entries) if n is None else n, n_targets, opt)[0] == code
    e = np.ascontiguousarray(np.array(entries if entries is not None else [(0, 0, 0, 0, 0)], np.int32).reshape(-1, 5))
    h = C.c_void_p(0x5a5a)                                        # not a handle: the entry must leave it as it is
    rc = engine.L.telr_merge_sites(engine.h, e.ctypes.data if entries is not None else None, len(e) if n is None else n, n_targets,
                                   C.byref(CohortOpt.default(**opt)), C.byref(h))
    assert rc == code and h.value == 0x5a5a
    assert b"telr_merge_sites: " in engine.L.telr_last_error(engine.h)
    if n is None:
        with pytest.raises(TelrError) as err:
            engine.merge_sites(entries, n_targets, CohortOpt.default(**opt))
        assert err.value.code == code and "telr_merge_sites" in str(err.value)


def test_null_arguments_and_defaults(engine):
    L = engine.L
    e = np.array([(0, 1000, 60, 0, 0)], np.int32)
    h = C.c_void_p()
    assert L.telr_merge_sites(engine.h, e.ctypes.data, 1, 3, None, None) == TELR_E_ARG
    assert L.telr_merge_sites(None, e.ctypes.data, 1, 3, None, C.byref(h)) == TELR_E_ARG and not h.value
    assert L.telr_merge_sites(engine.h, e.ctypes.data, 1, 3, None, C.byref(h)) == 0          # NULL options = the defaults
    assert L.telr_cohort_sites_count(h) == 1
    L.telr_cohort_sites_free(h)
    assert L.telr_merge_sites(engine.h, None, 0, 0, None, C.byref(h)) == 0                   # no entries: no array and no target needed
    assert L.telr_cohort_sites_count(h) == 0 and L.telr_cohort_sites_count(None) == 0 and not L.telr_cohort_sites_sites(None)
    L.telr_cohort_sites_free(h)
    L.telr_cohort_sites_free(None)
    o = CohortOpt(7, 7, 7, 7)
    L.telr_cohort_opt_default(C.byref(o))
    assert (o.dist, o.min_samples, o.reserved0, o.reserved1) == (50, 1, 0, 0) == tuple(getattr(CohortOpt.default(), k) for k, _ in CohortOpt._fields_)
    assert (TELR_E_ARG, TELR_E_RANGE) == (cref.E_ARG, cref.E_RANGE)


# ---- the neighbours on the same context --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ix(engine):
    io, _ = preset("map-ont")
    return engine.index(TARGETS, io)


def test_discovery_is_untouched_by_a_merge_call(engine, ix, generated):
    recs = [icases.simple(q, 1000 + 3 * q, 60 + q) for q in range(12)] + [icases.simple(20 + q, 5000 + q, 80, tid=1) for q in range(4)]
    r = ix.result_from_arrays(*icases.pack(recs))
    try:
        opt = InsOpt.default(min_support=3)
        before = ix.call_insertions(r, opt)
        merged = engine.merge_sites(generated["entries"], 3)
        after = ix.call_insertions(r, opt)
    finally:
        ix.free_raw(r)
    assert len(before.calls) == 2 and before.calls["support"].tolist() == [12, 4] and len(merged.sites) > 256
    assert before.sigs.tobytes() + before.calls.tobytes() + before.read_off.tobytes() + before.reads.tobytes() == \
        after.sigs.tobytes() + after.calls.tobytes() + after.read_off.tobytes() + after.reads.tobytes()


def test_site_list_is_what_call_at_sites_takes(engine, ix, generated):
    """the merged list of the generated cohort, shadowed sites left out, goes into telr_call_at_sites as it stands: one call per site"""
    merged = engine.merge_sites(generated["entries"], 3)
    sites = merged.site_list()
    assert len(sites) == int(((merged.sites["flags"] & 1) == 0).sum()) > 256 and len(sites) < len(merged.sites)
    k = int(np.flatnonzero(merged.sites["flags"][(merged.sites["flags"] & 1) == 0] == 0)[5])          # a site without a neighbour within reach
    at = tuple(int(x) for x in sites[k])
    recs = [icases.simple(q, at[1] + q, 60, tid=at[0]) for q in range(3)]
    r = ix.result_from_arrays(*icases.pack(recs))
    try:
        ic = ix.call_at_sites(r, sites)
    finally:
        ix.free_raw(r)
    assert len(ic.calls) == len(sites) and ic.calls["pos"].tolist() == sites[:, 1].tolist() and ic.calls["tid"].tolist() == sites[:, 0].tolist()
    assert int(ic.calls["support"][k]) == 3 and int(ic.calls["support"].sum()) == 3


# ---- the commands ----------------------------------------------------------------------------------------------------------------
VCF_HEAD = ["##fileformat=VCFv4.1", "##source=TELR", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s"]
CALLS = {"s1": [("chrA", 1000, "A" * 40, "roo"), ("chrA", 5000, "T" * 25, "roo")],
         "s2": [("chrA", 1008, "A" * 50, "roo"), ("chrA", 5000, "C" * 30, "copia"), ("chrA", 5030, "C" * 30, "gypsy")],
         "s3": [("chrA", 5000, "C" * 32, "copia"), ("chrB", 70, "G" * 20, "roo")]}


def test_merge_and_join_commands(engine, tmp_path, capfd):
    (tmp_path / "ref.fasta").write_text(">chrA\n" + "ACGT" * 2000 + "\n>chrB\n" + "GGCA" * 100 + "\n")
    paths = []
    for s, calls in CALLS.items():
        lines = [VCF_HEAD[0], VCF_HEAD[1], VCF_HEAD[2] % s]
        lines += ["\t".join([c, str(p + 1), "%s.%d" % (s, k), "N", alt, ".", "PASS", "SVTYPE=INS;FAMILY=" + fam, "GT:DR:DV", "0/1:5:5"]) for k, (c, p, alt, fam) in enumerate(calls)]
        (tmp_path / (s + ".telr.vcf")).write_text("\n".join(lines) + "\n")
        paths.append(str(tmp_path / (s + ".telr.vcf")))
    out = tmp_path / "out"
    got = telr_cohort.run(telr_cohort.get_args(["merge", "-r", str(tmp_path / "ref.fasta"), "-o", str(out)] + paths), engine=engine)
    err = capfd.readouterr().err
    assert all("[telr_cohort] " + s in err for s in ("inputs", "merge", "outputs"))
    assert got["counts"] == dict(samples=3, entries=7, families=3, sites=4, shadowed=1, crowded=2) and set(got["seconds"]) == {"inputs", "merge", "outputs"}
    assert sorted(p.name for p in out.iterdir()) == ["cohort.sites.tsv", "cohort.sites.vcf"]
    # copia (two samples) wins chrA:5000 over roo (one); gypsy 30 bases on crowds it
    assert [(r["id"], r["n_samples"], r["shadowed"], r["crowded"], r["samples"]) for r in got["rows"]] == [
        ("chrA:1000:roo", 2, False, False, ["s1", "s2"]), ("chrA:5000:copia", 2, False, True, ["s2", "s3"]), ("chrA:5000:roo", 1, True, False, ["s1"]),
        ("chrA:5030:gypsy", 1, False, True, ["s2"]), ("chrB:70:roo", 1, False, False, ["s3"])]
    chrom_ids = {"chrA": 0, "chrB": 1}
    want = [(0, 1000, 40), (0, 5000, 30), (0, 5030, 30), (1, 70, 20)]
    assert telr_sv.read_sites(got["files"]["sites_tsv"], chrom_ids)["sites"] == want == telr_sv.read_sites(got["files"]["sites_vcf"], chrom_ids)["sites"]
    # the same through the checker
    cohort = telr_sv.read_cohort(paths, chrom_ids)
    assert cref.site_list(cref.merge([tuple(x) for x in cohort["entries"].tolist()])) == want
    # --no_family --min_samples 2: roo and copia at chrA:5000 are one site of three samples
    flat = telr_cohort.run(telr_cohort.get_args(["merge", "-r", str(tmp_path / "ref.fasta"), "-o", str(tmp_path / "flat"), "--no_family", "--min_samples", "2"] + paths),
                           engine=engine)
    assert [(r["id"], r["n_samples"], r["n_members"]) for r in flat["rows"]] == [("chrA:1000:*", 2, 2), ("chrA:5000:*", 3, 4)]
    # join: the merged VCF's lines with a sample column each, as `telr --sites` writes them
    body = [l for l in open(got["files"]["sites_vcf"]).read().splitlines() if not l.startswith("#")]
    sites_files = []
    for k, s in enumerate(CALLS):
        p = tmp_path / (s + ".telr.sites.vcf")
        p.write_text("\n".join(VCF_HEAD[:2] + [VCF_HEAD[2] % s] + [l + "\tGT:DR:DV\t0/1:%d:%d" % (k, j) for j, l in enumerate(body)]) + "\n")
        sites_files.append(str(p))
    joined = telr_cohort.run(telr_cohort.get_args(["join", "-o", str(tmp_path / "cohort.vcf")] + sites_files))
    assert joined["counts"] == dict(samples=3, sites=4)
    text = [l.split("\t") for l in open(joined["files"]["vcf"]).read().splitlines()]
    assert text[2][8:] == ["FORMAT", "s1", "s2", "s3"] and [l[8:] for l in text[3:]] == [["GT:DR:DV"] + ["0/1:%d:%d" % (k, j) for k in range(3)] for j in range(4)]
    assert ["\t".join(l[:8]) for l in text[3:]] == body
