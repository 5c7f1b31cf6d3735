"""tests/cohort_ref.py, the plain-Python definition of telr_merge_sites, held to the hand-derived answers of tests/cohort_cases.py; what the
generated case has to contain; and the host layers around the merge (telr_sv.read_cohort, the two writers, join_sites_vcfs, the
telr_cohort command line), on small texts written here.  No device: the rows come from the checker's answer through telr_sv.cohort_rows."""
import os

import numpy as np
import pytest

import cohort_cases as cases
import cohort_ref as cref
from telr_amd import _abi, _lib, telr_cohort, telr_sv

HAND = cases.hand_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def generated():
    """the generated case with the checker's answers at min_samples 1 and 2: made once, shared, left unchanged"""
    e = cases.generated()
    return dict(entries=e, one=cref.merge(e), two=cref.merge(e, dict(min_samples=2)))


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_case(case):
    assert case["claim"](case)                                    # the case has the edge it is there for
    got = cref.merge(case["entries"], case["opt"])
    assert got["sites"] == case["sites"] and got["members"] == case["members"] and got["samples"] == case["samples"]
    assert cref.refusal(case["entries"], len(case["entries"]), cases.N_TARGETS, case["opt"]) is None


def test_hand_cases_cover_every_size():
    names = [c["name"] for c in HAND]
    assert all("singletons_%d" % n in names and "one_cluster_%d" % n in names for n in (255, 256, 257, 2047, 2048, 2049))


@pytest.mark.parametrize("case", cases.refusals(), ids=[r[0] for r in cases.refusals()])
def test_refusal_codes(case):
    name, entries, n, n_targets, opt, code = case
    got = cref.refusal(entries, len(entries) if n is None else n, n_targets, opt)
    assert got is not None and got[0] == code
    assert (cref.E_ARG, cref.E_RANGE) == (_abi.TELR_E_ARG, _abi.TELR_E_RANGE)


def test_generated_case_contains_what_it_must(generated):
    cov = cref.coverage(generated["entries"])
    print(cov)
    assert 5000 <= cov["entries"] <= 7000
    for k, least in cases.NEEDS.items():
        assert cov[k] >= least, k
    e = generated["entries"]
    assert len(set(x[0] for x in e)) == 3 and len(set(x[4] for x in e)) == 4 and len(set(x[3] for x in e)) == 40
    assert 0 < len(generated["two"]["sites"]) < len(generated["one"]["sites"])


@pytest.mark.parametrize("which", ("one", "two"))
def test_open_sites_ascend_and_members_partition(generated, which):
    res, e = generated[which], generated["entries"]
    keys = [(t, p) for t, p, _ in cref.site_list(res)]
    assert all(a < b for a, b in zip(keys, keys[1:])) and len(keys) == sum(1 for s in res["sites"] if not s["flags"] & cref.SHADOWED)
    flat = [i for m in res["members"] for i in m]
    assert len(flat) == len(set(flat))                            # no entry in two sites
    if which == "one":
        assert sorted(flat) == list(range(len(e)))                # nothing is dropped at min_samples 1
    for s, m, q in zip(res["sites"], res["members"], res["samples"]):
        assert len(m) == s["n_members"] and q == sorted(set(e[i][3] for i in m)) and len(q) == s["n_samples"]
        assert all((e[i][0], e[i][4]) == (s["tid"], s["group"]) for i in m) and s["rep"] in m
        if s["flags"] & cref.SHADOWED:
            w = res["sites"][s["winner"]]
            assert (w["tid"], w["pos"]) == (s["tid"], s["pos"]) and not w["flags"] & cref.SHADOWED and not s["flags"] & cref.CROWDED
    # every cluster that min_samples = 2 keeps is one that min_samples = 1 has, with the same members
    if which == "two":
        have = {tuple(m) for m in generated["one"]["members"]}
        assert all(tuple(m) in have for m in res["members"])


def test_abi_mirrors_and_exports():
    assert tuple(_abi.COHORT_ENTRY_DTYPE.names) == cref.ENTRY_FIELDS and tuple(_abi.COHORT_SITE_DTYPE.names) == cref.SITE_FIELDS
    assert (_abi.COHORT_SHADOWED, _abi.COHORT_CROWDED) == (cref.SHADOWED, cref.CROWDED)
    o = _abi.CohortOpt.default(min_samples=3)
    assert (o.dist, o.min_samples, o.reserved0, o.reserved1) == (50, 3, 0, 0)
    with pytest.raises(TypeError):
        _abi.CohortOpt.default(nope=1)
    header = open(os.path.join(ROOT, "include", "telr_hip.h")).read()
    for n in ("telr_cohort_opt_default", "telr_merge_sites", "telr_cohort_sites_count", "telr_cohort_sites_sites", "telr_cohort_sites_member_off",
              "telr_cohort_sites_members", "telr_cohort_sites_sample_off", "telr_cohort_sites_samples", "telr_cohort_sites_free"):
        assert n in _lib.EXPORTS and (n + "(") in header
    assert "NOT bcftools merge" in header


# ---- the host layers -------------------------------------------------------------------------------------------------------------
CHROM_IDS, CHROM_LENS = {"chrA": 0, "chrB": 1}, {"chrA": 100000, "chrB": 50000}
VCF_HEAD = ["##fileformat=VCFv4.1", "##source=TELR", '##INFO=<ID=FAMILY,Number=1,Type=String,Description="TE family">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s"]


def vcf_text(sample, calls):
    """calls: (chrom, pos0, alt, family)"""
    lines = [l % sample if "%s" in l else l for l in VCF_HEAD]
    for k, (chrom, pos, alt, fam) in enumerate(calls):
        lines.append("\t".join([chrom, str(pos + 1), "%s.%d" % (sample, k), "N", alt, ".", "PASS", "SVTYPE=INS;END=%d;FAMILY=%s;RE=5" % (pos + 1, fam), "GT:DR:DV", "0/1:5:5"]))
    return "\n".join(lines) + "\n"


def checked_rows(cohort, opt=None):
    """telr_sv's rows from the checker's answer on the cohort's entries"""
    e = [tuple(int(x) for x in r) for r in cohort["entries"].tolist()]
    res = cref.merge(e, opt)
    return telr_sv.cohort_rows(cohort, res["sites"], lambda k: res["members"][k], lambda k: res["samples"][k]), res


@pytest.fixture()
def three_vcfs(tmp_path):
    """s1 and s2 share a roo at chrA:1000 (8 apart); s2 and s3 share a copia at the very position of s3's roo at chrA:5000; s3 alone on chrB"""
    files = {"s1": [("chrA", 1000, "A" * 40, "roo")],
             "s2": [("chrA", 1008, "A" * 50, "roo"), ("chrA", 5000, "C" * 30, "copia")],
             "s3": [("chrA", 5000, "C" * 32, "copia"), ("chrA", 5000, "<INS>", "roo"), ("chrB", 70, "G" * 20, "roo|gypsy")]}
    paths = []
    for s, calls in files.items():
        p = tmp_path / (s + ".telr.vcf")
        p.write_text(vcf_text(s, calls))
        paths.append(str(p))
    return paths


def test_read_cohort_from_vcfs(three_vcfs):
    said = []
    c = telr_sv.read_cohort(three_vcfs, CHROM_IDS, CHROM_LENS, report=said.append)
    assert c["samples"] == ["s1", "s2", "s3"] and c["families"] == ["copia", "roo", "roo|gypsy"] and c["vcf"] and c["chroms"] == ["chrA", "chrB"]
    assert c["entries"].dtype == _abi.COHORT_ENTRY_DTYPE
    # read_sites' rules: one (chrom, pos) per file keeps its first line, so s3's second line at chrA:5000 is dropped, and said so
    assert c["entries"].tolist() == [(0, 1000, 40, 0, 1), (0, 1008, 50, 1, 1), (0, 5000, 30, 1, 0), (0, 5000, 32, 2, 0), (1, 70, 20, 2, 2)]
    assert len(said) == 1 and "s3.telr.vcf" in said[0] and c["inputs"][2]["duplicates"] == 1
    assert c["origin"] == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)] and c["family"] == ["roo", "roo", "copia", "copia", "roo|gypsy"]
    flat = telr_sv.read_cohort(three_vcfs, CHROM_IDS, CHROM_LENS, by_family=False, report=said.append)
    assert flat["families"] == ["*"] and set(flat["entries"]["group"].tolist()) == {0}


def test_read_cohort_from_tsvs_and_refusals(tmp_path, three_vcfs):
    a, b = tmp_path / "a.tsv", tmp_path / "b.sites.tsv"
    a.write_text("# a comment\nchrA\t1000\t40\tx\troo\nchrA\t3000\n")
    b.write_text("chrA\t1004\t0\ty\troo\nchrB\t5\t7\t\t\n")
    c = telr_sv.read_cohort([str(a), str(b)], CHROM_IDS, CHROM_LENS)
    assert c["samples"] == ["a", "b.sites"] and c["families"] == [".", "roo"] and not c["vcf"]
    assert c["entries"].tolist() == [(0, 1000, 40, 0, 1), (0, 3000, 0, 0, 0), (0, 1004, 0, 1, 1), (1, 5, 7, 1, 0)]
    mixed = telr_sv.read_cohort([str(a), three_vcfs[0]], CHROM_IDS, CHROM_LENS)
    assert not mixed["vcf"] and mixed["samples"] == ["a", "s1"]
    rows, _ = checked_rows(mixed)
    with pytest.raises(ValueError, match="every input must be a VCF"):
        telr_sv.write_cohort_vcf(rows, mixed, str(tmp_path / "no.vcf"))
    # two files of one sample name; a chromosome the reference does not have, with the file and the line
    twin = tmp_path / "sub"
    twin.mkdir()
    (twin / "a.tsv").write_text("chrA\t5\n")
    with pytest.raises(ValueError, match="sample 'a'"):
        telr_sv.read_cohort([str(a), str(twin / "a.tsv")], CHROM_IDS, CHROM_LENS)
    bad = tmp_path / "bad.tsv"
    bad.write_text("chrA\t5\nchrX\t5\n")
    with pytest.raises(ValueError, match="bad.tsv line 2"):
        telr_sv.read_cohort([str(a), str(bad)], CHROM_IDS, CHROM_LENS)


def test_read_sites_is_what_it_was(tmp_path):
    """all_lines is the one new argument: without it a TSV still gives no lines"""
    p = tmp_path / "t.tsv"
    p.write_text("chrA\t10\t5\tid\tfam\n")
    assert telr_sv.read_sites(str(p), CHROM_IDS)["lines"] == [] and telr_sv.read_sites(str(p), CHROM_IDS, all_lines=True)["lines"] == [["chrA", "10", "5", "id", "fam"]]


def test_writers_round_trip(three_vcfs, tmp_path):
    c = telr_sv.read_cohort(three_vcfs, CHROM_IDS, CHROM_LENS, report=lambda m: None)
    rows, res = checked_rows(c)
    # roo at 1000 / 1008: one site of two samples at the lower median 1000, length (40, 50) -> 40; copia at 5000: two samples; roo|gypsy alone
    assert [(r["id"], r["n_samples"], r["len"], r["samples"], r["shadowed"], r["crowded"]) for r in rows] == [
        ("chrA:1000:roo", 2, 40, ["s1", "s2"], False, False), ("chrA:5000:copia", 2, 30, ["s2", "s3"], False, False), ("chrB:70:roo|gypsy", 1, 20, ["s3"], False, False)]
    assert [r["members"] for r in rows] == [[0, 1], [2, 3], [4]] and [r["rep"] for r in rows] == [0, 2, 4]
    tsv, vcf = str(tmp_path / "cohort.sites.tsv"), str(tmp_path / "cohort.sites.vcf")
    telr_sv.write_cohort_tsv(rows, tsv)
    telr_sv.write_cohort_vcf(rows, c, vcf)
    want = cref.site_list(res)
    assert telr_sv.read_sites(tsv, CHROM_IDS, CHROM_LENS)["sites"] == want and telr_sv.read_sites(tsv, CHROM_IDS)["ids"] == [r["id"] for r in rows]
    back = telr_sv.read_sites(vcf, CHROM_IDS, CHROM_LENS)
    assert back["vcf"] and back["sites"] == want and back["ids"] == [r["id"] for r in rows]
    lines = [l.split("\t") for l in open(vcf).read().splitlines()]
    head = [l for l in lines if l[0].startswith("#")]
    assert head[-1] == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"] and ["##INFO=<ID=NSAMP" in l[0] for l in head].count(True) == 1
    assert [l[0] for l in head[:3]] == VCF_HEAD[:3]
    data = [l for l in lines if not l[0].startswith("#")]
    assert data[0] == ["chrA", "1001", "chrA:1000:roo", "N", "A" * 40, ".", "PASS", "SVTYPE=INS;END=1001;FAMILY=roo;RE=5;NSAMP=2;SAMPLES=s1,s2"]
    assert data[1][4] == "C" * 30 and data[1][7].endswith(";NSAMP=2;SAMPLES=s2,s3") and all(len(l) == 8 for l in data)
    # the TSV is itself an input of read_cohort: family in the fifth column
    again = telr_sv.read_cohort([tsv], CHROM_IDS, CHROM_LENS)
    assert again["families"] == ["copia", "roo", "roo|gypsy"] and again["entries"]["pos"].tolist() == [1000, 5000, 70]


def test_shadowed_rows_are_comment_lines(tmp_path):
    """two families at one position: the loser is written as a #shadowed line, which read_sites skips, and is left out of the VCF"""
    a, b = tmp_path / "a.telr.vcf", tmp_path / "b.telr.vcf"
    a.write_text(vcf_text("a", [("chrA", 500, "A" * 10, "roo"), ("chrA", 520, "A" * 10, "copia")]))
    b.write_text(vcf_text("b", [("chrA", 500, "A" * 12, "roo"), ("chrB", 9, "T" * 9, "roo")]))
    c = telr_sv.read_cohort([str(a), str(b)], CHROM_IDS, CHROM_LENS)
    c["entries"]["pos"][1] = 500                                  # copia of sample a onto the roo position
    rows, res = checked_rows(c)
    assert [(r["id"], r["shadowed"], r["winner"], r["crowded"]) for r in rows] == [("chrA:500:roo", False, -1, False), ("chrA:500:copia", True, 0, False), ("chrB:9:roo", False, -1, False)]
    tsv, vcf = str(tmp_path / "c.tsv"), str(tmp_path / "c.vcf")
    telr_sv.write_cohort_tsv(rows, tsv)
    telr_sv.write_cohort_vcf(rows, c, vcf)
    text = open(tsv).read().splitlines()
    assert text[0] == "#" + "\t".join(telr_sv.COHORT_FIELDS) and [l.split("\t")[0] for l in text[1:]] == ["chrA", "#shadowed", "chrB"]
    assert text[2].split("\t")[1:5] == ["chrA", "500", "10", "chrA:500:copia"]
    assert telr_sv.read_sites(tsv, CHROM_IDS)["sites"] == cref.site_list(res) == [(0, 500, 10), (1, 9, 9)]
    assert telr_sv.read_sites(vcf, CHROM_IDS)["sites"] == [(0, 500, 10), (1, 9, 9)]


def sites_vcf(sample, fixed, cols):
    head = ["##fileformat=VCFv4.1", "##source=TELR", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    return "\n".join(head + ["\t".join(f + ["GT:DR:DV", c]) for f, c in zip(fixed, cols)]) + "\n"


def test_join_sites_vcfs(tmp_path):
    fixed = [["chrA", "1001", "chrA:1000:roo", "N", "AAAA", ".", "PASS", "NSAMP=2"], ["chrB", "71", "chrB:70:roo", "N", "GG", ".", "PASS", "NSAMP=1"]]
    cols = {"s1": ["0/1:4:5", "./.:0:0"], "s2": ["1/1:0:9", "0/0:7:0"], "s3": ["0/0:6:0", "0/1:3:3"]}
    paths = []
    for s, col in cols.items():
        p = tmp_path / (s + ".telr.sites.vcf")
        p.write_text(sites_vcf(s, fixed, col))
        paths.append(str(p))
    out = str(tmp_path / "joined.vcf")
    assert telr_sv.join_sites_vcfs(paths, out) == 2
    text = open(out).read().splitlines()
    assert text[:2] == ["##fileformat=VCFv4.1", "##source=TELR"] and text[2].split("\t")[8:] == ["FORMAT", "s1", "s2", "s3"]
    assert [l.split("\t") for l in text[3:]] == [fixed[0] + ["GT:DR:DV", "0/1:4:5", "1/1:0:9", "0/0:6:0"], fixed[1] + ["GT:DR:DV", "./.:0:0", "0/0:7:0", "0/1:3:3"]]
    # a file whose fixed columns differ: refused with the file and the line; a file of another length; a line without the FORMAT
    other = [list(fixed[0]), list(fixed[1])]
    other[1][4] = "GT"
    (tmp_path / "x.vcf").write_text(sites_vcf("x", other, cols["s1"]))
    with pytest.raises(ValueError, match=r"x\.vcf line 5"):
        telr_sv.join_sites_vcfs(paths + [str(tmp_path / "x.vcf")], out)
    (tmp_path / "y.vcf").write_text(sites_vcf("y", fixed[:1], cols["s1"][:1]))
    with pytest.raises(ValueError, match=r"y\.vcf: 1 sites"):
        telr_sv.join_sites_vcfs(paths + [str(tmp_path / "y.vcf")], out)
    (tmp_path / "z.vcf").write_text(sites_vcf("z", fixed, cols["s1"]).replace("GT:DR:DV", "GT:DV:DR"))
    with pytest.raises(ValueError, match=r"z\.vcf line 4"):
        telr_sv.join_sites_vcfs([str(tmp_path / "z.vcf")], out)
    with pytest.raises(ValueError):
        telr_sv.join_sites_vcfs([], out)


def test_command_line_and_reference_table(tmp_path, capsys):
    a = telr_cohort.get_args(["merge", "-r", "ref.fa", "-o", "o", "--dist", "7", "--min_samples", "2", "--no_family", "a.vcf", "b.vcf"])
    assert (a.command, a.reference, a.out, a.dist, a.min_samples, a.no_family, a.device, a.inputs) == ("merge", "ref.fa", "o", 7, 2, True, 0, ["a.vcf", "b.vcf"])
    d = telr_cohort.get_args(["merge", "-r", "ref.fa", "x.vcf"])
    assert (d.out, d.dist, d.min_samples, d.no_family) == (".", 50, 1, False)
    j = telr_cohort.get_args(["join", "-o", "out.vcf", "s1.vcf", "s2.vcf"])
    assert (j.command, j.out, j.inputs) == ("join", "out.vcf", ["s1.vcf", "s2.vcf"])
    fa = tmp_path / "r.fasta"
    fa.write_text(">chrA desc\nACGT\nAC\n>chrB\nGG\n")
    assert telr_cohort.reference_table(str(fa)) == (["chrA", "chrB"], [6, 2])
    (tmp_path / "r.fasta.fai").write_text("chrA\t600\t6\t4\t5\nchrB\t20\t20\t2\t3\n")
    assert telr_cohort.reference_table(str(fa)) == (["chrA", "chrB"], [600, 20])          # the .fai is read when it is there
    # join needs no device: through run and through main
    fixed = [["chrA", "11", "i", "N", "A", ".", "PASS", "."]]
    for s in ("p", "q"):
        (tmp_path / (s + ".vcf")).write_text(sites_vcf(s, fixed, ["0/1:1:1"]))
    got = telr_cohort.run(telr_cohort.get_args(["join", "-o", str(tmp_path / "j.vcf"), str(tmp_path / "p.vcf"), str(tmp_path / "q.vcf")]))
    assert got["counts"] == dict(samples=2, sites=1) and open(got["files"]["vcf"]).read().splitlines()[-1].split("\t")[8:] == ["GT:DR:DV", "0/1:1:1", "0/1:1:1"]
    assert "[telr_cohort] join" in capsys.readouterr().err
    assert telr_cohort.main(["join", "-o", str(tmp_path / "k.vcf"), str(tmp_path / "p.vcf"), str(fa)]) == 1
    assert "telr_cohort: ValueError" in capsys.readouterr().err
