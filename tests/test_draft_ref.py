"""The draft step's definition (tests/draft_ref.py, the checker of telr_draft_contigs) against hand-derived answers, one case per rule
(tests/draft_cases.py works them out in its comments), against the bundled reads, and through the per-locus bundle on the CPU oracle."""
import pytest

import draft_cases as cases
import draft_ref as dref
import inscall_ref as iref
from inscall_cases import pack
from telr_amd.fasta import read_fasta, revcomp
from telr_amd.presets import preset

HAND = cases.hand_cases()


def trimmed(got):
    return [{k: d[k] for k in dref.DRAFT_FIELDS} for d in got]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(case):
    _, recs, calls, sigs, opt, want = case
    alns, cig = pack(recs)
    got, _ = dref.drafts(alns, cig, calls, sigs if sigs is not None else cases.sigs_of(alns, cig), None, opt)
    assert trimmed(got) == want


def test_hand_cases_cover_the_rules():
    names = [c[0] for c in HAND]
    assert len(set(names)) == len(names) >= 25
    assert any(d["rc"] for c in HAND for d in c[5]) and any(d["sig"] < 0 for c in HAND for d in c[5])
    assert dref.DEFAULTS == dict(flank=2000, min_flank=500, reach=50, max_len=100000)


def test_lo_hi_by_hand():
    # 10M 3I 10M 2D 5M from (100, 7): states (100,7) .. (110,17) -> I -> (110,20) .. (120,30) -> D (121,30) (122,30) .. (127,35)
    alns, cig = pack([cases.rec(0, 50, 7, 35, 100, 127, [(10, "M"), (3, "I"), (10, "M"), (2, "D"), (5, "M")])])
    a = alns[0]
    assert dref.lo_hi(a, cig, 100) == (7, 7) and dref.lo_hi(a, cig, 110) == (17, 20) and dref.lo_hi(a, cig, 115) == (25, 25)
    assert dref.lo_hi(a, cig, 120) == (30, 30) and dref.lo_hi(a, cig, 121) == (30, 30) and dref.lo_hi(a, cig, 127) == (35, 35)
    assert dref.lo_hi(a, cig, 99) is None and dref.lo_hi(a, cig, 128) is None
    # the same record on the reverse strand: qs' = 50 - 35 = 15
    alns, cig = pack([cases.rec(0, 50, 7, 35, 100, 127, [(10, "M"), (3, "I"), (10, "M"), (2, "D"), (5, "M")], flags=8)])
    assert dref.lo_hi(alns[0], cig, 110) == (25, 28)


def test_sequences_are_on_the_reference_strand():
    reads = ["ACGTNACGTTGCAAGGCTTA" * 5]            # 100 bases
    recs = [cases.rec(0, 100, 10, 90, 1000, 1020, [(10, "M"), (60, "I"), (10, "M")], flags=8)]
    alns, cig = pack(recs)
    got, seqs = dref.drafts(alns, cig, [cases.call(0, 1010, 60, [0])], cases.sigs_of(alns, cig), reads, cases.SMALL)
    assert trimmed(got) == [cases.D(0, 0, 10, 80, 1, 10, 60, 0)]
    assert seqs == [revcomp(reads[0][10:90])] and seqs[0].count("N") == 4


# ---- the bundled reads through the oracle ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(data_dir):
    from oracle import binding as ob
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    out = dict(tn=tn, ts=ts, qn=qn, qs=qs)
    for name in ("map-pb", "map-ont", "ngmlr-pacbio"):
        io, mo = preset(name)
        out[name] = ob.OracleIndex(ts, io).map(qs, mo)
    return out


# measured on the CPU (oracle records, inscall_ref calls): the backbone read, its piece on the forward read, where the insertion lies
BUNDLED = {"map-pb": dict(sig=6, qid=4, start=1, len=7750, rc=1, ins_off=2035, ins_len=4562, n_candidates=6),
           "map-ont": dict(sig=9, qid=17, start=300, len=8416, rc=0, ins_off=1819, ins_len=4586, n_candidates=5),
           "ngmlr-pacbio": dict(sig=18, qid=4, start=1, len=7739, rc=1, ins_off=2034, ins_len=4554, n_candidates=6)}


@pytest.mark.parametrize("name", sorted(BUNDLED))
def test_bundled_reads(bundled, name):
    r = bundled[name]
    sigs, calls = iref.call_insertions(r["alns"], r["cigars"])
    got, seqs = dref.drafts(r["alns"], r["cigars"], calls, sigs, bundled["qs"])
    print(name, got)
    assert len(got) == len(seqs) == 1
    d = got[0]
    assert d["sig"] >= 0 and d["set_index"] == 0 and len(seqs[0]) == d["len"]
    assert d["ins_off"] >= dref.DEFAULTS["min_flank"] and d["ins_off"] + d["ins_len"] <= d["len"] - dref.DEFAULTS["min_flank"]      # the insertion inside it
    assert d["qid"] in calls[0]["reads"] and d["n_valid"] == d["n_candidates"]
    assert {k: d[k] for k in BUNDLED[name]} == BUNDLED[name]


def bundled_locus(bundled, name="map-pb"):
    """the one locus of the bundled reads as run_loci takes it (window reads as sequences): name, draft, ALT, the reads"""
    from telr_amd import telr_assembly
    r = bundled[name]
    sigs, calls = iref.call_insertions(r["alns"], r["cigars"])
    got, seqs = dref.drafts(r["alns"], r["cigars"], calls, sigs, bundled["qs"])
    c = calls[0]
    row = [bundled["tn"][0], str(c["pos"]), str(c["pos"] + 1)]
    s = sigs[c["rep"]]
    alt = bundled["qs"][s["qid"]][s["seg_start"]:s["seg_start"] + s["seg_len"]]
    if int(r["alns"][s["rec"]]["flags"]) & 8:
        alt = revcomp(alt)
    wr = telr_assembly.window_reads(r["alns"], {bundled["tn"][0]: 0}, [row])[0]
    return dict(name="_".join(row), contig=seqs[0], alt=alt, read_idx=wr), got[0]


def oracle_bundle(bundled, data_dir):
    from oracle_backend import OracleBackend
    from telr_amd import locus_pipeline
    ln, lib = read_fasta(data_dir + "/library.fasta")
    locus, _ = bundled_locus(bundled)
    locus = dict(locus, reads=[bundled["qs"][i] for i in locus.pop("read_idx")])
    be = OracleBackend()
    io10, _ = preset("asm10")
    res = locus_pipeline.run_loci(be, be.index(bundled["ts"], io10), bundled["tn"], lambda ch: bundled["ts"][0], [locus], ln, lib, presets="pacbio")
    return locus, res


def test_bundled_locus_on_the_oracle(bundled, data_dir, tmp_path):
    """The draft of the bundled reads through run_loci to write_outputs on the CPU oracle, WITHOUT polishing (the consensus kernels have no
    CPU counterpart).  Measured: the element is found in the draft -- one `jockey`, minus strand, contig bases 2,045-6,600 -- and the allele
    frequency is 0.682; the flanks of the unpolished read piece (a raw PacBio read) do not map with asm10, so the liftover reports
    `unlifted` and the VCF and BED hold no row.  SURVEY 4's coordinate (33,006-33,029) is therefore NOT confirmed by the CPU run."""
    from telr_amd import locus_pipeline
    locus, res = oracle_bundle(bundled, data_dir)
    assert locus["name"] == "chr2L_33024_33025" and len(locus["reads"]) == 18
    assert res["annotation"] == [["chr2L_33024_33025", "2045", "6600", "jockey", ".", "-"]]
    assert len(res["liftover"]) == 1
    rep = res["liftover"][0]["report"]
    print(rep, res["af"])
    assert (rep["type"], rep["family"], rep["chrom"], rep["start"]) == ("unlifted", "jockey", None, None)
    assert res["af"]["chr2L_33024_33025"]["freq"] == 0.682
    ref_fa = tmp_path / "ref.fa"                      # (write_outputs leaves a .fai next to the reference)
    ref_fa.write_text(">%s\n%s\n" % (bundled["tn"][0], bundled["ts"][0]))
    final, _ = locus_pipeline.write_outputs(res, [locus], str(tmp_path), "s", str(ref_fa), today="DATE")
    assert final == []
    vcf = (tmp_path / "s.telr.vcf").read_text().splitlines()
    assert vcf[0].startswith("##fileformat=VCF") and [l for l in vcf if not l.startswith("#")] == []
    assert (tmp_path / "s.telr.bed").read_text() == ""
