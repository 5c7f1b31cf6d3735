"""The `telr` command end to end on the bundled reads (telr_amd/telr.py): both routes meet the known answer of SURVEY 4
(one non-reference `jockey` on chr2L, minus strand, inside 33,006-33,029; the bounds are those of tests/test_gpu_draft.py's end-to-end
test, derived from the signatures), neither decodes the read set to host text, and telr_sv.call_insertions / telr_assembly.draft_loci
give the same rows and loci from the resident set as from host strings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from telr_amd import aligner, telr, telr_assembly, telr_sv
from telr_amd._abi import MF_KEEP_CIGARS
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def argv_for(data_dir, reads, out, *extra):
    return ["-i", reads, "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out)] + list(extra)


MM2 = ("--aligner", "minimap2", "-x", "pacbio", "--polish", "poa")


class Watch:
    """counts what would be a decode of the whole set, and the bytes SeqSet.extract returns against the pieces the run needs"""
    def __init__(self, engine):
        self.mp = pytest.MonkeyPatch()
        self.decodes, self.extract_bytes, self.extract_calls, self.needed = [], 0, 0, 0
        w = self
        ascii_fn, extract, drafts, calls = engine.L.telr_bam_in_ascii, aligner.SeqSet.extract, telr.draft_stage, telr.call_stage

        def counted_ascii(*a):
            w.decodes.append("telr_bam_in_ascii")
            return ascii_fn(*a)

        def counted_extract(self_, *a, **k):
            got = extract(self_, *a, **k)
            w.extract_calls += 1
            w.extract_bytes += sum(len(g) for g in got)
            return got

        def watched_calls(*a):
            rows, ic = calls(*a)
            w.needed += sum(len(r[7]) for r in rows)
            return rows, ic

        def watched_drafts(*a):
            loci, cset, skipped = drafts(*a)
            w.needed += sum(len(l["contig"]) for l in loci)
            return loci, cset, skipped
        self.mp.setattr(engine.L, "telr_bam_in_ascii", counted_ascii)
        self.mp.setattr(aligner.BamInput, "reads", lambda self_: w.decodes.append("BamInput.reads") or pytest.fail("BamInput.reads() called"))
        self.mp.setattr(aligner.BamInput, "write_fasta", lambda self_, p: w.decodes.append("BamInput.write_fasta") or pytest.fail("write_fasta called"))
        self.mp.setattr(aligner.SeqSet, "extract", counted_extract)
        self.mp.setattr(telr, "call_stage", watched_calls)
        self.mp.setattr(telr, "draft_stage", watched_drafts)

    def undo(self):
        self.mp.undo()


def watched_run(engine, argv):
    w = Watch(engine)
    try:
        out = telr.run(telr.get_args(argv), engine=engine)
    finally:
        w.undo()
    return out, w


def brief(res):
    """the final rows without their sequences, for the log"""
    return [{k: v for k, v in f.items() if k != "te_sequence"} for f in res["final"]], res["counts"]


def vcf_body(path):
    return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("#")]


def assert_known_answer(out):
    """SURVEY 4's insertion, with the bounds of tests/test_gpu_draft.py::test_bundled_reads_end_to_end"""
    final, files, counts = out["final"], out["files"], out["counts"]
    assert len(final) == 1
    f = final[0]
    assert (f["type"], f["chrom"], f["family"], f["strand"]) == ("non-reference", "chr2L", "jockey", "-")
    assert 33006 <= f["start"] <= f["end"] <= 33029
    assert 13 / 18 - 0.1 <= f["allele_frequency"] <= 13 / 16 + 0.1
    body = vcf_body(files["vcf"])
    assert len(body) == 1 and body[0][0] == "chr2L" and int(body[0][1]) == f["start"] + 1 and body[0][-2] == "GT:DR:DV"
    assert "FAMILY=jockey" in body[0][7] and "STRANDS=-" in body[0][7] and len(body[0][-1].split(":")) == 3
    bed = [l.split("\t") for l in open(files["bed"]).read().splitlines()]
    assert len(bed) == 1 and (bed[0][0], int(bed[0][1]), int(bed[0][2]), bed[0][3], bed[0][5]) == ("chr2L", f["start"], f["end"], "jockey", "-")
    assert counts["reads"] == 18 and counts["records"] >= 18 and counts["calls"] == 1 and counts["calls_without_draft"] == 0
    assert (counts["loci_annotated"], counts["loci_lifted"], counts["loci_written"]) == (1, 1, 1)
    assert set(out["seconds"]) == {"inputs", "index", "reads", "calls", "drafts", "index10", "loci", "outputs"}


def assert_no_whole_set_decode(w):
    assert w.decodes == []
    assert w.extract_calls == 2                     # one for the ALT pieces, one for the contigs
    assert 0 < w.extract_bytes <= w.needed


@pytest.fixture(scope="module")
def reads_run(engine, data_dir, tmp_path_factory):
    out = tmp_path_factory.mktemp("telr_reads")
    res, w = watched_run(engine, argv_for(data_dir, data_dir + "/reads.fasta", out, *MM2, "-k"))
    return res, w, out


def test_reads_route_known_answer(reads_run):
    res, w, out = reads_run
    print(brief(res), res["seconds"])
    assert_known_answer(res)
    inter = out / "intermediate_files"
    assert res["files"]["bam"] == str(inter / "reads_sort.bam")
    assert (inter / "reads_sort.bam").stat().st_size > 1000 and (inter / "reads_sort.bam.bai").stat().st_size > 0
    table = telr_sv.read_locus_table(res["files"]["locus_table"])
    assert len(table) == 1 and len(table[0]) == 14 and table[0][0] == "chr2L" and table[0][10] in telr_sv.GENOTYPES
    assert_no_whole_set_decode(w)


def test_reads_route_removes_the_intermediate_files(engine, data_dir, tmp_path, reads_run):
    res = telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", tmp_path, *MM2)), engine=engine)
    assert not (tmp_path / "intermediate_files").exists()
    assert vcf_body(res["files"]["vcf"]) == vcf_body(reads_run[0]["files"]["vcf"])
    assert not os.path.exists(data_dir + "/ref_38kb.fasta.fai")


def test_bam_route(engine, data_dir, tmp_path, reads_run):
    res, w = watched_run(engine, argv_for(data_dir, reads_run[0]["files"]["bam"], tmp_path, *MM2, "-k"))
    print(brief(res))
    assert "bam" not in res["files"] and not (tmp_path / "reads_sort.telr.fasta").exists()
    assert_known_answer(res)
    assert_no_whole_set_decode(w)
    same = vcf_body(res["files"]["vcf"]) == vcf_body(reads_run[0]["files"]["vcf"])
    print("BAM route VCF body equals the reads route's:", same)          # recorded in DESIGN.md 5.14; not asserted (the read numbering differs)


def test_a_bam_of_another_reference_is_refused(engine, data_dir, tmp_path, reads_run, capsys):
    other = tmp_path / "other.fasta"
    other.write_text(">chrX\n" + "ACGTTGCA" * 200 + "\n")
    argv = argv_for(data_dir, reads_run[0]["files"]["bam"], tmp_path / "o", *MM2)
    argv[argv.index("-r") + 1] = str(other)
    with pytest.raises(ValueError, match="references are not"):
        telr.run(telr.get_args(argv), engine=engine)


def test_default_aligner_runs(engine, data_dir, tmp_path):
    """the ngmlr-pacbio preset: asserted only that it ran and that its files parse; what it finds is printed and recorded in DESIGN.md 5.14"""
    res = telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", tmp_path)), engine=engine)
    print(brief(res))
    body = vcf_body(res["files"]["vcf"])
    assert len(body) == res["counts"]["loci_written"] == len(open(res["files"]["bed"]).read().splitlines())
    for row in body:
        assert len(row) == 10 and int(row[1]) > 0
    head = [l for l in open(res["files"]["vcf"]).read().splitlines() if l.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.1" and head[-1].startswith("#CHROM")


def test_subprocess_run(data_dir, tmp_path, reads_run):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "telr_amd.telr"] + argv_for(data_dir, data_dir + "/reads.fasta", tmp_path, *MM2, "-k"),
                       cwd=str(tmp_path), env=env, timeout=240, capture_output=True, text=True)
    print(p.stderr[-3000:])
    assert p.returncode == 0
    assert vcf_body(str(tmp_path / "reads.telr.vcf")) == vcf_body(reads_run[0]["files"]["vcf"])
    assert "[telr] finished" in p.stderr and "1 insertions" in p.stderr


# ---- the two functions that take the resident set as `reads` ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(engine, data_dir):
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-pb")
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    ix = engine.index(ts, io)
    qset = engine.seqset(qs)
    r = ix.map_raw(qset, mo)
    yield dict(ix=ix, r=r, tn=tn, qn=qn, qs=qs, qset=qset)
    ix.free_raw(r)


def test_rows_and_loci_from_the_set_equal_those_from_strings(bundled):
    b = bundled
    assert all(set(s) <= set("ACGTN") for s in b["qs"])
    for gt in (None, True):
        rows = telr_sv.call_insertions(b["ix"], b["r"], b["tn"], b["qn"], b["qs"], sample="s", genotype=gt)
        assert rows == telr_sv.call_insertions(b["ix"], b["r"], b["tn"], b["qn"], b["qset"], sample="s", genotype=gt)
    assert len(rows) == 1 and len(rows[0][7]) > 4000
    ic = b["ix"].call_insertions(b["r"])
    chrom_ids = {b["tn"][0]: 0}
    l1, c1, s1 = telr_assembly.draft_loci(b["ix"], b["r"], ic, rows, b["qset"], b["qs"], chrom_ids)
    l2, c2, s2 = telr_assembly.draft_loci(b["ix"], b["r"], ic, rows, b["qset"], b["qset"], chrom_ids)
    assert s1 == s2 == [] and len(l1) == len(l2) == 1
    for x, y in zip(l1, l2):
        assert x["name"] == y["name"] and x["contig"] == y["contig"] and x["alt"] == y["alt"]
        np.testing.assert_array_equal(x["read_idx"], y["read_idx"])
    c1.free(); c2.free()
