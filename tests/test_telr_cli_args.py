"""The `telr` command's arguments (telr_amd/telr.py): every default, every refused value, the options that are parsed and have no
effect, the choice of the route by the reads file's extension, and the normal end of a run without calls -- all without an engine:
the loaders and the stages are stubbed."""
import os

import pytest

from telr_amd import telr


@pytest.fixture
def inputs(tmp_path):
    p = {}
    for k, text in (("reads", ">r1\nACGT\n"), ("ref", ">chrA\n" + "ACGT" * 30 + "\n"), ("lib", ">te1\nACGTACGT\n"), ("bam", "")):
        p[k] = str(tmp_path / ("in_%s.%s" % (k, "bam" if k == "bam" else "fasta")))
        with open(p[k], "w") as f:
            f.write(text)
    p["out"] = str(tmp_path / "out")
    return p


def base(inputs, reads="reads"):
    return ["-i", inputs[reads], "-r", inputs["ref"], "-l", inputs["lib"], "-o", inputs["out"]]


def test_every_default(inputs, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = telr.get_args(["-i", inputs["reads"], "-r", inputs["ref"], "-l", inputs["lib"]])
    assert (a.aligner, a.assembler, a.polisher, a.presets) == ("nglmr", "wtdbg2", "wtdbg2", "pacbio")
    assert (a.polish_iterations, a.thread, a.gap, a.overlap, a.flank_len) == (1, 1, 20, 20, 500)
    assert (a.af_flank_interval, a.af_flank_offset, a.af_te_interval, a.af_te_offset) == (100, 200, 50, 50)
    assert (a.different_contig_name, a.minimap2_family, a.keep_files) == (False, False, False)
    assert a.out == os.path.abspath(".")
    assert (a.polish, a.device, a.keep_qual, a.chain_skip, a.seed_rescue, a.mm2_mapq) == ("poa", 0, False, False, False, False)
    assert a.sample == "in_reads" and a.inert_given == []
    assert telr.aligner_preset(a)[0] == "ngmlr-pacbio" and telr.aligner_preset(a)[1] == ("in_reads", "in_reads", "pb")


def test_given_values_and_short_options(inputs):
    a = telr.get_args(base(inputs) + ["--aligner", "minimap2", "-x", "ont", "-p", "3", "-t", "8", "-g", "5", "-v", "7", "--flank_len", "400",
                                      "--af_flank_interval", "10", "--af_flank_offset", "0", "--af_te_interval", "1", "--af_te_offset", "0", "-k",
                                      "--polish", "none", "--device", "2", "--keep_qual", "--chain_skip", "--seed_rescue", "--mm2_mapq", "--sample", "S1"])
    assert (a.aligner, a.presets, a.polish_iterations, a.thread, a.gap, a.overlap, a.flank_len) == ("minimap2", "ont", 3, 8, 5, 7, 400)
    assert (a.af_flank_interval, a.af_flank_offset, a.af_te_interval, a.af_te_offset, a.keep_files) == (10, 0, 1, 0, True)
    assert (a.polish, a.device, a.keep_qual, a.chain_skip, a.seed_rescue, a.mm2_mapq, a.sample) == ("none", 2, True, True, True, True, "S1")
    assert a.out == inputs["out"] and os.path.isdir(a.out)
    name, rg, cmd = telr.aligner_preset(a)
    assert name == "map-ont" and rg is None and "--max-chain-skip 25" in cmd and "-e 500" in cmd


REFUSED = [(["--aligner", "bwa"], "valid alignment method (nglmr/minimap2)"), (["--assembler", "canu"], "valid assembly method (wtdbg2/flye)"),
           (["--polisher", "racon"], "valid polish method (wtdbg2/flye)"), (["-x", "hifi"], "valid preset option (pacbio/ont)"),
           (["-p", "0"], "valid number of iterations"), (["--af_flank_interval", "0"], "flanking sequence interval size"),
           (["--af_flank_interval", "-3"], "flanking sequence interval size"), (["--af_flank_offset", "-1"], "flanking sequence offset size"),
           (["--af_te_interval", "0"], "TE interval size"), (["--af_te_offset", "-1"], "TE offset size"),
           (["--polish", "racon"], "valid polishing step (none/pileup/poa)"), (["--device", "-1"], "valid device"),
           (["--chain_skip"], "options of the minimap2 aligner"), (["--seed_rescue"], "options of the minimap2 aligner"),
           (["--mm2_mapq"], "options of the minimap2 aligner")]


@pytest.mark.parametrize("extra, text", REFUSED, ids=[" ".join(r[0]) for r in REFUSED])
def test_refused_values_exit_with_1(inputs, capsys, extra, text):
    with pytest.raises(SystemExit) as e:
        telr.get_args(base(inputs) + extra)
    assert e.value.code == 1
    assert text in capsys.readouterr().out
    assert telr.main.__module__ == "telr_amd.telr"


@pytest.mark.parametrize("which", ["-i", "-r", "-l"])
def test_an_unreadable_input_exits_with_1(inputs, capsys, which):
    argv = base(inputs)
    argv[argv.index(which) + 1] = inputs["out"] + "/nowhere.fasta"
    with pytest.raises(SystemExit) as e:
        telr.main(argv)
    assert e.value.code == 1
    cap = capsys.readouterr()
    assert "No such file" in cap.out and "Can not open input file: " + inputs["out"] + "/nowhere.fasta" in cap.err


def test_the_four_inert_options_parse(inputs):
    a = telr.get_args(base(inputs) + ["--assembler", "flye", "--polisher", "flye", "--different_contig_name", "--minimap2_family"])
    assert (a.assembler, a.polisher, a.different_contig_name, a.minimap2_family) == ("flye", "flye", True, True)
    assert a.inert_given == ["--assembler", "--polisher", "--different_contig_name", "--minimap2_family"]
    assert telr.get_args(base(inputs) + ["--assembler=wtdbg2"]).inert_given == ["--assembler"]


class Stub:
    """stands where the engine, an index, a set stand: takes any call, frees nothing"""
    def __getattr__(self, name):
        return Stub()

    def __call__(self, *a, **k):
        return Stub()

    def __int__(self):
        return 0


def stub_run(monkeypatch, argv, rows):
    seen = []
    monkeypatch.setattr(telr, "make_engine", lambda device: Stub())
    monkeypatch.setattr(telr, "load_reads", lambda eng, ix, args, tn, bam: (seen.append(("reads", bam)), (["r1"], Stub(), Stub(), lambda: seen.append("released")))[1])
    monkeypatch.setattr(telr, "load_bam", lambda eng, ix, args, tn, tl: (seen.append(("bam", tn, tl)), (["r1"], Stub(), Stub(), lambda: seen.append("released")))[1])
    monkeypatch.setattr(telr, "call_stage", lambda *a: (rows, Stub()))
    monkeypatch.setattr(telr, "draft_stage", lambda *a: pytest.fail("no calls: no drafts"))
    monkeypatch.setattr(telr, "loci_stage", lambda *a: pytest.fail("no calls: no loci"))
    return seen, telr.main(argv)


def test_the_extension_selects_the_route(inputs, monkeypatch):
    assert telr.is_bam("a/b.bam") and not telr.is_bam("a/b.fasta") and not telr.is_bam("a/b.bam.gz") and not telr.is_bam("a/bam")
    seen, code = stub_run(monkeypatch, base(inputs), [])
    assert code == 0 and seen == [("reads", os.path.join(inputs["out"], "intermediate_files", "in_reads_sort.bam")), "released"]
    seen, code = stub_run(monkeypatch, base(inputs, "bam"), [])
    assert code == 0 and seen == [("bam", ["chrA"], [120]), "released"]


@pytest.mark.parametrize("keep", [False, True])
def test_no_calls_is_a_normal_end_with_header_only_files(inputs, monkeypatch, capsys, keep):
    seen, code = stub_run(monkeypatch, base(inputs) + ["--assembler", "flye"] + (["-k"] if keep else []), [])
    assert code == 0
    out = inputs["out"]
    vcf = open(os.path.join(out, "in_reads.telr.vcf")).read().splitlines()
    assert vcf[0] == "##fileformat=VCFv4.1" and "##contig=<ID=chrA,length=120>" in vcf and vcf[-1].startswith("#CHROM")
    assert all(l.startswith("#") for l in vcf)
    assert open(os.path.join(out, "in_reads.telr.bed")).read() == ""
    assert open(os.path.join(out, "in_reads.telr.json")).read().strip() == "[]"
    inter = os.path.join(out, "intermediate_files")
    assert os.path.isdir(inter) == keep
    if keep:
        assert open(os.path.join(inter, "in_reads.vcf_filtered.tsv")).read() == ""
    assert not os.path.exists(inputs["ref"] + ".fai")                  # the index of the reference goes with the intermediate files
    err = capsys.readouterr().err
    assert err.count("have no effect here") == 1 and "TELR found no non-reference TE insertions" in err
    for stage in ("inputs", "index", "reads", "calls", "outputs"):
        assert "[telr] " + stage in err


def test_an_engine_error_is_status_1_and_its_text(inputs, monkeypatch, capsys):
    from telr_amd._lib import TelrError

    def fail(*a):
        raise TelrError("telr_map: out of device memory [somewhere]", -5)
    monkeypatch.setattr(telr, "make_engine", lambda device: Stub())
    monkeypatch.setattr(telr, "load_reads", fail)
    assert telr.main(base(inputs)) == 1
    assert "TelrError: telr_map: out of device memory" in capsys.readouterr().err
    assert not os.path.exists(os.path.join(inputs["out"], "in_reads.telr.vcf"))
