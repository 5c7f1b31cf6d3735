"""gzip and BGZF reads files through the product: `telr` writes the same VCF, BED and JSON bodies from reads.fasta as
gzip and as BGZF as from the plain file, without calling the Python reader for the reads; alignment(keep_qual=True) writes the same BAM
stream from a .gz FASTQ as from the plain one; a .gz that the device parser refuses still runs, through the reader, to the same outputs."""
import json
import os
import random

import pytest

import bam_in_ref as B
import reads_in_ref as R
from telr_amd import fasta, telr, telr_alignment
from telr_amd.telr_alignment import alignment, wait_release

pytestmark = pytest.mark.gpu

MM2 = ("--aligner", "minimap2", "-x", "pacbio", "--polish", "poa")


def argv_for(data_dir, reads, out, *extra):
    return ["-i", str(reads), "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out), "--sample", "s"] + list(extra)


def bodies(res):
    f = res["files"]
    vcf = [l for l in open(f["vcf"]).read().splitlines() if not l.startswith("#")]
    return vcf, open(f["bed"]).read(), json.load(open(f["json"]))


class CountedReader:
    """fasta.read_fasta, with the paths it is called for"""
    def __init__(self):
        self.mp, self.paths, inner = pytest.MonkeyPatch(), [], fasta.read_fasta

        def counted(path, *a, **k):
            self.paths.append(str(path))
            return inner(path, *a, **k)
        self.mp.setattr(fasta, "read_fasta", counted)
        self.mp.setattr(telr_alignment, "read_fasta", counted)


@pytest.fixture(scope="module")
def plain_run(engine, data_dir, tmp_path_factory):
    out = tmp_path_factory.mktemp("plain")
    return bodies(telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", out, *MM2)), engine=engine))


@pytest.mark.parametrize("kind", ["gz6", "bgzf"])
def test_telr_on_compressed_reads(engine, data_dir, tmp_path, plain_run, kind):
    text = open(data_dir + "/reads.fasta", "rb").read()
    reads = tmp_path / "reads.fasta.gz"
    reads.write_bytes(R.container(kind, text, list(range(40000, len(text), 40000))))
    w = CountedReader()
    try:
        res = telr.run(telr.get_args(argv_for(data_dir, reads, tmp_path / "out", *MM2, "--reads_chunk_mb", "1")), engine=engine)
    finally:
        w.mp.undo()
    assert str(reads) not in w.paths and len(w.paths) == 2          # the reference and the library, not the reads
    assert bodies(res) == plain_run and len(plain_run[0]) == 1


def test_blank_lines_and_the_fallback(engine, data_dir, tmp_path, plain_run):
    """a blank line between FASTA records adds nothing, by the definition: the device route takes the file.  A file that opens with a
    blank line is refused (its first byte is neither '@' nor '>'); fasta.read_fasta accepts it, so the run goes through the fallback.
    Both give the plain file's outputs"""
    names, seqs = fasta.read_fasta(data_dir + "/reads.fasta")
    between = b"".join(b">%s\n%s\n\n" % (n.encode(), s.encode()) for n, s in zip(names, seqs))
    for text, falls_back in ((between, False), (b"\n" + between, True)):
        reads = tmp_path / ("reads%d.fasta.gz" % falls_back)
        reads.write_bytes(R.gz(text))
        assert (fasta.load_reads(str(reads), engine) is None) == falls_back == isinstance(R.parse(text), tuple)
        w = CountedReader()
        try:
            res = telr.run(telr.get_args(argv_for(data_dir, reads, tmp_path / ("out%d" % falls_back), *MM2)), engine=engine)
        finally:
            w.mp.undo()
        assert (str(reads) in w.paths) == falls_back
        assert bodies(res) == plain_run


def test_alignment_keep_qual_same_bam_stream(engine, data_dir, tmp_path):
    rng = random.Random(5)
    names, seqs = fasta.read_fasta(data_dir + "/reads.fasta")
    text = b"".join(b"@%s\n%s\n+\n%s\n" % (n.encode(), s.encode(), bytes(rng.randrange(33, 127) for _ in s)) for n, s in zip(names, seqs))
    plain, gzp = tmp_path / "rrrr.fastq", tmp_path / "r.fastq.gz"          # (names of one length: the @PG line holds the path)
    plain.write_bytes(text); gzp.write_bytes(R.gz(text))
    streams = []
    for reads in (plain, gzp):
        bam = str(tmp_path / (reads.name + ".bam"))
        w = CountedReader()
        try:
            alignment(bam, str(reads), data_dir + "/ref_38kb.fasta", str(tmp_path), "s", 1, "minimap2", "ont", engine=engine, keep_qual=True)
        finally:
            w.mp.undo()
        wait_release()
        assert str(reads) not in w.paths
        raw = B.inflate_file(open(bam, "rb").read())[0]
        streams.append(raw.replace(str(reads).encode(), str(plain).encode()))
    assert streams[0] == streams[1] and len(streams[0]) > 10000
    assert b"\xff" * 50 not in streams[1]                                   # QUAL is there
