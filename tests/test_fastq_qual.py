"""The FASTQ quality lines as telr_fasta_load keeps them (telr_fasta_qual / telr_fasta_qual_off; host code, no device): the views
must hold exactly the file's quality lines -- in place (the mapped file) and on the copying path (CR line ends, TELR_AB=fasta_copy)
-- while names, bases, offsets and lengths stay what they were; a FASTA has none; a quality line of another length than its
sequence line is refused (TELR_E_ARG: fasta.load() hands the file to the Python reader)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from telr_amd import _lib
from telr_amd._abi import TELR_E_ARG
from telr_amd.fasta import FastaFile, load, read_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QCHARS = "".join(chr(33 + v) for v in range(94))          # every Phred value 0..93


def _records(seed, n, lens=None):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(lens[i]) if lens is not None else int(rng.integers(1, 300))
        seq = "".join("ACGTN"[x] for x in rng.integers(0, 5, L))
        qual = "".join(QCHARS[x] for x in rng.integers(0, 94, L))
        out.append(("r%d" % i, seq, qual))
    return out


def _text(recs, plus_name=False, eol="\n", final_eol=True, blank_between=0):
    parts = []
    for name, seq, qual in recs:
        parts.append("@%s some text%s%s%s+%s%s%s%s" % (name, eol, seq, eol, name if plus_name else "", eol, qual, eol) + eol * blank_between)
    t = "".join(parts)
    if not final_eol:
        t = t.rstrip("\r\n")
    return t


def _check(path, recs, in_place):
    f = FastaFile(str(path))
    try:
        assert f.names == [r[0] for r in recs]
        assert f.seqs() == [r[1] for r in recs]
        assert f.qual is not None
        assert f.quals() == [r[2] for r in recs]
        buf, off = f.qual
        assert off.dtype == np.int64 and len(off) == len(recs)
        if in_place:          # nothing was copied: the buffer is the file, the offsets are where the quality lines start in it
            raw = open(str(path), "rb").read()
            assert len(f.triple[0]) == len(raw) and len(buf) == len(raw)
            for (name, seq, qual), o in zip(recs, off):
                if qual:
                    assert raw[int(o):int(o) + len(qual)] == qual.encode()
        else:
            assert len(f.triple[0]) == f.bases
    finally:
        f.close()


def test_plain_four_line_file(tmp_path):
    recs = _records(1, 300)
    p = tmp_path / "plain.fq"
    p.write_text(_text(recs))
    _check(p, recs, in_place=True)


def test_every_phred_value_survives(tmp_path):
    recs = [("all", ("ACGT" * 24)[:94], QCHARS)]
    p = tmp_path / "all.fq"
    p.write_text(_text(recs))
    _check(p, recs, in_place=True)


def test_quality_lines_that_begin_with_at_and_plus(tmp_path):
    recs = [("a", "ACGTA", "@IIII"), ("b", "GGC", "+@+"), ("c", "T", "@"), ("d", "AC", "++"), ("e", "ACGT", "!~!~")]
    p = tmp_path / "at.fq"
    p.write_text(_text(recs))
    _check(p, recs, in_place=True)


def test_plus_line_repeats_the_name(tmp_path):
    recs = _records(2, 40)
    p = tmp_path / "plus.fq"
    p.write_text(_text(recs, plus_name=True))
    _check(p, recs, in_place=True)


def test_crlf_line_ends_take_the_folded_path(tmp_path):
    recs = _records(3, 120) + [("z", "", "")]
    p = tmp_path / "crlf.fq"
    p.write_bytes(_text(recs, eol="\r\n").encode())
    _check(p, recs, in_place=False)


def test_zero_length_read_no_final_newline_and_blank_lines(tmp_path):
    recs = [("a", "ACGT", "IIII"), ("empty", "", ""), ("b", "GG", "#$")]
    p = tmp_path / "zero.fq"
    p.write_text(_text(recs))
    _check(p, recs, in_place=True)
    q = tmp_path / "nofinal.fq"
    q.write_text(_text(_records(4, 25), final_eol=False))
    _check(q, _records(4, 25), in_place=True)
    b = tmp_path / "blank.fq"
    b.write_text("\n\n" + _text(_records(5, 70), blank_between=2))
    _check(b, _records(5, 70), in_place=True)


def test_copying_path_in_a_child_process(tmp_path):
    """TELR_AB=fasta_copy is read once per process: the qualities are copied next to the bases, the same strings come out"""
    recs = _records(6, 150)
    p = tmp_path / "copy.fq"
    p.write_text(_text(recs))
    code = ("import sys; sys.path.insert(0, %r)\nfrom telr_amd.fasta import FastaFile\nf = FastaFile(sys.argv[1])\n"
            "import hashlib\nprint(len(f.triple[0]) == f.bases, hashlib.sha1('\\n'.join(f.quals()).encode()).hexdigest(), hashlib.sha1('\\n'.join(f.seqs()).encode()).hexdigest())" % ROOT)
    import hashlib
    hq = hashlib.sha1("\n".join(r[2] for r in recs).encode()).hexdigest()
    hs = hashlib.sha1("\n".join(r[1] for r in recs).encode()).hexdigest()
    for env, copied in (({}, "False"), ({"TELR_AB": "fasta_copy"}, "True")):
        r = subprocess.run([sys.executable, "-c", code, str(p)], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        assert r.stdout.decode().split() == [copied, hq, hs], (env, r.stdout)


def test_fasta_and_empty_file_have_no_qualities(tmp_path):
    p = tmp_path / "a.fa"
    p.write_text(">a\nACGT\n>b\nGG\nTT\n")
    f = FastaFile(str(p))
    assert f.qual is None and f.quals() is None
    L = _lib.lib()
    assert L.telr_fasta_qual(f.h) is None and L.telr_fasta_qual_off(f.h) is None
    f.close()
    e = tmp_path / "e.fq"
    e.write_text("")
    f = FastaFile(str(e))
    assert f.n == 0 and f.qual is None
    f.close()
    assert _lib.lib().telr_fasta_qual(None) is None


@pytest.mark.parametrize("qual", ["III", "IIIII", ""])
def test_quality_line_of_another_length_is_refused(tmp_path, qual):
    p = tmp_path / "bad.fq"
    p.write_text("@a\nACGT\n+\nIIII\n@b\nACGT\n+\n%s\n@c\nAC\n+\nII\n" % qual)
    with pytest.raises(_lib.TelrError) as ei:
        FastaFile(str(p))
    assert ei.value.code == TELR_E_ARG
    assert load(str(p)) is None          # the caller's Python reader decides


def test_python_reader_agrees_with_the_c_reader(tmp_path):
    recs = _records(7, 90) + [("q@", "ACG", "@+@")]
    p = tmp_path / "py.fq"
    p.write_text(_text(recs, plus_name=True))
    names, seqs, quals = read_fasta(str(p), with_qual=True)
    f = FastaFile(str(p))
    assert names == f.names and seqs == f.seqs() and quals == f.quals() == [r[2] for r in recs]
    f.close()
    assert read_fasta(str(p)) == (names, seqs)          # the two-list form is what it was
    a = tmp_path / "py.fa"
    a.write_text(">x\nACGT\n")
    assert read_fasta(str(a), with_qual=True) == (["x"], ["ACGT"], None)
