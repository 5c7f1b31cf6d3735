"""FASTQ base qualities in QUAL of the SAM / BAM writers (telr_seqset_attach_qual -> k_bam_write, the fourth deflate class;
telr_write_bam_qual, telr_write_sam_qual; telr_alignment.alignment(keep_qual=True)).

Records come from the edit-script builder of tests/bam_edges.py (no mapper: every kind of record is there by construction, and
the precondition test holds the set to that), qualities from a seeded generator.  Every file is inflated with zlib (its CRC
check covers the BGZF framing) and parsed with struct; the expected QUAL of a record is derived here from the read's FASTQ
values, the record's FLAG (0x4, 0x10) and the clip operations of its own CIGAR -- not from any writer.  Bytes, no tolerance."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_edges as be
import bam_reference as br
from telr_amd._abi import F_SECONDARY, F_SUPPL, TELR_E_ARG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 3, 4, 5, 6, 63, 64, 65, 2049, 2050, 3003, 4100)          # l_seq mod 4: 1 3 0 1 2 3 0 1 1 2 3 0


def _case():
    rng = np.random.default_rng(101)
    T = [be.rseq(rng, 60000), be.rseq(rng, 30000)]
    b = be.Builder(T, seed=7)
    k = 0
    for n in LENGTHS:
        for nl in range(2, 10):          # the name's length moves the QUAL field over the four byte alignments
            for rev in (False, True):
                b.read(name="%02x" % k + "n" * (nl - 2)).rec(k % 2, 100 + 11 * k, [("=", n - 1), ("X", 1)] if n > 1 else [("=", 1)], rev=rev)
                k += 1
    sc = [("=", 30), ("X", 1), ("=", 10), ("I", 2), ("=", 20), ("D", 3), ("=", 25)]
    long_sc = [("=", 700), ("I", 3), ("=", 900), ("D", 2), ("=", 650)]
    for rev in (False, True):
        for left, right in ((7, 0), (0, 9), (5, 11)):          # soft-clipped primaries
            b.read(left=left, right=right).rec(0, 20000 + 10 * left + right, sc, rev=rev)
        # a chimeric read: primary + supplementary on the other strand (+ a secondary over the same piece); a repeat: primary + secondary
        b.read(left=13, right=6).rec(0, 30000, long_sc, rev=rev).rec(1, 500, sc, rev=not rev, kind=F_SUPPL, gap=4).dup(kind=F_SECONDARY)
        b.read(left=2).rec(1, 9000, sc, rev=rev).rec(0, 41000, long_sc, rev=rev, kind=F_SUPPL, gap=1)
        b.read().rec(1, 12000, long_sc, rev=rev).dup(kind=F_SECONDARY, mapq=0)
    for n in (0, 1, 2, 3, 7, 64, 2049):
        b.unmapped(be.rseq(rng, n))
    soft = b.case("qual_soft", "qual", flags=be.ALL)
    hard = be.with_flags(soft, "qual_hard", be.MD | be.CS)
    assert be.check_case(soft) is None
    # Phred values over the whole range, 0 and 93 in every read long enough to hold them
    quals = []
    for r in soft["reads"]:
        q = rng.integers(0, 94, len(r)).astype(np.uint8)
        if len(q) >= 8:
            q[1] = 0; q[-2] = 93; q[0] = 93; q[-1] = 0
        quals.append(q)
    return soft, hard, quals


def _peaked_case():
    """long reads whose qualities follow a binomial around Q12: QUAL dominates the stream"""
    rng = np.random.default_rng(202)
    T = [be.rseq(rng, 200000)]
    b = be.Builder(T, seed=9)
    for i in range(60):
        n = 3000 + 37 * i
        b.read().rec(0, 100 + 3000 * i, [("=", n // 2), ("X", 1), ("=", n - n // 2 - 1)], rev=bool(i & 1))
    c = b.case("qual_peaked", "qual", flags=be.ALL)
    quals = [rng.binomial(40, 0.3, len(r)).astype(np.uint8) for r in c["reads"]]
    return c, quals


def _qstrings(quals):
    return [bytes(q + 33) for q in quals]


def _records(raw):
    """parse_records plus the QUAL bytes, at the offset bam_reference computes p_qual with"""
    out = []
    for p, refid, pos, bn, mapq, flag, name, cig, lseq, seq, tags in br.parse_records(raw):
        lrn = raw[p + 12]
        p_qual = p + 36 + lrn + 4 * len(cig) + (lseq + 1) // 2
        out.append(dict(off=p, flag=flag, name=name, cig=cig, l_seq=lseq, p_qual=p_qual, qual=raw[p_qual:p_qual + lseq]))
    return out


def _expected_qual(rec, q):
    """from the read's own values, the record's FLAG and the clips of its CIGAR"""
    if rec["flag"] & 4:
        return bytes(q)
    if rec["l_seq"] == 0:
        return b""
    o = q[::-1] if rec["flag"] & 0x10 else q
    cig = rec["cig"]
    lead = cig[0] >> 4 if cig[0] & 15 == 5 else 0
    trail = cig[-1] >> 4 if len(cig) > 1 and cig[-1] & 15 == 5 else 0
    return bytes(o[lead:len(o) - trail])


def _check_quals(raw, qnames, quals, what):
    by_name = dict(zip(qnames, quals))
    recs = _records(raw)
    bad = []
    for i, r in enumerate(recs):
        want = _expected_qual(r, by_name[r["name"]])
        if len(want) != r["l_seq"] or r["qual"] != want:
            k = next((j for j in range(min(len(want), len(r["qual"]))) if want[j] != r["qual"][j]), -1)
            bad.append("%s record %d (%s flag %#x l_seq %d, QUAL at %d mod 4): first difference at byte %d: %r / %r" % (
                what, i, r["name"], r["flag"], r["l_seq"], r["p_qual"] & 3, k, r["qual"][max(0, k - 4):k + 8], want[max(0, k - 4):k + 8]))
    assert not bad, "%d records:\n%s" % (len(bad), "\n".join(bad[:20]))
    return recs


def _mask_qual(raw, recs):
    m = bytearray(raw)
    for r in recs:
        m[r["p_qual"]:r["p_qual"] + r["l_seq"]] = b"\xff" * r["l_seq"]
    return bytes(m)


class Written:
    pass


def _write_all(engine, c, quals, tmp, tag):
    """the case through the device writer (levels 0 and 1, with and without qualities), the host writer and the SAM writer"""
    from telr_amd.presets import preset
    fl = c["flags"]
    kw = dict(md=bool(fl & be.MD), cs=bool(fl & be.CS), softclip=bool(fl & be.SOFT), rg=c["rg"], cmdline="t")
    ix = engine.index(c["targets"], preset("map-ont")[0])
    r = ix.result_from_arrays(c["alns"], c["cigars"])
    w = Written()
    w.path = {}
    try:
        plain = engine.seqset(c["reads"])
        assert not plain.has_qual
        qset = engine.seqset(c["reads"], qual=_qstrings(quals))
        assert qset.has_qual
        for name, s, level in (("plain0", plain, 0), ("plain1", plain, 1), ("dev0", qset, 0), ("dev1", qset, 1)):
            p = os.path.join(tmp, "%s_%s.bam" % (tag, name))
            ix.write_bam_device(r, s, c["qnames"], c["tnames"], p, index=True, level=level, **kw)
            w.path[name] = p
        # a quality below the offset: refused, and the set is left without qualities
        badq = _qstrings(quals)
        k = next(i for i, q in enumerate(badq) if len(q) > 2)
        badq[k] = badq[k][:1] + b" " + badq[k][2:]
        from telr_amd.aligner import _qual_arrays
        buf, off = _qual_arrays(badq)
        third = engine.seqset(c["reads"], qual=_qstrings(quals))
        w.bad_rc = engine.L.telr_seqset_attach_qual(engine.h, third.h, buf.ctypes.data, off.ctypes.data, 33)
        w.bad_has = third.has_qual
        p = os.path.join(tmp, "%s_refused.bam" % tag)
        ix.write_bam_device(r, third, c["qnames"], c["tnames"], p, index=False, level=1, **kw)
        w.path["refused"] = p
        p = os.path.join(tmp, "%s_host.bam" % tag)
        ix.write_bam(r, c["qnames"], c["reads"], c["tnames"], c["targets"], p, index=True, level=1, qual=_qstrings(quals), **kw)
        w.path["host"] = p
        p = os.path.join(tmp, "%s_host_plain.bam" % tag)
        ix.write_bam(r, c["qnames"], c["reads"], c["tnames"], c["targets"], p, index=False, level=1, **kw)
        w.path["host_plain"] = p
        for name, q in (("sam", _qstrings(quals)), ("sam_plain", None)):
            p = os.path.join(tmp, "%s_%s.sam" % (tag, name))
            ix.write_sam(r, c["qnames"], c["reads"], c["tnames"], c["targets"], p, coordinate_sorted=True, header=False, qual=q, **kw)
            w.path[name] = p
        # the slice writer goes through the same kernels: one rank that holds every record
        p = os.path.join(tmp, "%s_slice.bam" % tag)
        open(p, "wb").close()
        seg = ix.write_bam_slice(r, qset, c["qnames"], c["tnames"], np.ones(len(c["alns"]), np.uint8), with_header=True, level=1, **kw)
        try:
            ix.segment_write(seg, p, 0, True)
        finally:
            ix.segment_free(seg)
        w.path["slice"] = p
        for s in (plain, qset, third):
            s.free()
    finally:
        ix.free_raw(r)
        ix.free()
    w.raw = {k: br.read_bgzf(p)[0] for k, p in w.path.items() if p.endswith(".bam")}
    return w


@pytest.fixture(scope="module")
def inputs():
    return _case()


@pytest.fixture(scope="module", params=["soft", "hard"])
def written(request, engine, inputs, tmp_path_factory):
    soft, hard, quals = inputs
    c = soft if request.param == "soft" else hard
    return c, quals, _write_all(engine, c, quals, str(tmp_path_factory.mktemp("q" + request.param)), request.param)


def test_the_generator_makes_every_kind_of_record(inputs):
    """precondition: a shortfall of the inputs fails here instead of passing below"""
    soft, hard, quals = inputs
    allq = np.concatenate(quals)
    assert set(np.unique(allq)) == set(range(94)), "Phred values 0..93"
    assert sorted(set(len(r) for r in soft["reads"]) & set(LENGTHS)) == sorted(LENGTHS)
    for c, clipop in ((soft, 4), (hard, 5)):
        s = be.stream_of(c)
        ps = br.parse_records(s.raw)
        kinds = set()
        combos = set()
        for r, p in zip(s.recs, ps):
            fl = r["flag"]
            kinds.add("unmapped" if fl & 4 else "secondary" if fl & 0x100 else "supplementary" if fl & 0x800 else "reverse" if fl & 0x10 else "forward")
            if r["l_seq"]:
                combos.add((r["p_qual"] & 3, r["l_seq"] & 3, bool(fl & 0x10)))
            if fl & 0x800:
                assert p[7][0] & 15 == clipop or p[7][-1] & 15 == clipop, "clip operation of the supplementary records"
                assert (r["l_seq"] < len(c["reads"][r["qid"]])) == (clipop == 5)
            if fl & 0x100:
                assert r["l_seq"] == 0
        assert kinds == {"forward", "reverse", "supplementary", "secondary", "unmapped"}, kinds
        assert any(r["flag"] & 0x800 and r["flag"] & 0x10 for r in s.recs) and any(r["flag"] & 0x800 and not r["flag"] & 0x10 for r in s.recs)
        assert len(combos) == 32, "QUAL alignment x l_seq mod 4 x strand: %d of 32" % len(combos)
        for n in LENGTHS:
            assert {r["p_qual"] & 3 for r in s.recs if r["l_seq"] == n} == {0, 1, 2, 3}, "QUAL alignments of l_seq %d" % n
        assert any(r["flag"] & 4 and r["l_seq"] == 0 for r in s.recs) and any(r["flag"] & 4 and r["l_seq"] > 2000 for r in s.recs)


def test_qual_of_every_record(written):
    """1. every record's QUAL, in every file with qualities"""
    c, quals, w = written
    for k in ("dev0", "dev1", "host", "slice"):
        recs = _check_quals(w.raw[k], c["qnames"], quals, k)
        assert len(recs) == len(be.stream_of(c).recs)


def test_nothing_else_moved(written):
    """2. with QUAL masked out the stream is the one written without qualities; 6. which holds 0xff and equals the plain encoder's"""
    c, quals, w = written
    s = be.stream_of(c)
    assert w.raw["plain0"] == s.raw and w.raw["plain1"] == s.raw and w.raw["host_plain"] == s.raw
    recs = _records(w.raw["plain0"])
    assert all(r["qual"] == b"\xff" * r["l_seq"] for r in recs)
    for k in ("dev0", "dev1", "host", "slice"):
        assert _mask_qual(w.raw[k], _records(w.raw[k])) == w.raw["plain0"], k


def test_three_writers_one_stream(written):
    """3. device (both levels), host and SAM agree"""
    c, quals, w = written
    assert w.raw["dev0"] == w.raw["dev1"] == w.raw["host"] == w.raw["slice"]
    recs = _records(w.raw["dev1"])
    lines = [l.split("\t") for l in open(w.path["sam"]).read().splitlines()]
    plain = [l.split("\t") for l in open(w.path["sam_plain"]).read().splitlines()]
    assert len(lines) == len(recs) == len(plain)
    for r, l, pl in zip(recs, lines, plain):
        assert l[0] == r["name"] and int(l[1]) == r["flag"]
        want = "*" if r["l_seq"] == 0 else bytes(b + 33 for b in r["qual"]).decode()
        assert l[10] == want, (r["name"], r["flag"])
        assert len(l[9]) == r["l_seq"] or l[9] == "*"
        assert pl[10] == "*" and l[:10] + l[11:] == pl[:10] + pl[11:]          # the other columns did not move


def test_index_of_the_quality_file(written):
    """4. the .bai passes the walk of tools/validate_bam.py, and equals the plain encoder's index"""
    c, quals, w = written
    for k in ("dev1", "dev0", "host"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "validate_bam.py"), w.path[k], str(len(be.stream_of(c).recs))], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert '"bai_linear_entries": null' not in p.stdout
    s = be.stream_of(c)
    got, blocks = br.read_bgzf(w.path["dev1"])
    br.compare_bai(open(w.path["dev1"] + ".bai", "rb").read(), blocks, br.bai_reference(s, [len(t) for t in c["targets"]]))


def test_refused_qualities_leave_the_set_without(written):
    """7. a byte below the offset: TELR_E_ARG, and the set writes 0xff"""
    c, quals, w = written
    assert w.bad_rc == TELR_E_ARG and w.bad_has is False
    assert w.raw["refused"] == w.raw["plain1"]


def test_level_1_codes_qual_with_its_own_table(engine, tmp_path):
    """5. peaked qualities (binomial around Q12): the level-1 file is smaller than the level-0 file"""
    c, quals = _peaked_case()
    w = _write_all(engine, c, quals, str(tmp_path), "peaked")
    _check_quals(w.raw["dev1"], c["qnames"], quals, "peaked level 1")
    assert w.raw["dev0"] == w.raw["dev1"] == w.raw["host"]
    n0, n1 = os.path.getsize(w.path["dev0"]), os.path.getsize(w.path["dev1"])
    p0, p1 = os.path.getsize(w.path["plain0"]), os.path.getsize(w.path["plain1"])
    nb = sum(len(q) for q in quals)
    print("peaked qualities, %d bases: level 0 %d bytes, level 1 %d bytes (%.3f B/base; QUAL alone %.3f B/base); without qualities %d / %d" % (
        nb, n0, n1, n1 / nb, (n1 - p1) / nb, p0, p1))
    assert n1 < n0


def test_alignment_keep_qual(engine, tmp_path, data_dir):
    """8. alignment(keep_qual=True) on a FASTQ: check 1 on its BAM; keep_qual=False: the stream it always wrote (QUAL 0xff)"""
    from telr_amd.fasta import read_fasta, revcomp
    from telr_amd.telr_alignment import alignment, wait_release
    rng = np.random.default_rng(303)
    names, seqs = read_fasta(os.path.join(data_dir, "reads.fasta"))
    names, seqs = names[:40], seqs[:40]
    names += ["rc%d" % i for i in range(5)] + ["noise"]
    seqs += [revcomp(s) for s in seqs[:5]] + [be.rseq(rng, 700)]
    quals = [rng.binomial(40, 0.3, len(s)).astype(np.uint8) for s in seqs]
    quals[0][:4] = (0, 93, 0, 93)
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for n, s, q in zip(names, seqs, quals):
            f.write(b"@" + n.encode() + b" x\n" + s.encode() + b"\n+\n" + bytes(q + 33) + b"\n")
    ref = os.path.join(data_dir, "ref_38kb.fasta")
    raws = {}
    for keep in (True, False):
        bam = str(tmp_path / ("keep%d.bam" % keep))
        alignment(bam, str(fq), ref, str(tmp_path), "s", 1, "minimap2", "ont", engine=engine, keep_qual=keep)
        wait_release()
        raws[keep] = br.read_bgzf(bam)[0]
    recs = _check_quals(raws[True], names, quals, "alignment")
    fl = [r["flag"] for r in recs]
    assert any(f & 4 for f in fl) and any(f & 0x10 and not f & 0x900 for f in fl) and any(not f & 0x914 for f in fl), "forward, reverse and unmapped records"
    plain = _records(raws[False])
    assert all(r["qual"] == b"\xff" * r["l_seq"] for r in plain)
    assert _mask_qual(raws[True], recs) == raws[False]
