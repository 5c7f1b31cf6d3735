"""The SAM text of telr_write_sam against the plain encoder of tests/bam_reference.py: every hand-built case of
tests/bam_edges.py whose edge is in the records themselves (groups walk, layout and sa, and sort_equal_keys_and_strands) goes
through telr_result_from_arrays and Index.write_sam, coordinate-sorted and in the order of the reads, header on, and the whole
file must equal the reference stream decoded to text (bam_reference.sam_text): strings, no tolerance.  The cases of the 8-Mb and
64-Mb targets and the groups framing and deflate are left to tests/test_gpu_bam_edges.py: their edges are in BGZF and the sort.
tests/test_bam_reference.py holds the decoder to lines written out by hand, on the CPU."""
import os
import re

import pytest

import bam_edges as be
import bam_reference as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return be.walk_cases() + be.layout_cases() + be.sort_cases(big=False) + be.sa_cases()


def _first_difference(got, want):
    g, w = got.split("\n"), want.split("\n")
    k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
    return "%d / %d lines, first difference in line %d:\n%r\n%r" % (len(g), len(w), k, (g + [""])[k][:400], (w + [""])[k][:400])


def _written(engine, c, tmp, **kw):
    """the case through Index.write_sam with its own flags (TELR_SAM_NO_UNMAPPED is the wrapper's unmapped=False)"""
    from telr_amd.presets import preset
    fl = c["flags"]
    ix = engine.index(c["targets"], preset("map-ont")[0])
    r = ix.result_from_arrays(c["alns"], c["cigars"])
    p = os.path.join(tmp, "out.sam")
    try:
        ix.write_sam(r, c["qnames"], c["reads"], c["tnames"], c["targets"], p, md=bool(fl & be.MD), cs=bool(fl & be.CS), softclip=bool(fl & be.SOFT), rg=c["rg"],
                     cmdline="t", unmapped=not fl & be.NO_UNMAPPED, header=True, **kw)
    finally:
        ix.free_raw(r); ix.free()
    return open(p).read()


@pytest.mark.parametrize("group", ["walk", "layout", "sort", "sa"])
def test_sam_text_equals_the_decoded_stream(engine, cases, tmp_path, group):
    mine = [c for c in cases if c["group"] == group]
    assert len(mine) >= (1 if group == "sort" else 2)
    bad = []
    for c in mine:
        assert be.check_case(c) is None, c["name"]
        s = be.stream_of(c)
        for srt in (True, False):
            got, want = _written(engine, c, str(tmp_path), coordinate_sorted=srt), br.sam_text(s, coordinate_sorted=srt)
            if got != want:
                bad.append("%s %s: %s" % (c["name"], "sorted" if srt else "unsorted", _first_difference(got, want)))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_the_cases_without_unmapped_reads_are_among_them(cases):
    assert sorted(c["name"] for c in cases if c["flags"] & be.NO_UNMAPPED) == ["layout_no_unmapped", "layout_zero_records"]
    assert "layout_long_cigar" in [c["name"] for c in cases] and len(cases) >= 30
    assert [c["name"] for c in cases if c["group"] == "sort"] == ["sort_equal_keys_and_strands"]


@pytest.mark.parametrize("name", ["layout_suppl_hard", "sa_groups"])
def test_primary_only_drops_secondary_and_supplementary_lines(engine, cases, tmp_path, name):
    c = next(c for c in cases if c["name"] == name)
    s = be.stream_of(c)
    assert any(r["flag"] & 0x100 for r in s.recs) and any(r["flag"] & 0x800 for r in s.recs)
    for srt in (True, False):
        got = _written(engine, c, str(tmp_path), coordinate_sorted=srt, primary_only=True)
        want = br.sam_text(s, coordinate_sorted=srt, keep=lambda f: not f & 0x900)
        assert got == want, _first_difference(got, want)


def test_qualities_in_column_11(engine, cases, tmp_path):
    """Phred + 33 strings of the reads' lengths: column 11 is the read's string, reversed where FLAG has 0x10, cut to the bases
    SEQ holds where the record is hard-clipped, `*` where SEQ is `*`; every other column as without qualities"""
    c = next(c for c in cases if c["name"] == "layout_suppl_hard")
    quals = ["".join(chr(33 + (7 * q + 3 * x) % 94) for x in range(len(rd))) for q, rd in enumerate(c["reads"])]
    s = be.stream_of(c)
    seen = set()
    for srt in (True, False):
        want = br.sam_text(s, coordinate_sorted=srt).split("\n")
        for k, l in enumerate(want):
            if not l or l[0] == "@":
                continue
            f = l.split("\t")
            q = quals[c["qnames"].index(f[0])]
            hard, m = "H" in f[5], re.match(r"(\d+)H", f[5])
            lead = int(m.group(1)) if m else 0
            f[10] = "*" if f[9] == "*" else (q[::-1] if int(f[1]) & 16 else q)[lead:lead + len(f[9])]
            seen.add((bool(int(f[1]) & 16), hard, f[9] == "*"))
            want[k] = "\t".join(f)
        got = _written(engine, c, str(tmp_path), coordinate_sorted=srt, qual=quals)
        assert got == "\n".join(want), _first_difference(got, "\n".join(want))
    assert len(c["qnames"]) == len(set(c["qnames"])) and {(False, True, False), (True, True, False), (False, False, True), (False, False, False)} <= seen
