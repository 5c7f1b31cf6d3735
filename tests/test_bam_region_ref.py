"""The region load's definition (tests/bam_region_ref.py) against hand-derived answers; telr_bai_plan (a host export: no device) against
the reference's plan for every case; the case table held to what it claims; telr_alignment.parse_regions; the refusals with their codes;
and the reference's .bai writer held to the rules of tests/bam_reference.py (bai_reference / compare_bai) on the generated file."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_in_ref as R
import bam_reference as BR
import bam_region_ref as G
from telr_amd import _lib
from telr_amd.aligner import Engine
from telr_amd.telr_alignment import parse_regions, split_region_specs

CASES = G.cases()
E_ARG, E_RANGE, E_IO = -3, -4, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def v(c, u):
    return c << 16 | u


# ---- 1. the definition by hand -----------------------------------------------------------------------------------------------------
def test_regions_by_hand():
    tl = [1000, 500]
    assert G.merge_regions([], tl) == []
    assert G.merge_regions([(1, 5, 9), (0, 10, 20), (0, 20, 30), (0, 0, 5)], tl) == [(0, 0, 5), (0, 10, 30), (1, 5, 9)]          # touching merges, a gap does not
    assert G.merge_regions([(0, 10, 50), (0, 20, 30)], tl) == [(0, 10, 50)]                                                    # one inside the other
    assert G.merge_regions([(0, 990, 5000)], tl) == [(0, 990, 1000)]                                                           # clipped to the target
    assert G.merge_regions([(0, 990, 5000)], None, n_ref=2) == [(0, 990, 5000)]
    for bad in ([(2, 0, 1)], [(-1, 0, 1)], [(0, -1, 1)], [(0, 5, 5)], [(0, 6, 5)], [(0, 1000, 2000)], [(0, 0, 1, 7)]):
        with pytest.raises(R.BamInError) as e:
            G.merge_regions(bad, tl)
        assert e.value.code == E_ARG


def test_reg2bins_by_hand():
    assert G.reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681]
    assert G.reg2bins(16383, 16385) == [0, 1, 9, 73, 585, 4681, 4682]
    assert G.reg2bins((1 << 17) - 1, (1 << 17) + 1) == [0, 1, 9, 73, 585, 586, 4681 + 7, 4681 + 8]
    assert G.reg2bins(0, 1 << 29)[-1] == 37448 and len(G.reg2bins(0, 1 << 29)) == 37449
    for beg, end in ((0, 1), (100, 16384), (16000, 17000), (131000, 132000), (5 << 20, (5 << 20) + 1), (0, 1 << 29)):
        assert BR.reg2bin(beg, end) in G.reg2bins(beg, end)          # a record's own bin is among those of its span


def test_span_and_selection_by_hand():
    def rec(cigar, pos=100, flag=0, refid=0, lseq=10, cg=None):
        return dict(flag=flag, refid=refid, pos=pos, ops=R.ops_of(cigar), lseq=lseq, cg=cg)
    assert G.ref_span(rec("10M")) == 10
    assert G.ref_span(rec("5M3D5M2I")) == 13
    assert G.ref_span(rec("4S6I")) == 1 and G.ref_span(rec("")) == 1
    assert G.ref_span(rec("10M", flag=4)) is None and G.ref_span(rec("10M", refid=-1)) is None
    assert G.ref_span(rec("10S7N", cg=R.ops_of("4M2D6M"))) == 12          # the CG array is in force
    assert G.ref_span(rec("10S7N")) == 7                                  # without the tag the record's own words are
    r = rec("10M")                                                        # [100, 110)
    assert not G.is_selected(r, [(0, 50, 100)]) and G.is_selected(r, [(0, 50, 101)])
    assert not G.is_selected(r, [(0, 110, 200)]) and G.is_selected(r, [(0, 109, 200)])
    assert not G.is_selected(r, [(1, 0, 1000)])
    assert G.is_selected(rec("6I"), [(0, 100, 101)]) and not G.is_selected(rec("6I"), [(0, 101, 102)])


def hand_bai(refs, tail=True):
    """[(bins {bin: [(vbeg, vend)]}, linear [...])] -> index bytes"""
    out = b"BAI\1" + struct.pack("<i", len(refs))
    for bins, lin in refs:
        out += struct.pack("<i", len(bins))
        for b, ch in bins.items():
            out += struct.pack("<Ii", b, len(ch)) + b"".join(struct.pack("<QQ", *c) for c in ch)
        out += struct.pack("<i", len(lin)) + struct.pack("<%dQ" % len(lin), *lin)
    return out + (struct.pack("<Q", 0) if tail else b"")


HAND_REFS = [({4681: [(v(0, 100), v(0, 900)), (v(0, 950), v(200, 0)), (v(300, 5), v(300, 5))],          # the third is empty
               4682: [(v(200, 10), v(400, 7))],
               585: [(v(0, 40), v(0, 100)), (v(900, 0), v(950, 0))],
               37450: [(1, 2), (3, 4)]},
              [v(0, 100), v(200, 10)]),
             ({}, [])]
HAND_PLANS = [
    # window 0's entry is v(0, 100): 585's chunk (v(0, 40), v(0, 100)) ends AT it and is dropped, 4681's empty chunk is dropped, its other
    # two merge because the second starts in the member in which the first ends; 585's second chunk lies members away
    ([(0, 0, 10)], [(v(0, 100), v(200, 0)), (v(900, 0), v(950, 0))]),
    ([(0, 16384, 16385)], [(v(200, 10), v(400, 7)), (v(900, 0), v(950, 0))]),          # bin 4682, and what window 1's entry leaves of 585
    # both: v(200, 10) starts in the member in which v(200, 0) ends -- the rule is on members, not on bytes -- and 585's chunk comes twice
    ([(0, 16384, 16385), (0, 0, 10)], [(v(0, 100), v(400, 7)), (v(900, 0), v(950, 0))]),
    ([(0, 40000, 40001)], [(v(0, 40), v(0, 100)), (v(900, 0), v(950, 0))]),            # behind the last linear entry: nothing is cut
    ([(1, 0, 100)], []),
    ([], []),
]


def test_plan_by_hand():
    bai = hand_bai(HAND_REFS)
    for regions, want in HAND_PLANS:
        assert G.plan(bai, 2, G.merge_regions(regions, None, n_ref=2)) == want, regions
    assert G.plan(hand_bai(HAND_REFS, tail=False), 2, [(0, 0, 10)]) == HAND_PLANS[0][1]          # n_no_coor is optional


# ---- 2. the case table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_claims_its_edge(case):
    F = G.layout(case["layout"])
    L = G.load(F["data"], F["bai"], case["regions"], case["keep_qual"])
    assert case["claim"](L, [F["names"][k] for k in L.selected])
    assert L.region_info["selected"] <= L.region_info["walked"]


def test_generated_file_is_what_the_cases_need():
    F = G.layout("mid")
    _, _, recs = R.parse_stream(F["raw"])
    assert 300 <= len(recs) <= 600 and all(50 <= r["lseq"] <= 400 for r in recs)
    members = G.member_table(F["data"])
    seams = {m[1] for m in members[1:]}
    assert len(members) > len(recs) and not seams & set(F["starts"])          # every seam lies inside a record: every record straddles
    assert len(F["raw"]) < 1 << 20
    assert len(G.member_table(G.layout("big")["data"])) <= 5


# ---- 3. telr_bai_plan ----------------------------------------------------------------------------------------------------------------
def c_plan(path, n_ref, regions, cap=None, n_regions=None, null_regions=False):
    L = _lib.lib()
    reg = np.zeros((max(len(regions), 1), 4), np.int32)
    for i, r in enumerate(regions):
        reg[i, :len(r)] = r
    cap = 4096 if cap is None else cap
    vb, ve = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint64)
    n = C.c_int64(-1)
    rc = L.telr_bai_plan(None if path is None else str(path).encode(), n_ref, len(regions) if n_regions is None else n_regions,
                         None if null_regions else reg.ctypes.data, vb.ctypes.data, ve.ctypes.data, cap, C.byref(n))
    return rc, int(n.value), [(int(a), int(b)) for a, b in zip(vb[:min(cap, max(int(n.value), 0))], ve)]


@pytest.fixture(scope="module")
def bai_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bai")
    out = {}
    for name in sorted({c["layout"] for c in CASES}):
        out[name] = d / (name + ".bai")
        out[name].write_bytes(G.layout(name)["bai"])
    out["hand"] = d / "hand.bai"
    out["hand"].write_bytes(hand_bai(HAND_REFS))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_c_plan_equals_the_reference_plan(case, bai_files):
    F = G.layout(case["layout"])
    want = G.plan(F["bai"], 3, G.merge_regions(case["regions"], None, n_ref=3)) if case["regions"] else []
    rc, n, got = c_plan(bai_files[case["layout"]], 3, case["regions"])
    assert (rc, n, got) == (0, len(want), want)
    vb, ve = Engine.bai_plan(bai_files[case["layout"]], 3, case["regions"])
    assert list(zip(vb.tolist(), ve.tolist())) == want
    if len(want) > 1:          # more intervals than cap: the first cap of them, the exact count
        assert c_plan(bai_files[case["layout"]], 3, case["regions"], cap=1) == (E_RANGE, len(want), want[:1])


def test_c_plan_by_hand(bai_files):
    for regions, want in HAND_PLANS:
        assert c_plan(bai_files["hand"], 2, regions) == (0, len(want), want), regions


def test_c_plan_refusals(bai_files, tmp_path):
    L = _lib.lib()
    good = bai_files["mid"]
    assert c_plan(tmp_path / "none.bai", 3, [(0, 0, 10)])[0] == E_IO and b"cannot open" in L.telr_bai_plan_error()
    for bad in ([(3, 0, 1)], [(-1, 0, 1)], [(0, -1, 1)], [(0, 5, 5)], [(0, 6, 5)], [(0, 0, 1, 7)]):
        assert c_plan(good, 3, bad)[0] == E_ARG, bad
        assert L.telr_bai_plan_error().startswith(b"telr_bai_plan: region 0")
    assert c_plan(good, 3, [], n_regions=-1)[0] == E_ARG
    assert c_plan(good, 3, [(0, 0, 1)], null_regions=True)[0] == E_ARG
    assert c_plan(good, 2, [(0, 0, 10)])[0] == E_ARG and b"references" in L.telr_bai_plan_error()          # another file's index
    data = G.layout("mid")["bai"]
    p = tmp_path / "bad.bai"
    p.write_bytes(b"BAJ\1" + data[4:])
    assert c_plan(p, 3, [(0, 0, 10)])[0] == E_ARG and b"magic" in L.telr_bai_plan_error()
    # truncations: the C reader and the reference's agree on which are still an index (only the trailing n_no_coor may go)
    for cut in list(range(1, 40)) + [len(data) // 2, len(data) - 9, len(data) - 4]:
        p.write_bytes(data[:len(data) - cut])
        try:
            G.parse_bai(data[:len(data) - cut], 3)
            want = 0
        except R.BamInError as e:
            want = e.code
        assert c_plan(p, 3, [(0, 0, 10)])[0] == want, cut
        assert (want == 0) == (cut <= 8)
    # counts that run past the file's end
    n_bin_at = 8
    for at, val in ((n_bin_at, 1 << 30), (n_bin_at, -1), (n_bin_at + 8, 1 << 27), (n_bin_at + 8, -5)):
        b = bytearray(data)
        struct.pack_into("<i", b, at, val)
        p.write_bytes(bytes(b))
        assert c_plan(p, 3, [(0, 0, 10)])[0] == E_ARG, (at, val)
        with pytest.raises(R.BamInError):
            G.parse_bai(bytes(b), 3)
    assert c_plan(good, 3, [])[:2] == (0, 0)


# ---- 4. region texts -----------------------------------------------------------------------------------------------------------------
def test_parse_regions():
    tn, tl = ["chr2L", "chr2R", "HLA:A", "HLA"], [1000, 5000000, 300, 200]
    assert parse_regions(["chr2L"], tn, tl) == [(0, 0, 1000)]
    assert parse_regions(["chr2L:1-10", "chr2R:1,000,001-2,000,000"], tn, tl) == [(0, 0, 10), (1, 1000000, 2000000)]
    assert parse_regions(["chr2L:500"], tn, tl) == [(0, 499, 1000)]
    assert parse_regions(["chr2L:990-2000"], tn, tl) == [(0, 989, 1000)]          # an end behind the target is clipped
    assert parse_regions(["chr2L:7-7"], tn, tl) == [(0, 6, 7)]
    assert parse_regions(["HLA:A"], tn, tl) == [(2, 0, 300)]                        # a name with a colon matches whole first
    assert parse_regions(["HLA:A:5-9", "HLA:5-9"], tn, tl) == [(2, 4, 9), (3, 4, 9)]
    assert parse_regions([b"chr2L"[:].decode()], [b"chr2L"], [10]) == [(0, 0, 10)]
    assert parse_regions([], tn, tl) == []
    # one option holds several specs; a comma that groups digits does not separate
    assert split_region_specs("chr2L:32,000-34,000") == ["chr2L:32,000-34,000"]
    assert split_region_specs("chr2R:1,000,001-2,000,000,chr2L,sites,chr2L:5-9") == ["chr2R:1,000,001-2,000,000", "chr2L", "sites", "chr2L:5-9"]
    assert split_region_specs("chr2L:1,000-2000,chr2L:500") == ["chr2L:1,000-2000", "chr2L:500"]
    assert split_region_specs("1,2,,3:4-5,666") == ["1", "2", "3:4-5,666"] and split_region_specs("") == []
    for bad in ("chrX", "chrX:1-5", "chr2L:0-5", "chr2L:5-4", "chr2L:a-5", "chr2L:1-", "chr2L:-5", "chr2L:1001", "chr2L:1-2-3", "chr2L:", "chr2L:1.5-3", ""):
        with pytest.raises(ValueError) as e:
            parse_regions([bad], tn, tl)
        assert repr(bad) in str(e.value)


# ---- 5. the reference's .bai writer against the rules of tests/bam_reference.py ------------------------------------------------------------
@pytest.mark.parametrize("lay", ["mid", "big", "kb", "unmapped"])
def test_bai_writer_follows_the_bam_writers_rules(lay):
    F = G.layout(lay)
    raw = F["raw"]
    _, _, recs = R.parse_stream(raw)
    head, offs, end = G.record_offsets(raw)
    rows = []
    for r, o, e in zip(recs, offs, offs[1:] + [end]):
        span = G.ref_span(r) or 1
        rows.append(dict(tid=r["refid"], pos=r["pos"], end=r["pos"] + span, off=o, size=e - o, bin=BR.reg2bin(r["pos"], r["pos"] + span) if r["refid"] >= 0 else 4680))
    ref_index = BR.bai_reference(BR.Stream(raw, head, offs, rows), G.TLENS)
    blocks = [(start, u0, isize) for start, u0, isize in G.member_table(F["data"])]
    BR.compare_bai(F["bai"], blocks, ref_index)
    # and the per-record writer: the same records covered, no chunk merged
    per = BR.parse_bai(G.write_bai(F["data"], merge=False))
    assert sum(len(c) for X in per["refs"] for c in X["bins"].values()) == sum(1 for r in rows if r["tid"] >= 0)


# ---- 6. bai_plan.h on the CPU under the sanitizers -------------------------------------------------------------------------------------------
def test_host_program_under_sanitizers(tmp_path):
    """tools/ubench/bai_plan_host.cpp = telr_amd/csrc/bai_plan.h compiled for the CPU with -fsanitize=address,undefined, a program of
    its own: a valid index, every truncation of it, and copies with counts and bin numbers overwritten"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bai_plan_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "ubench", "bai_plan_host.cpp"), "-o", exe])
    idx = tmp_path / "mid.bai"
    idx.write_bytes(G.layout("mid")["bai"])
    p = subprocess.run([exe, str(idx)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert ", 0 failures" in p.stdout and "3 regions -> 1 intervals" in p.stdout
