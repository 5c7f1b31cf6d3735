"""The chunk plan of telr_bam_load_chunked: tests/bam_chunks_ref.plan against hand-derived answers, telr_bam_chunk_plan (a host export: no
device) against it, and the seam cases of tests/test_gpu_bam_chunks.py held to what they claim -- well-formed files whose chunk seams lie
where the case's name says."""
import ctypes as C
from itertools import accumulate

import numpy as np
import pytest

import bam_in_ref as R
import bam_chunks_ref as K
from telr_amd import _lib
from telr_amd.aligner import Engine

SEAMS = K.seam_cases()
RECORD = R.record_cases()

# (ISIZE list, chunk_bytes, first member of every chunk), derived by hand from the rule
HAND = [
    ([], 1, []),                                                   # the empty file: no chunks
    ([], 1 << 20, []),
    ([0], 1, [0]),
    ([5], 1, [0]),                                                 # one member above chunk_bytes: a chunk of its own
    ([0, 0, 0], 1, [0]),                                           # zeros never close a chunk that is not above the limit
    ([5, 0, 0, 3], 1, [0, 1, 3]),                                  # 5 | 0 0 | 3: behind a chunk above the limit even a zero starts anew
    ([1, 0, 1, 0], 1, [0, 2]),                                     # 1 0 | 1 0: a zero joins a chunk that is exactly full
    ([3, 4, 5], 1, [0, 1, 2]),                                     # chunk_bytes = 1: one member per chunk
    ([10, 20, 30], 60, [0]),                                       # chunk_bytes = total
    ([10, 20, 30], 61, [0]),                                       # total + 1
    ([10, 20, 30], 59, [0, 2]),                                    # total - 1
    ([10, 20, 30], 30, [0, 2]),                                    # 10 20 | 30: exactly full, then exactly full
    ([10, 20, 30], 29, [0, 1, 2]),
    ([0, 10, 0, 20, 0, 30, 0], 30, [0, 5]),                        # 0 10 0 20 0 | 30 0
    ([65536, 65536, 1, 65536], 65536, [0, 1, 2, 3]),               # every sum of two neighbours is above 65,536
    ([70, 10, 10], 50, [0, 1]),                                    # a member above the limit, then two that fit together
]


@pytest.mark.parametrize("isize,c,want", HAND, ids=["%s@%d" % ("-".join(map(str, i)) or "empty", c) for i, c, _ in HAND])
def test_plan_by_hand(isize, c, want):
    assert K.plan(isize, c) == want


def c_plan(isize, c, cap=None):
    L = _lib.lib()
    a = np.ascontiguousarray(isize, dtype=np.int32)
    cap = len(a) if cap is None else cap
    first = np.full(max(cap, 1), -7, np.int64); n = C.c_int64(-1)
    rc = L.telr_bam_chunk_plan(len(a), a.ctypes.data, c, first.ctypes.data, cap, C.byref(n))
    return rc, int(n.value), [int(x) for x in first[:min(cap, max(int(n.value), 0))]]


def test_c_plan_equals_the_python_plan():
    for isize, c, want in HAND:
        assert c_plan(isize, c) == (0, len(want), want), (isize, c)
        assert [int(x) for x in Engine.bam_chunk_plan(isize, c)] == want
    rng = np.random.RandomState(11)
    for _ in range(300):
        n = int(rng.randint(0, 40))
        isize = [int(x) for x in rng.choice([0, 0, 1, 2, 100, 30000, 65535, 65536], n)]
        c = int(rng.choice([1, 2, 100, 65535, 65536, 65537, 200000, 1 << 40]))
        want = K.plan(isize, c)
        assert c_plan(isize, c) == (0, len(want), want), (isize, c)
        # the rule itself: no chunk but a single member is above c, and no chunk would still fit with its successor's first member
        sums = [sum(isize[a:b]) for a, b in zip(want, want[1:] + [n])]
        for k, (a, b) in enumerate(zip(want, want[1:] + [n])):
            assert b > a and (sums[k] <= c or b - a == 1)
            if b < n:
                assert sums[k] + isize[b] > c


def test_c_plan_codes():
    assert c_plan([1, 2], 0)[0] == R.E_ARG and c_plan([1, 2], -5)[0] == R.E_ARG
    assert c_plan([1, -2], 5)[0] == R.E_ARG
    rc, n, first = c_plan([5, 5, 5], 1, cap=2)                    # more chunks than cap: the count is exact, the first cap are written
    assert (rc, n, first) == (R.E_RANGE, 3, [0, 1])
    L = _lib.lib()
    assert L.telr_bam_chunk_plan(1, None, 5, None, 0, None) == R.E_ARG


def same_loaded(a, b):
    assert a.tnames == b.tnames and a.tlens == b.tlens and a.qnames == b.qnames and a.seqs == b.seqs and a.quals == b.quals
    assert a.counters == b.counters and a.alns.tobytes() == b.alns.tobytes() and a.cigars.tobytes() == b.cigars.tobytes()


@pytest.mark.parametrize("case", SEAMS + RECORD, ids=[c["name"] for c in SEAMS + RECORD])
def test_cases_are_well_formed(case):
    """the chunks' members concatenated are the file's stream: load_stream on them gives what load gives, at both small chunk sizes"""
    whole = R.load(case["data"], case["keep_qual"])
    ms = R.hop(case["data"])
    no_eof = 0 if case["data"][-28:] == R.EOF_MARKER else 1
    for c in (1, 65536):
        parts = K.chunk_streams(case["data"], c)
        assert len(parts) == len(K.plan([m[2] for m in ms], c))
        same_loaded(R.load_stream(b"".join(parts), case["keep_qual"], len(ms), no_eof), whole)


@pytest.mark.parametrize("case", [c for c in SEAMS if c["seam"]], ids=[c["name"] for c in SEAMS if c["seam"]])
def test_seam_is_where_the_case_claims(case):
    """record i starts `off` bytes before a chunk seam of chunk_bytes = 1"""
    i, off = case["seam"]
    start = K.record_starts(case["head"], case["recs"])[i]
    seams = list(accumulate(len(p) for p in K.chunk_streams(case["data"], 1)))[:-1]
    assert start + off in seams and start + off in K.member_cuts(case["data"])
    assert 0 <= off < len(case["recs"][i])
    rec = case["recs"][i]
    F = K._field_offsets(rec)
    where = {"block_size_1": (1, 2), "block_size_2": (2, 3), "block_size_3": (3, 4), "record_boundary": (0, 1), "inside_read_name": (F["name"] + 1, F["cigar"] - 1),
             "inside_cigar": (F["cigar"] + 1, F["seq"]), "inside_seq_odd_base": (F["seq"] + 1, F["qual"]), "inside_qual": (F["qual"] + 1, F["tags"]),
             "inside_b_tag": (F["tags"] + 8, F["tags"] + 8 + 40), "no_eof_marker": (F["qual"] + 1, F["tags"])}
    if case["name"] in where:
        lo, hi = where[case["name"]]
        assert lo <= off < hi
    if case["name"] == "inside_seq_odd_base":
        assert 2 * (off - F["seq"]) - 1 == 51                      # the last base before the seam is the odd base 51


def test_seam_cases_reach_what_they_name():
    by = {c["name"]: c for c in SEAMS}
    # the primary of `far` lies two chunks behind its supplementary and secondary records; the orphan is alone in the last data chunk
    c = by["supp_sec_two_chunks_before_primary_orphan_last"]
    parts = K.chunk_streams(c["data"], 1)
    where = lambda rec: next(k for k, p in enumerate(parts) if rec in p)
    supp, seco, prim, orph = c["recs"][0], c["recs"][1], c["recs"][8], c["recs"][-1]
    assert where(prim) - where(supp) >= 2 and where(prim) - where(seco) >= 2
    assert parts[-1] == b"" and parts[-2] == orph                  # (the EOF marker is the last chunk, the orphan the one before)
    L = R.load(c["data"], True)
    assert L.counters["orphans"] == 1 and sum(1 for a in L.alns if L.qnames[a["qid"]] == "far") == 3
    # first name wins: the two orders give different bases for `twice`
    a, b = R.load(by["first_name_wins_file_order"]["data"]), R.load(by["first_name_wins_reversed"]["data"])
    assert a.seqs[a.qnames.index("twice")] != b.seqs[b.qnames.index("twice")]
    assert a.counters["kept"] == b.counters["kept"] and a.qnames != b.qnames
    # the header spans more than two chunks of 65,536
    c = by["long_header"]
    assert len(c["head"]) > 2 * 65536 and len(K.chunk_streams(c["data"], 65536)) >= 3
    # the last chunk is the EOF marker only / no EOF marker
    assert K.chunk_streams(by["eof_marker_alone"]["data"], 1)[-1] == b"" and R.load(by["eof_marker_alone"]["data"]).counters["no_eof"] == 0
    assert R.load(by["no_eof_marker"]["data"]).counters["no_eof"] == 1
    # the one record without QUAL is alone in the last data chunk, and takes every read's qualities with it
    c = by["one_ff_in_the_last_chunk"]
    assert K.chunk_streams(c["data"], 1)[-2] == c["recs"][-1] and R.load(c["data"], True).quals is None
    assert R.load(R.bgzf(c["head"] + b"".join(c["recs"][:-1])), True).quals is not None


def test_filler_file_shape():
    """the memory-bound test's files: at least 64 members of about 4 MB, and twice that, with the same longest record"""
    d1 = K.filler_file(K.FILLER_COPIES)
    ms = R.hop(d1)
    assert len(ms) >= 64 and 3.5e6 < sum(m[2] for m in ms) < 5e6
