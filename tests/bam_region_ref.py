"""What telr_bam_load_regions is documented to compute (include/telr_hip.h), stated in plain Python on top of
tests/bam_in_ref.py (the whole-file definition) and reg2bin of tests/bam_reference.py:

  * merge_regions / ref_span / select: the regions, a record's reference span, which records are selected;
  * filtered_stream / load: the header and exactly the selected records in file order, through bam_in_ref.load_stream;
  * write_bai: a .bai in virtual offsets from a file's own member cuts (SAM specification 5.2);
  * reg2bins / plan: the bins of a region, the index's chunks -> intervals;
  * interval_members / header_members / walked: what a load inflates and walks;
  * record_set / layouts / cases: the generated file of the GPU test and the case table; every case asserts the edge it claims.
"""
import struct

import numpy as np

import bam_in_ref as R
from bam_reference import reg2bin

E_ARG, E_RANGE, E_IO = R.E_ARG, R.E_RANGE, R.E_IO
REGION_INFO = ("regions", "intervals", "members", "header_members", "walked", "selected")
MAX_COOR = 1 << 29


# ---- regions and selection ------------------------------------------------------------------------------------------------------
def merge_regions(regions, tlens, n_ref=None):
    """[(tid, beg, end[, reserved])] -> disjoint ascending [(tid, beg, end)]; tlens None: no clip to the targets (telr_bai_plan)"""
    n_ref = len(tlens) if n_ref is None else n_ref
    out = []
    for i, r in enumerate(regions):
        tid, beg, end = r[:3]
        if len(r) > 3 and r[3]:
            raise R.BamInError(E_ARG, "region %d: the reserved field is not 0" % i)
        if tid < 0 or tid >= n_ref:
            raise R.BamInError(E_ARG, "region %d: tid outside the header's targets" % i)
        if beg < 0:
            raise R.BamInError(E_ARG, "region %d: beg below 0" % i)
        end = min(end, MAX_COOR) if tlens is None else min(end, MAX_COOR, tlens[tid])
        if end <= beg:
            raise R.BamInError(E_ARG, "region %d: end at or below beg" % i)
        out.append((tid, beg, end))
    out.sort()
    merged = []
    for tid, beg, end in out:
        if merged and merged[-1][0] == tid and beg <= merged[-1][2]:
            merged[-1] = (tid, merged[-1][1], max(merged[-1][2], end))
        else:
            merged.append((tid, beg, end))
    return merged


def ref_span(r):
    """a parsed record (bam_in_ref.parse_stream) -> M + D of the CIGAR in force, at least 1; None for an unmapped one"""
    if r["flag"] & 4 or r["refid"] < 0:
        return None
    ops = r["ops"]
    if len(ops) == 2 and ops[0] == (r["lseq"] << 4 | 4) and ops[1] & 15 == 3 and r["cg"] is not None:
        ops = r["cg"]
    _, _, _, sm, _, sd = R.normalise(ops)
    return max(1, sm + sd)


def is_selected(r, merged):
    span = ref_span(r)
    return span is not None and any(t == r["refid"] and r["pos"] < e and r["pos"] + span > b for t, b, e in merged)


def record_offsets(raw):
    """-> (length of the header, [offset of every record], the stream's end)"""
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    head, offs = p, []
    while p < len(raw):
        offs.append(p); p += 4 + struct.unpack_from("<i", raw, p)[0]
    assert p == len(raw)
    return head, offs, p


def filtered_stream(raw, merged):
    """the header and exactly the selected records, in file order -> (stream, indices of the selected records)"""
    head, offs, end = record_offsets(raw)
    _, _, recs = R.parse_stream(raw)
    keep = [k for k, r in enumerate(recs) if "err" not in r and is_selected(r, merged)]
    ends = offs[1:] + [end]
    return raw[:head] + b"".join(raw[offs[k]:ends[k]] for k in keep), keep


# ---- the index ----------------------------------------------------------------------------------------------------------------
def member_table(data):
    """[(file offset of the member, inflated bytes before it, ISIZE)]"""
    out, start, u = [], 0, 0
    for off, n, isize, _ in R.hop(data):
        out.append((start, u, isize)); start = off + n + 8; u += isize
    return out


def voffset(members, u, at_end=False):
    """the virtual offset of inflated byte u: in the member that holds it; an end that falls on a seam stays in the member before it
    when at_end, as a writer that has not flushed its block says it"""
    for k, (start, u0, isize) in enumerate(members):
        if u0 <= u < u0 + isize or (at_end and u == u0 + isize and isize):
            return start << 16 | (u - u0)
    k = max(k for k, m in enumerate(members) if m[1] <= u)          # the stream's end: behind the last byte
    return members[k][0] << 16 | (u - members[k][1])


def write_bai(data, merge=True, fill=True, ends_stay=False, pseudo=True):
    """the .bai of a coordinate-sorted file.  merge: neighbouring records of a bin become one chunk when the first ends in the member the
    second starts in (samtools); else one chunk per record.  fill: an untouched 16-kb window repeats the one before (samtools); else 0"""
    raw, _, _ = R.inflate_file(data)
    members = member_table(data)
    tnames, tlens, recs = R.parse_stream(raw)
    head, offs, end = record_offsets(raw)
    ends = offs[1:] + [end]
    refs = [dict(bins={}, lin=[], meta=None) for _ in tlens]
    n_no_coor = 0
    for k, r in enumerate(recs):
        if r["refid"] < 0:
            n_no_coor += 1
            continue
        span = ref_span(r) or 1
        X = refs[r["refid"]]
        vb, ve = voffset(members, offs[k]), voffset(members, ends[k], ends_stay)
        ch = X["bins"].setdefault(reg2bin(r["pos"], r["pos"] + span), [])
        if merge and ch and ch[-1][1] >> 16 == vb >> 16:
            ch[-1][1] = ve
        else:
            ch.append([vb, ve])
        for w in range(r["pos"] >> 14, ((r["pos"] + span - 1) >> 14) + 1):
            while len(X["lin"]) <= w:
                X["lin"].append(0)
            if X["lin"][w] == 0:
                X["lin"][w] = vb
        m = X["meta"]
        X["meta"] = [vb if m is None else m[0], ve, (0 if m is None else m[2]) + 1, 0]          # (the pseudo-bin, by the rule of bam_reference.bai_reference)
    out = b"BAI\1" + struct.pack("<i", len(refs))
    for X in refs:
        if fill:
            for w in range(1, len(X["lin"])):
                if X["lin"][w] == 0:
                    X["lin"][w] = X["lin"][w - 1]
        out += struct.pack("<i", len(X["bins"]) + (1 if pseudo and X["meta"] else 0))
        for b in sorted(X["bins"]):
            out += struct.pack("<Ii", b, len(X["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in X["bins"][b])
        if pseudo and X["meta"]:
            out += struct.pack("<IiQQQQ", 37450, 2, *X["meta"])
        out += struct.pack("<i", len(X["lin"])) + struct.pack("<%dQ" % len(X["lin"]), *X["lin"])
    return out + struct.pack("<Q", n_no_coor)


def parse_bai(bai, n_ref):
    """-> [(bins {bin: [(vbeg, vend)]}, linear [...])] per reference; BamInError as the engine refuses"""
    def need(p, n, what):
        if p + n > len(bai):
            raise R.BamInError(E_ARG, "%s runs past the index's end" % what)
    need(0, 8, "the magic")
    if bai[:4] != b"BAI\1":
        raise R.BamInError(E_ARG, "no BAI magic")
    if struct.unpack_from("<i", bai, 4)[0] != n_ref:
        raise R.BamInError(E_ARG, "the index holds another number of references")
    p, refs = 8, []
    for _ in range(n_ref):
        need(p, 4, "a bin count")
        n_bin = struct.unpack_from("<i", bai, p)[0]; p += 4
        if n_bin < 0:
            raise R.BamInError(E_ARG, "a bin count runs past the index's end")
        bins = {}
        for _ in range(n_bin):
            need(p, 8, "a bin")
            b, nch = struct.unpack_from("<Ii", bai, p); p += 8
            if nch < 0:
                raise R.BamInError(E_ARG, "a chunk count runs past the index's end")
            need(p, 16 * nch, "a chunk")
            if b != 37450:
                bins.setdefault(b, []).extend(struct.unpack_from("<QQ", bai, p + 16 * c) for c in range(nch))
            p += 16 * nch
        need(p, 4, "the linear index")
        n_intv = struct.unpack_from("<i", bai, p)[0]; p += 4
        if n_intv < 0:
            raise R.BamInError(E_ARG, "the linear index runs past the index's end")
        need(p, 8 * n_intv, "the linear index")
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, p)))); p += 8 * n_intv
    return refs


def reg2bins(beg, end):
    """SAM specification 5.3: every bin that may hold a record overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def plan(bai, n_ref, merged):
    """merged regions -> the intervals [(vbeg, vend)]"""
    refs = parse_bai(bai, n_ref)
    chunks = []
    for tid, beg, end in merged:
        bins, lin = refs[tid]
        w = beg >> 14
        min_off = lin[w] if w < len(lin) else 0
        for b in reg2bins(beg, end):
            chunks += [(cb, ce) for cb, ce in bins.get(b, []) if cb < ce and ce > min_off]
    chunks.sort()
    out = []
    for cb, ce in chunks:
        if out and cb >> 16 <= out[-1][1] >> 16:
            out[-1][1] = max(out[-1][1], ce)
        else:
            out.append([cb, ce])
    return [tuple(x) for x in out]


def interval_members(data, intervals):
    """per interval the members it inflates: [(index of the first, one behind the last)]"""
    members = member_table(data)
    at = {m[0]: k for k, m in enumerate(members)}
    return [(at[vb >> 16], at[ve >> 16] + (1 if ve & 0xffff else 0)) for vb, ve in intervals]


def header_members(data, raw):
    head, _, _ = record_offsets(raw)
    members = member_table(data)
    return next(k + 1 for k, m in enumerate(members) if m[1] + m[2] >= head)


def walked(data, raw, intervals):
    """the records inside the intervals: [index], in file order"""
    members = member_table(data)
    at = {m[0]: m[1] for m in members}
    _, offs, _ = record_offsets(raw)
    spans = [(at[vb >> 16] + (vb & 0xffff), at[ve >> 16] + (ve & 0xffff)) for vb, ve in intervals]
    return [k for k, o in enumerate(offs) if any(a <= o < b for a, b in spans)]


class Ref:
    pass


def load(data, bai, regions, keep_qual=False):
    """the whole definition: file bytes, index bytes, regions -> bam_in_ref.Loaded of the filtered stream, with counters["members"] =
    the members inflated for the intervals, and region_info (dict), selected (record indices), intervals"""
    raw, _, no_eof = R.inflate_file(data)
    tnames, tlens, _ = R.parse_stream(raw[:record_offsets(raw)[0]])
    merged = merge_regions(regions, tlens)
    intervals = plan(bai, len(tlens), merged) if merged else []
    im = interval_members(data, intervals)
    stream, keep = filtered_stream(raw, merged)
    w = walked(data, raw, intervals)
    assert set(keep) <= set(w), "the index misses a selected record"
    L = R.load_stream(stream, keep_qual, sum(b - a for a, b in im), no_eof)
    L.selected, L.intervals, L.walked, L.merged = keep, intervals, w, merged
    L.region_info = dict(zip(REGION_INFO, (len(merged), len(intervals), sum(b - a for a, b in im), header_members(data, raw), len(w), len(keep))))
    return L


# ---- the generated file ---------------------------------------------------------------------------------------------------------
TNAMES, TLENS = ["chrA", "chrB", "chrC"], [4600000, 100000, 60000]
N_WINDOWS = 264            # chrA: one plain record per 16-kb window
N_CLUSTER = 220            # chrC: a dense run of short records in one window
W16, W128 = 20 * 16384, 8 * 16384          # a 16-kb seam that is no 128-kb seam, and one that is (bin level 585 / 73 above it)


def record_set(placed=False):
    """-> [(name, record bytes)] in coordinate order: about 500 records of 50 to 400 bases on chrA and chrC, none on chrB.  placed: with
    the unmapped record that has a place on chrA"""
    rng = np.random.RandomState(520)
    out = []

    def rec(name, tid, pos, cigar, flag=0, mapq=40, seq_len=None, tags=b""):
        ops = R.ops_of(cigar)
        n = sum(o >> 4 for o in ops if o & 15 in (0, 1, 4, 7, 8)) if seq_len is None else seq_len
        out.append((tid, pos, name, R.bam_record(name, flag, tid, pos, mapq, ops, R._dna(rng, n), bytes(rng.randint(0, 60, n).astype(np.uint8)), tags)))
    for w in range(N_WINDOWS):
        n = int(rng.randint(50, 401))
        a = int(rng.randint(10, n - 20))
        rec("w%d" % w, 0, w * 16384 + 5000, ["%dM" % n, "%dM3I%dM" % (a, n - a - 3), "%dM5D%dM" % (a, n - a), "7S%dM" % (n - 7)][w % 4], flag=0x10 * (w & 1))
    # the seams of the linear index and of the bin levels
    rec("ends_at_w16", 0, W16 - 100, "100M")
    rec("spans_w16", 0, W16 - 60, "120M")
    rec("starts_at_w16", 0, W16, "80M")
    rec("ends_at_w128", 0, W128 - 90, "90M")
    rec("spans_w128", 0, W128 - 50, "60M40D50M")
    rec("starts_at_w128", 0, W128, "70M")
    rec("ins_only", 0, 40 * 16384 + 9000, "25I30S")                # I and S only: span 1
    rec("placed_unmapped", 0, 41 * 16384 + 9000, "", flag=4, seq_len=60)
    rec("split", 0, 50 * 16384 + 9000, "200H150M", flag=0x800)      # its primary lies on chrC
    # chrC: a dense cluster of short records in one 16-kb window, the primary of "split", and one record far behind the cluster
    rec("split", 2, 900, "200M150S")
    for i in range(N_CLUSTER):
        rec("c%d" % i, 2, 2000 + 37 * i, "%dM" % int(rng.randint(50, 90)), flag=0x10 * (i & 1))
    rec("c_span", 2, 16340, "100M")                               # across a 16-kb seam: it lives in the coarser bin
    rec("cg_span", 2, 30000, "100S100N", tags=R.tag_cg(R.ops_of("60M300D40M")))          # the CG array is in force: 400 bases of reference, not 100
    rec("c_last", 2, 40000, "300M")
    out.sort(key=lambda x: (x[0], x[1]))
    return [(name, b) for _, _, name, b in out if placed or name != "placed_unmapped"]


def unmapped_tail():
    rng = np.random.RandomState(521)
    return [("u%d" % i, R.bam_record("u%d" % i, 4, -1, -1, 0, (), R._dna(rng, 80), bytes(rng.randint(0, 60, 80).astype(np.uint8)))) for i in range(3)]


_FILES = {}


def layout(name):
    """-> dict(data, bai, raw, names (per record), starts): the record set under a BGZF layout.  mid: every member seam lies inside a
    record, so every record straddles; big: members of 65,280 bytes (several bins' chunks in one member); kb: a seam every 1,000
    bytes; unmapped: `mid` with a placed unmapped record on chrA and unmapped records appended; no_eof: `mid` without the EOF marker, ends said in the member before a seam;
    per_record: `mid` with one chunk per record and unset linear windows left 0"""
    if name in _FILES:
        return _FILES[name]
    recs = record_set(name == "unmapped") + (unmapped_tail() if name == "unmapped" else [])
    head = R.bam_header(TNAMES, TLENS)
    stream = head + b"".join(b for _, b in recs)
    starts, p = [], len(head)
    for _, b in recs:
        starts.append(p); p += len(b)
    if name == "big":
        cuts = None
    elif name == "kb":
        cuts = list(range(1000, len(stream), 1000))
    else:
        cuts = [s + 30 for s in starts]
    data = R.bgzf(stream, cuts, eof=name != "no_eof")
    bai = write_bai(data, merge=name != "per_record", fill=name != "per_record", ends_stay=name == "no_eof")
    _FILES[name] = dict(data=data, bai=bai, raw=stream, names=[n for n, _ in recs], starts=starts, head=len(head))
    return _FILES[name]


def _pos(name, which=0):
    """(tid, pos, end) of the record(s) of that name in the record set"""
    F = layout("mid")
    _, _, recs = R.parse_stream(F["raw"])
    hits = [(r["refid"], r["pos"], r["pos"] + ref_span(r)) for r, n in zip(recs, F["names"]) if n == name and ref_span(r) is not None]
    return hits[which]


def cases():
    """[dict(name, layout, regions, keep_qual, chunk_bytes, claim)]: claim(L, names) asserts the edge, L = load(...) of the case, names =
    the selected records' names"""
    cs = []

    def add(name, lay, regions, claim, keep_qual=False, chunk_bytes=1 << 40):
        cs.append(dict(name=name, layout=lay, regions=regions, keep_qual=keep_qual, chunk_bytes=chunk_bytes, claim=claim))
    t, p, e = _pos("w100")
    add("end_at_pos", "mid", [(t, p - 50, p)], lambda L, n: "w100" not in n and not n)
    add("end_behind_pos", "mid", [(t, p - 50, p + 1)], lambda L, n: n == ["w100"])
    add("start_at_end", "mid", [(t, e, e + 50)], lambda L, n: not n)
    add("start_before_end", "mid", [(t, e - 1, e + 50)], lambda L, n: n == ["w100"])
    t, p, e = _pos("ins_only")
    add("ins_only_span_1", "mid", [(t, p, p + 1), (t, p + 1, p + 2000)], lambda L, n, p=p, e=e: n == ["ins_only"] and e == p + 1)
    add("ins_only_behind", "mid", [(t, p + 1, p + 2000)], lambda L, n: not n)
    add("w16_left", "mid", [(0, W16 - 1, W16)], lambda L, n: n == ["ends_at_w16", "spans_w16"])
    add("w16_right", "mid", [(0, W16, W16 + 1)], lambda L, n: n == ["spans_w16", "starts_at_w16"])
    add("w128_left", "mid", [(0, W128 - 1, W128)], lambda L, n: n == ["ends_at_w128", "spans_w128"])
    add("w128_right", "mid", [(0, W128 + 59, W128 + 60)], lambda L, n: n == ["spans_w128", "starts_at_w128"])          # (inside the spanning record's deletion)
    add("empty_target", "mid", [(1, 0, 100000)], lambda L, n: not n and L.region_info["intervals"] == 0)
    add("behind_the_linear_index", "mid", [(2, 50000, 60000)], lambda L, n: not n and L.region_info["walked"] >= 1)          # (c_span's coarser bin is read: nothing cuts it)
    add("placed_unmapped_not_selected", "unmapped", [(0, 41 * 16384, 42 * 16384)], lambda L, n: n == ["w41"] and L.region_info["walked"] >= 2)
    add("unsorted_overlapping", "mid", [(2, 3000, 4000), (0, 16384 * 3, 16384 * 5), (2, 1000, 3500), (0, 16384 * 4, 16384 * 4 + 1), (0, 0, 16384)],
        lambda L, n: L.region_info["regions"] == 3 and n[:3] == ["w0", "w3", "w4"] and "split" in n)
    add("zero_regions", "mid", [], lambda L, n: not n and L.region_info["members"] == 0 and L.region_info["header_members"] >= 1)
    everything = [(0, 0, TLENS[0]), (1, 0, TLENS[1]), (2, 0, TLENS[2])]
    add("every_target", "mid", everything, lambda L, n: n == layout("mid")["names"], keep_qual=True)          # no unmapped record: the whole file
    add("every_target_unmapped_added", "unmapped", everything, lambda L, n: n == layout("mid")["names"] and len(layout("unmapped")["names"]) == len(n) + 4,
        keep_qual=True)
    add("mid_member_start", "big", [(0, 30 * 16384, 31 * 16384)], lambda L, n: n == ["w30"] and L.intervals[0][0] & 0xffff > 0)
    add("seam_behind_start", "kb", [(0, 29 * 16384, 30 * 16384)],
        lambda L, n: n == ["w29"] and L.intervals[0][0] & 0xffff > 0 and (L.intervals[0][1] >> 16) > (L.intervals[0][0] >> 16))
    def two_in_one(L, n):
        bins = parse_bai(layout("big")["bai"], 3)[0][0]
        a, b = bins[4681 + 30], bins[4681 + 31]          # one chunk each, of two bins, starting in one member
        return n == ["w30", "w31"] and len(a) == len(b) == 1 and a[0] != b[0] and a[0][0] >> 16 == b[0][0] >> 16 and L.region_info["intervals"] == 1
    add("two_chunks_one_member", "big", [(0, 30 * 16384, 32 * 16384)], two_in_one)

    def at_the_end(L, n):
        F = layout("mid")
        members = member_table(F["data"])
        return n == ["c_last"] and L.intervals[-1][1] == voffset(members, len(F["raw"])) == members[-1][0] << 16 and members[-1][2] == 0
    add("ends_at_file_end", "mid", [(2, 39000, 41000)], at_the_end)          # the interval's end is the EOF marker's member, offset 0
    t, p, e = _pos("cg_span")
    add("cg_span_in_force", "mid", [(t, p + 200, p + 250)], lambda L, n, p=p, e=e: n == ["cg_span"] and e == p + 400)          # the raw 100N would end at p + 100
    add("no_eof", "no_eof", [(2, 39000, 41000), (0, 0, 16384)], lambda L, n: n == ["w0", "c_last"] and L.counters["no_eof"] == 1)
    add("every_member_a_chunk", "mid", [(0, 16384 * 60, 16384 * 70), (2, 0, 60000)], lambda L, n: len(n) == 10 + N_CLUSTER + 4, keep_qual=True, chunk_bytes=1)
    add("every_member_a_chunk_kb", "kb", [(0, 16384 * 60, 16384 * 70), (2, 0, 60000)], lambda L, n: len(n) == 10 + N_CLUSTER + 4, keep_qual=True, chunk_bytes=1)
    every_other = [(0, 16384 * w, 16384 * (w + 1)) for w in range(0, N_WINDOWS, 2)]
    add("many_intervals_one_chunk", "per_record", every_other, lambda L, n: L.region_info["intervals"] >= 130 and L.region_info["intervals"] % 64 != 0)
    add("short_intervals_next_to_a_long_one", "per_record", every_other[:40] + [(2, 1900, 11000)],
        lambda L, n: 40 < L.region_info["intervals"] <= 64 and sum(1 for x in n if x.startswith("c")) == N_CLUSTER)
    t, p, e = _pos("split", 0)
    add("orphan", "mid", [(t, p, e)], lambda L, n: n == ["split"] and L.counters["orphans"] == 1 and L.counters["reads"] == 0 and L.counters["kept"] == 0)
    add("qualities_kept", "kb", [(0, 0, 16384 * 30)], lambda L, n: L.quals is not None and len(n) > 30, keep_qual=True, chunk_bytes=4000)
    add("qualities_dropped", "kb", [(0, 0, 16384 * 30)], lambda L, n: L.quals is None, chunk_bytes=4000)
    return cs
