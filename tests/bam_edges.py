"""Hand-built records aimed at the branch points of the device BAM writer (telr_amd/csrc/bam_dev.hip.h: k_bam_scan / d_bam_walk,
k_bam_size, k_bam_write, d_bam_sa, k_bgzf_store, k_blk_first_rec, k_bgzf_deflate), without the mapper: every case is a dict
(name, group, targets, reads, qnames, tnames, alns (ALN_DTYPE), cigars, flags (TELR_SAM_*), rg) plus `reach`, a function of the
reference stream (tests/bam_reference.py) and the case that returns None when the case hits the edge it is aimed at and
otherwise what it missed.  tests/test_bam_reference.py checks, on the CPU, that every case is valid and reaches its edge;
tests/test_gpu_bam_edges.py runs every case through the writers and compares the files with the reference, byte for byte.

Records are built from an edit script over the target (Builder.rec): the builder derives the read, the CIGAR, qs / qe / te,
mlen and blen from it, so NM from a column walk equals blen - mlen; `check_case` restates the rules of telr_debug_check_records.

usage: python tests/bam_edges.py   (prints every case with what it reached)
"""
import os
import re
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

import bam_reference as br
from telr_amd._abi import ALN_DTYPE, F_PRIMARY, F_SECONDARY, F_SUPPL, F_REV

BAM_BLK = 65280          # BAM_BLK
DEFL_PIECE = 64          # DEFL_PIECE
DEFL_SEGCAP = 256        # DEFL_SEGCAP
DEFL_MINSEG = 192        # DEFL_MINSEG
MD, CS, SOFT, NO_UNMAPPED = br.SAM_MD, br.SAM_CS, br.SAM_SOFTCLIP, br.SAM_NO_UNMAPPED
ALL = MD | CS | SOFT
_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rseq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def other(b):
    return "ACGT"[("ACGT".find(b) + 1) % 4] if b in "ACGT" else "A"


class Builder:
    """reads made of pieces; every piece is one record, written as an edit script over the target:
    ("=", n) n columns copied, ("X", n) n mismatching columns, ("N", n) n columns with N in the read, ("I", n | bases),
    ("D", n).  `=`, `X` and `N` merge into M operations."""

    def __init__(self, targets, tnames=None, seed=1):
        self.targets = list(targets)
        self.tnames = list(tnames) if tnames else ["t%d" % i for i in range(len(self.targets))]
        self.rng = np.random.default_rng(seed)
        self.reads, self.qnames, self.recs, self.cur = [], [], [], None

    def read(self, name=None, left=0, right=0):
        """start a read; left / right: unaligned bases at its ends"""
        self._close()
        self.cur = dict(name=name if name is not None else "q%d" % len(self.reads), left=rseq(self.rng, left), right=rseq(self.rng, right), pieces=[])
        return self

    def unmapped(self, bases, name=None):
        self._close()
        self.reads.append(bases); self.qnames.append(name if name is not None else "q%d" % (len(self.reads) - 1))
        return self

    def rec(self, tid, ts, script, rev=False, kind=F_PRIMARY, gap=0, **fields):
        """one more piece of the current read (gap: unaligned read bases before it)"""
        t, ti = self.targets[tid], ts
        q, ops, mlen, blen = [], [], 0, 0
        for op, arg in script:
            if op in "=XN":
                for _ in range(arg):
                    tc = t[ti].upper()
                    qc = tc if op == "=" else ("N" if op == "N" else other(tc))
                    mlen += 1 if (op == "=" and tc in "ACGT") else 0
                    q.append(qc); ti += 1
                blen += arg
                if ops and ops[-1][0] == 0:
                    ops[-1][1] += arg
                else:
                    ops.append([0, arg])
            elif op == "I":
                s = arg if isinstance(arg, str) else rseq(self.rng, arg)
                q.append(s); blen += len(s); ops.append([1, len(s)])
            elif op == "D":
                ti += arg; blen += arg; ops.append([2, arg])
            else:
                raise ValueError(op)
        assert ti <= len(t), (ts, ti, len(t))
        for x, y in zip(ops, ops[1:]):
            assert x[0] != y[0], "adjacent operations of one kind"
        self.cur["pieces"].append(dict(tid=tid, ts=ts, te=ti, aligned="".join(q), cig=[n << 4 | o for o, n in ops], rev=rev, kind=kind, gap=rseq(self.rng, gap),
                                       mlen=mlen, blen=blen, fields=fields, same_as=None))
        return self

    def dup(self, kind=F_SECONDARY, **fields):
        """another record over the SAME piece of the read as the last one (same target interval, strand and CIGAR)"""
        p = dict(self.cur["pieces"][-1]); p["kind"] = kind; p["fields"] = fields; p["same_as"] = len(self.cur["pieces"]) - 1
        while self.cur["pieces"][p["same_as"]]["same_as"] is not None:
            p["same_as"] = self.cur["pieces"][p["same_as"]]["same_as"]
        self.cur["pieces"].append(p)
        return self

    def _close(self):
        c, self.cur = self.cur, None
        if c is None:
            return
        # the read in its own direction: left + (gap + piece as the read shows it)* + right
        read, spans = c["left"], []
        for p in c["pieces"]:
            if p["same_as"] is not None:
                spans.append(spans[p["same_as"]]); continue
            read += p["gap"]
            seg = revcomp(p["aligned"]) if p["rev"] else p["aligned"]
            spans.append((len(read), len(read) + len(seg))); read += seg
        read += c["right"]
        qid = len(self.reads)
        self.reads.append(read); self.qnames.append(c["name"])
        for p, (qs, qe) in zip(c["pieces"], spans):
            a = np.zeros(1, ALN_DTYPE)
            a["qid"] = qid; a["tid"] = p["tid"]; a["qlen"] = len(read); a["qs"] = qs; a["qe"] = qe; a["tlen"] = len(self.targets[p["tid"]])
            a["ts"] = p["ts"]; a["te"] = p["te"]; a["mlen"] = p["mlen"]; a["blen"] = p["blen"]; a["n_cigar"] = len(p["cig"])
            a["flags"] = p["kind"] | (F_REV if p["rev"] else 0); a["mapq"] = 60; a["score"] = p["mlen"]; a["cnt"] = max(1, p["mlen"] // 15)
            a["dp_score"] = 2 * p["mlen"] - 4 * (p["blen"] - p["mlen"]); a["subsc"] = 0
            for k, v in p["fields"].items():
                a[k] = v
            self.recs.append((a, p["cig"]))

    def case(self, name, group, flags=ALL, rg=None, reach=None, **extra):
        self._close()
        alns, cigs = [], []
        for a, c in self.recs:
            a = a.copy(); a["cigar_off"] = len(cigs); cigs += c; alns.append(a)
        alns = np.concatenate(alns) if alns else np.zeros(0, ALN_DTYPE)
        d = dict(name=name, group=group, targets=self.targets, tnames=self.tnames, reads=self.reads, qnames=self.qnames, alns=alns,
                 cigars=np.array(cigs, np.uint32), flags=flags, rg=rg, reach=reach, stored_last=False)
        d.update(extra)
        return d


def with_flags(case, name, flags, rg=None, reach=None):
    c = dict(case); c["name"] = name; c["flags"] = flags; c["rg"] = rg
    if reach is not None:
        c["reach"] = reach
    return c


def check_case(c):
    """the rules of telr_debug_check_records, plus: records of a read contiguous, qids ascending, names short enough, mlen / blen
    consistent with the CIGAR; -> None or what is wrong"""
    al, cg = c["alns"], c["cigars"]
    last_q = -1
    for i, a in enumerate(al):
        q, t = int(a["qid"]), int(a["tid"])
        if not (0 <= q < len(c["reads"]) and 0 <= t < len(c["targets"])):
            return "record %d: ids" % i
        if q < last_q:
            return "record %d: reads out of order" % i
        last_q = q
        if not (0 <= a["ts"] <= a["te"] <= len(c["targets"][t])) or a["tlen"] != len(c["targets"][t]):
            return "record %d: target interval" % i
        if a["qlen"] != len(c["reads"][q]) or not (0 <= a["qs"] <= a["qe"] <= a["qlen"]):
            return "record %d: query interval" % i
        if a["n_cigar"] <= 0 or a["cigar_off"] < 0 or a["cigar_off"] + a["n_cigar"] > len(cg):
            return "record %d: CIGAR range" % i
        ops = cg[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]
        if np.any((ops & 15) > 2):
            return "record %d: CIGAR op" % i
        ln = (ops >> 4).astype(np.int64)
        tl, ql = int(ln[(ops & 15) != 1].sum()), int(ln[(ops & 15) != 2].sum())
        if tl != a["te"] - a["ts"] or ql != a["qe"] - a["qs"]:
            return "record %d: CIGAR lengths" % i
        if a["blen"] != int(ln.sum()) or not 0 <= a["mlen"] <= a["blen"]:
            return "record %d: mlen / blen" % i
        if not (a["flags"] & 7) in (F_PRIMARY, F_SECONDARY, F_SUPPL):
            return "record %d: kind" % i
    if any(not 1 <= len(n) <= 254 for n in c["qnames"]) or len(c["qnames"]) != len(c["reads"]):
        return "names"
    return None


def stream_of(c):
    return br.bam_stream(c["alns"], c["cigars"], c["reads"], c["targets"], c["qnames"], c["tnames"], c["flags"], c["rg"], "t")


# ---- reach predicates: f(stream, case) -> None | what was missed -----------------------------------------------------------
def need(pred, what):
    def f(s, c):
        return None if pred(s, c) else what
    return f


def all_of(*fs):
    def f(s, c):
        for g in fs:
            r = g(s, c)
            if r:
                return r
        return None
    return f


def mapped(s):
    return [r for r in s.recs if r["tid"] >= 0]


def both_strands(s, c):
    fl = set(bool(r["flag"] & 16) for r in mapped(s))
    return None if fl == {False, True} else "one strand only"


def md_numbers(md):
    return [int(x) for x in re.findall(r"\d+", md)]


def md_mismatch_cols(md):
    """reference columns (deletions count) of the substituted bases of an MD string"""
    out, p = [], 0
    for num, dele, sub in re.findall(r"(\d+)|(\^[A-Z]+)|([A-Z])", md):
        if num:
            p += int(num)
        elif dele:
            p += len(dele) - 1
        else:
            out.append(p); p += 1
    return out


def byte_runs(b):
    """lengths of the maximal runs of equal bytes"""
    out, i = [], 0
    while i < len(b):
        j = i
        while j < len(b) and b[j] == b[i]:
            j += 1
        out.append(j - i); i = j
    return out


def switch_candidates(s):
    """per BGZF block of the stream: the number of candidate table switches as k_bgzf_deflate's d_defl_segments counts them
    (a field start strictly inside the block whose field -- fixed part + name + CIGAR / SEQ + QUAL / tags -- has at least
    DEFL_MINSEG bytes), and the positions"""
    nblk = -(-len(s.raw) // BAM_BLK)
    cnt, pos = [0] * nblk, []
    for r in s.recs:
        for start, end in ((r["off"], r["p_seq"]), (r["p_seq"], r["p_tags"]), (r["p_tags"], r["off"] + r["size"])):
            if end - start >= DEFL_MINSEG and start % BAM_BLK:
                cnt[start // BAM_BLK] += 1; pos.append(start)
    return cnt, pos


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _alt_ops(n):
    """an edit script of exactly n CIGAR operations (n odd): M3 I1 M3 D1 M3 ... M3"""
    assert n % 2
    return [("=", 3) if i % 2 == 0 else (("I", 1) if i % 4 == 1 else ("D", 1)) for i in range(n)]


def walk_cases():
    rng = np.random.default_rng(11)
    T = [rseq(rng, 60000)]
    out = []
    for n in (1, 63, 64, 65, 127, 128, 129):
        b = Builder(T, seed=n)
        for rev in (False, True):
            # n operations, starting and ending with M (n odd) or ending with M after a leading insertion (n even)
            sc = _alt_ops(n) if n % 2 else [("I", 2)] + _alt_ops(n - 1)
            b.read().rec(0, 100 + 7 * n, sc, rev=rev)
        out.append(b.case("walk_ops_%d" % n, "walk", reach=all_of(both_strands, need(lambda s, c, n=n: all(r["n_ops"] == n for r in s.recs), "op count"))))
    # a match run over >= 3 trips of 64 operations, insertions in between: MD is ONE number; then the same with one mismatch in
    # the fourth trip, and with a deletion there
    b = Builder(T, seed=2)
    run = []
    for i in range(110):
        run += [("=", 5), ("I", 1 + i % 3)]
    for rev in (False, True):
        b.read().rec(0, 2000, run + [("=", 9)], rev=rev)
        b.read().rec(0, 3000, run + [("=", 4), ("X", 1), ("=", 4)], rev=rev)
        b.read().rec(0, 4000, run + [("=", 4), ("D", 2), ("=", 4)], rev=rev)
    out.append(b.case("walk_md_run_over_trips", "walk", reach=all_of(both_strands, need(
        lambda s, c: all(r["n_ops"] >= 193 for r in s.recs) and sorted(set(r["md"] for r in s.recs if r["md"].isdigit())) == ["559"]
        and any(re.fullmatch(r"554[ACGT]4", r["md"]) for r in s.recs) and any(re.fullmatch(r"554\^[ACGT]{2}4", r["md"]) for r in s.recs), "MD run across trips"))))
    # mismatches at the edges of an operation, of a 32-column word and of the record
    b = Builder(T, seed=3)
    cols = (0, 31, 32, 33, 63, 64, 99)
    for rev in (False, True):
        for col in cols:
            b.read().rec(0, 5000 + col, [("=", col), ("X", 1), ("=", 99 - col)], rev=rev)
        sc, p = [], 0
        for col in cols:
            sc += [("=", col - p), ("X", 1)]; p = col + 1
        b.read().rec(0, 6000, [x for x in sc if x[1]], rev=rev)
        # the last column of one operation and the first of the next (an insertion between them)
        b.read().rec(0, 6500, [("=", 30), ("X", 1), ("I", 2), ("X", 1), ("=", 30)], rev=rev)
    out.append(b.case("walk_mismatch_columns", "walk", reach=all_of(both_strands, need(
        lambda s, c: set(tuple(md_mismatch_cols(r["md"])) for r in s.recs) == set([(x,) for x in cols] + [cols, (30, 31)]), "mismatch columns"))))
    b = Builder(T, seed=4)
    for rev in (False, True):
        b.read().rec(0, 7000, [("=", 10), ("X", 3), ("=", 18), ("X", 2), ("=", 40)], rev=rev)          # 10,11,12 and 31,32
        b.read().rec(0, 7200, [("X", 2), ("=", 20), ("X", 2)], rev=rev)                                 # at both ends of the record
    out.append(b.case("walk_adjacent_mismatches", "walk", reach=all_of(both_strands, need(
        lambda s, c: all(re.search(r"[ACGT]0[ACGT]0[ACGT]", r["md"]) or (r["md"].startswith("0") and r["md"].endswith("0")) for r in s.recs)
        and all("*" in r["cs"] for r in s.recs), "0 separators"))))
    b = Builder(T, seed=5)
    for rev in (False, True):
        b.read().rec(0, 8000, [("=", 12), ("D", 2), ("X", 1), ("=", 12)], rev=rev)                     # ^AC0T: the mismatch opens the next M
        b.read().rec(0, 8100, [("=", 12), ("D", 2), ("=", 1), ("X", 1), ("=", 12)], rev=rev)           # ^AC1T
        b.read().rec(0, 8200, [("=", 12), ("X", 1), ("D", 3), ("=", 9)], rev=rev)                      # T0^ACG: mismatch, then the deletion
        b.read().rec(0, 8300, [("=", 12), ("D", 3), ("=", 7)], rev=rev)                                # the deletion is the last event
        b.read().rec(0, 8400, [("=", 12), ("D", 2), ("I", 3), ("=", 7)], rev=rev)                      # D and I adjacent
        b.read().rec(0, 8500, [("=", 12), ("I", 3), ("D", 2), ("=", 7)], rev=rev)
        b.read().rec(0, 8600, [("=", 5), ("I", 1), ("D", 1), ("I", 2), ("D", 2), ("=", 5)], rev=rev)
    out.append(b.case("walk_deletion_neighbours", "walk", reach=all_of(both_strands, need(
        lambda s, c: all(any(re.fullmatch(p, r["md"]) for r in s.recs) for p in (r"12\^[ACGT]{2}0[ACGT]12", r"12\^[ACGT]{2}1[ACGT]12", r"12[ACGT]0\^[ACGT]{3}9",
                                                                                   r"12\^[ACGT]{3}7", r"12\^[ACGT]{2}7", r"5\^[ACGT]0\^[ACGT]{2}5")), "MD around deletions"))))
    b = Builder(T, seed=6)
    for rev in (False, True):
        sc = []
        for i in range(40):
            sc += [("=", 1) if i % 3 else ("X", 1), ("I", 1) if i % 2 else ("D", 1)]
        b.read().rec(0, 9000, sc + [("=", 1)], rev=rev)
    out.append(b.case("walk_M_of_length_1", "walk", reach=all_of(both_strands, need(
        lambda s, c: all(int(x) >> 4 == 1 for x in c["cigars"] if int(x) & 15 == 0) and len(c["cigars"]) == 162, "M1 operations"))))
    # numbers at every power of ten, in MD and in cs
    nums = (9, 10, 99, 100, 999, 1000, 9999, 10000)
    b = Builder(T, seed=7)
    for rev in (False, True):
        for n in nums:
            b.read().rec(0, 10000, [("=", n), ("X", 1), ("=", n), ("D", 1), ("=", n), ("I", 1), ("=", n)], rev=rev)
    out.append(b.case("walk_numbers", "walk", reach=all_of(both_strands, need(
        lambda s, c: sorted(set(x for r in s.recs for x in md_numbers(r["md"]))) == sorted(set(nums) | set(2 * n for n in nums))
        and set(int(x) for r in s.recs for x in re.findall(r":(\d+)", r["cs"])) == set(nums), "numbers"))))
    # N in the read, in the target, in both at one column; inside a deletion and an insertion
    tn = list(rseq(rng, 3000))
    for p in (100, 101, 140, 205, 230, 231, 232, 300, 331, 332):
        tn[p] = "N"
    TN = ["".join(tn)]
    b = Builder(TN, seed=8)
    for rev in (False, True):
        b.read().rec(0, 80, [("=", 10), ("N", 1), ("=", 9), ("X", 1), ("=", 31)], rev=rev)          # N in the read at 90, in the target at 100 (read: a base) and 101 (read: N)
        b.read().rec(0, 200, [("=", 5), ("X", 1), ("=", 24), ("D", 6), ("=", 20), ("I", "ANNT"), ("=", 10)], rev=rev)          # target N at 205 (M) and at 230..232 inside the deletion
        b.read().rec(0, 300, [("=", 31), ("X", 2), ("=", 30)], rev=rev)          # target N in columns 0 (both N), 31 and 32 of one M
    out.append(b.case("walk_N_bases", "walk", reach=all_of(both_strands, need(
        lambda s, c: all(any(p in r["cs"] for r in s.recs) for p in ("*nn", "+annt")) and any(re.search(r"\*n[acgt]", r["cs"]) for r in s.recs)
        and any(re.search(r"\*[acgt]n", r["cs"]) for r in s.recs) and any(re.search(r"\^N", r["md"]) for r in s.recs)
        and any(r["md"].startswith("0N") for r in s.recs), "N columns"))))
    b = Builder(T, seed=9)
    for rev in (False, True):
        for n in (1, 31, 32, 33, 64, 65):
            b.read().rec(0, 20000 + 300 * n, [("=", 20), ("I", n), ("=", 20), ("D", n), ("=", 20)], rev=rev)
    out.append(b.case("walk_indel_lengths", "walk", reach=all_of(both_strands, need(
        lambda s, c: set(int(x) >> 4 for x in c["cigars"] if int(x) & 15) == {1, 31, 32, 33, 64, 65}, "indel lengths"))))
    b = Builder(T, seed=10)
    for rev in (False, True):
        for n in (1, 2, 31, 32, 33, 64, 65, 5000):
            b.read().rec(0, 30000 + n, [("=", n)], rev=rev)
    out.append(b.case("walk_perfect_match", "walk", reach=all_of(both_strands, need(lambda s, c: all(r["md"].isdigit() and r["nm"] == 0 for r in s.recs), "perfect"))))
    return out


def layout_cases():
    rng = np.random.default_rng(21)
    T = [rseq(rng, 50000), rseq(rng, 30000)]
    out = []
    sc = [("=", 30), ("X", 1), ("=", 10), ("I", 2), ("=", 20), ("D", 3), ("=", 25)]
    b = Builder(T, seed=1)
    for rev in (False, True):
        for left, right in ((7, 0), (0, 9), (5, 11), (0, 0)):
            b.read(left=left, right=right).rec(0, 1000 + 10 * left + right, sc, rev=rev)

    def clips(s, c):
        got = set()
        for r, p in zip(s.recs, br.parse_records(s.raw)):
            got.add((bool(r["flag"] & 16), p[7][0] & 15 == 4, p[7][-1] & 15 == 4))
        return None if len(got) == 8 else "clip / strand combinations: %d of 8" % len(got)
    out.append(b.case("layout_clips", "layout", reach=clips))
    # supplementary records: hard clips and a shortened SEQ without TELR_SAM_SOFTCLIP, soft clips with it; a secondary: no SEQ
    b = Builder(T, seed=2)
    for rev in (False, True):
        b.read(left=13, right=6).rec(0, 2000, sc, rev=rev).rec(1, 500, sc, rev=not rev, kind=F_SUPPL, gap=4).dup(kind=F_SECONDARY)
        b.read().rec(1, 900, sc, rev=rev).dup(kind=F_SECONDARY, mapq=0)

    def suppl(op):
        def f(s, c):
            ps = br.parse_records(s.raw)
            sup = [(r, p) for r, p in zip(s.recs, ps) if r["flag"] & 0x800]
            sec = [(r, p) for r, p in zip(s.recs, ps) if r["flag"] & 0x100]
            if not sup or any(p[7][0] & 15 != op or p[7][-1] & 15 != op for r, p in sup):
                return "clip operation of the supplementary records"
            if any((r["l_seq"] < len(c["reads"][r["qid"]])) != (op == 5) for r, p in sup):
                return "SEQ of the supplementary records"
            if len(sec) < 4 or any(r["l_seq"] or b"s2i" in p[10] or b"SAZ" in p[10] or b"tpAS" not in p[10] for r, p in sec):
                return "secondary records"
            return None
        return f
    base = b.case("layout_suppl_hard", "layout", flags=MD | CS, reach=suppl(5))
    out += [base, with_flags(base, "layout_suppl_soft", ALL, reach=suppl(4))]
    for i, fl in enumerate((0, MD, CS)):
        out.append(with_flags(base, "layout_tags_md%d_cs%d" % (fl & 1, fl >> 1 & 1), fl | SOFT, reach=need(
            lambda s, c, fl=fl: all((b"MDZ" in p[10]) == bool(fl & MD) and (b"csZ" in p[10]) == bool(fl & CS) for p in br.parse_records(s.raw)), "tags")))
    out.append(with_flags(base, "layout_rg", ALL, rg=("grp1", "smp", "lib9"), reach=need(lambda s, c: all(b"RGZgrp1\0" in p[10] for p in br.parse_records(s.raw)), "RG")))
    # l_seq x name length: the QUAL head / body / tail split depends on the address of QUAL modulo 4
    lens = list(range(1, 10)) + [31, 32, 33, 63, 64, 65, 2047, 2048, 2049]
    b = Builder(T, seed=3)
    k = 0
    for n in lens:
        for nl in range(1, 17):
            b.read(name="abcdefghijklmnop"[:nl]).rec(k % 2, 3000 + 3 * k, [("=", n)], rev=bool(k & 4))
            for _ in range(1 + k % 3):
                b.dup(kind=F_SECONDARY)      # l_seq n and, for the secondary, 0
            k += 1
    for nl in range(1, 5):
        for n in (0, 1, 2):
            b.unmapped(rseq(rng, n), name="zyxw"[:nl])

    def qual(s, c):
        seen = {}
        for r in s.recs:
            seen.setdefault(r["l_seq"], set()).add(r["p_qual"] & 3)
        miss = [n for n in [0] + lens if seen.get(n) != {0, 1, 2, 3}]
        return None if not miss else "QUAL alignments not all seen for l_seq %s" % miss
    out.append(b.case("layout_lseq_x_name", "layout", reach=qual))
    b = Builder(T, seed=4)
    b.read(name="n" * 254, left=3).rec(0, 4000, sc).read(name="m" * 253).rec(0, 4000, sc, rev=True)
    out.append(b.case("layout_name_254", "layout", reach=need(lambda s, c: max(r["l_name"] for r in s.recs) == 255, "l_read_name 255")))
    b = Builder(T, seed=5)
    b.unmapped("", "e0").read().rec(0, 100, sc).unmapped("G", "e1").unmapped("TN", "e2").read().rec(1, 100, sc, rev=True).unmapped("", "e3")
    um = need(lambda s, c: [r["l_seq"] for r in s.recs if r["flag"] == 4] == [0, 1, 2, 0], "unmapped reads of 0, 1, 2 bases")
    base = b.case("layout_unmapped", "layout", reach=um)
    out += [base, with_flags(base, "layout_unmapped_rg", ALL, rg=("g", "s", "l"), reach=um),
            with_flags(base, "layout_no_unmapped", ALL | NO_UNMAPPED, reach=need(lambda s, c: len(s.recs) == 2 and len(c["reads"]) == 6, "unmapped reads dropped"))]
    b = Builder(T, seed=6)
    b.unmapped("ACGTTGCA", "only")
    out.append(b.case("layout_zero_records", "layout", flags=ALL | NO_UNMAPPED, reach=need(lambda s, c: not s.recs and len(s.raw) == s.head_len, "no record")))
    b = Builder(T, seed=7)
    b.read().rec(0, 100, sc, dp_score=-77, mapq=0, subsc=-1, score=0, cnt=0).read().rec(0, 100, sc, mapq=255, dp_score=-2147483647).read().rec(0, 100, sc, mapq=60, rev=True)
    out.append(b.case("layout_fields", "layout", reach=need(lambda s, c: [p[4] for p in br.parse_records(s.raw)] == [0, 255, 60], "mapq 0 / 255 / 60")))
    # the <l_seq>S<ref_len>N placeholder: decided by the operations COUNTING the clips
    rngl = np.random.default_rng(22)
    TL = [rseq(rngl, 215000)]
    b = Builder(TL, seed=8)

    def ops_n(n):          # n operations, M2 I1 M2 D1 ..., first and last M
        return [("=", 2) if i % 2 == 0 else (("I", 1) if i % 4 == 1 else ("D", 1)) for i in range(n)]
    b.read(left=5).rec(0, 10, [("I", 1)] + ops_n(65533))                    # 65,535 with the clip: in the record
    b.read(left=5).rec(0, 20, ops_n(65535), rev=True)                                  # 65,536 with the clip: placeholder
    b.read(left=5, right=3).rec(0, 30, [("I", 1)] + ops_n(65533))           # 65,534 + 2 clips: placeholder
    b.read().rec(0, 40, ops_n(65535))                                                  # 65,535 without clips: in the record
    b.read().rec(0, 50, ops_n(65535) + [("I", 1)], rev=True)                           # 65,536 without clips: placeholder

    def longcig(s, c):
        got = [(r["n_ops"], r["n_cig"]) for r in s.recs]
        want = [(65535, 65535), (65536, 2), (65536, 2), (65535, 65535), (65536, 2)]
        return None if got == want and [int(a["n_cigar"]) for a in c["alns"]] == [65534, 65535, 65534, 65535, 65536] else "operation counts %s" % got
    out.append(b.case("layout_long_cigar", "layout", reach=longcig))
    return out


def bin_level(b):
    return 14 if b >= 4681 else 17 if b >= 585 else 20 if b >= 73 else 23 if b >= 9 else 26 if b >= 1 else 29


def sort_cases(big=True):
    rng = np.random.default_rng(31)
    T = [rseq(rng, 40000), rseq(rng, 20000), rseq(rng, 30000)]
    out = []
    sc = [("=", 40), ("X", 1), ("=", 40)]
    b = Builder(T, seed=1)
    for i in range(4):
        b.read().rec(1, 5000, sc, rev=True)
        b.read().rec(1, 5000, sc)
    b.read().rec(1, 5000, [("I", 4)])                      # te == ts: no reference base
    b.read().rec(2, 29919, sc).read().rec(0, 0, sc, rev=True).read().rec(2, 0, sc).read().rec(0, 39919, sc)
    b.unmapped("ACGT", "u").read().rec(1, 4999, sc, rev=True).read().rec(1, 5001, sc)

    def order(s, c):
        m = mapped(s)
        at = [r for r in m if r["tid"] == 1 and r["pos"] == 5000]
        want = [1, 3, 5, 7, 8, 0, 2, 4, 6]                 # forward records in input order (the I-only one among them), then the reverse ones
        if [r["idx"] for r in at] != want:
            return "order at one position: %s" % [r["idx"] for r in at]
        if m[0]["tid"] != 0 or m[0]["pos"] != 0 or m[-1]["tid"] != 2 or s.recs[-1]["flag"] != 4:
            return "first / last target"
        if not any(r["pos"] == r["end"] for r in m):
            return "te == ts"
        return None
    out.append(b.case("sort_equal_keys_and_strands", "sort", reach=order))
    if big:
        L = (1 << 23) + 6000
        TB = [rseq(rng, 3000), rseq(np.random.default_rng(32), L)]
        b = Builder(TB, seed=2)
        k = 0
        for sh, mult in ((14, 3), (17, 3), (20, 3), (23, 1)):
            bd = mult << sh
            for ts, n in ((bd - 100, 100), (bd - 100, 101), (bd - 50, 100), (bd, 100), (bd - 1, 1), (bd - 1, 2), (bd + 200, 100)):
                b.read().rec(1, ts, [("=", n - 1), ("X", 1)] if n > 1 else [("=", 1)], rev=bool(k & 1)); k += 1
        b.read().rec(0, 10, [("=", 50)])

        def bins(s, c):
            lv = {}
            for r in mapped(s):
                lv.setdefault(bin_level(r["bin"]), []).append(r)
            if sorted(lv) != [14, 17, 20, 23, 26]:
                return "bin levels %s" % sorted(lv)
            for sh, mult in ((14, 3), (17, 3), (20, 3), (23, 1)):
                bd = mult << sh
                if not (any(r["end"] == bd and bin_level(r["bin"]) == 14 for r in mapped(s)) and any(r["end"] == bd + 1 and bin_level(r["bin"]) > sh - 1 and r["pos"] < bd for r in mapped(s))):
                    return "records ending on / one past %d << %d" % (mult, sh)
            return None
        out.append(b.case("sort_bins_8mb_target", "sort", reach=bins))
        L = (1 << 26) + 5000
        TH = [rseq(np.random.default_rng(33), L)]
        b = Builder(TH, seed=3)
        bd = 1 << 26
        for k, (ts, n) in enumerate(((bd - 100, 100), (bd - 100, 101), (bd - 50, 100), (bd, 100), ((1 << 23) - 20, 40), (100, 100), (bd + 4800, 200))):
            b.read().rec(0, ts, [("=", n - 1), ("X", 1)], rev=bool(k & 1))
        out.append(b.case("sort_bins_64mb_target", "sort", reach=need(
            lambda s, c: sorted(set(bin_level(r["bin"]) for r in s.recs)) == [14, 26, 29] and sum(r["bin"] == 0 for r in s.recs) == 2, "bin 0 and level 26")))
    return out


def sa_cases():
    rng = np.random.default_rng(41)
    T = [rseq(rng, 30000), rseq(rng, 30000), rseq(rng, 30000)]
    tn = ["chrA", "b", "a_rather_long_target_name.3"]
    plain = [("=", 60)]
    indel = [("=", 30), ("I", 3), ("=", 30), ("D", 12), ("=", 20), ("X", 2), ("=", 9)]
    ins = [("=", 30), ("I", 11), ("=", 30)]
    dele = [("=", 30), ("D", 100), ("=", 30)]
    b = Builder(T, tn, seed=1)
    # the first read of the array: five non-secondary records with secondaries between them
    b.read(left=8, right=0).rec(0, 100, indel).dup().rec(1, 200, plain, rev=True, kind=F_SUPPL).rec(2, 999, ins, kind=F_SUPPL, gap=10).dup() \
        .rec(0, 9999, dele, rev=True, kind=F_SUPPL).rec(2, 29000, plain, kind=F_SUPPL, mapq=0)
    b.read().rec(1, 1000, plain)                                                        # one record: no SA
    b.read().rec(1, 7000, plain, rev=True).dup(kind=F_SUPPL)          # two records over the whole read: SA entries without clips
    b.read().rec(1, 9000, dele).dup(kind=F_SUPPL)
    b.read().rec(1, 1000, plain).dup()                                                  # one + a secondary: no SA
    b.unmapped("ACGTA", "u")
    b.read(right=4).rec(0, 20000, plain, rev=True).rec(0, 20100, indel, rev=True, kind=F_SUPPL)          # two
    b.read().rec(2, 5, ins, rev=True).dup().dup().rec(1, 99, dele, kind=F_SUPPL, mapq=3).dup()
    # the last read of the array: three
    b.read(left=0, right=21).rec(1, 15000, dele).rec(0, 15000, indel, rev=True, kind=F_SUPPL, mapq=17).rec(2, 15000, plain, kind=F_SUPPL)

    def sa(s, c):
        per_read = {}
        for a in c["alns"]:
            if not a["flags"] & F_SECONDARY:
                per_read[int(a["qid"])] = per_read.get(int(a["qid"]), 0) + 1
        if sorted(set(per_read.values())) != [1, 2, 3, 5]:
            return "records per read %s" % sorted(set(per_read.values()))
        for r in s.recs:
            if r["tid"] < 0:
                continue
            want = 0 if r["flag"] & 0x100 else per_read[r["qid"]] - 1
            if r["sa"].count(";") != want:
                return "SA entries of record %d" % r["idx"]
        if per_read[int(c["alns"]["qid"][0])] != 5 or per_read[int(c["alns"]["qid"][-1])] != 3:
            return "first / last read"
        txt = "".join(r["sa"] for r in s.recs)
        for p in (r",\+,\d+S\d+M\d+I\d+D\d+S,", r",-,\d+M,", r",\d+M\d+D,", r",\d+S\d+M\d+I,", r",[+-],\d+M[0-9ID]*S,", r"a_rather_long_target_name\.3,6,-,", r",0,0;", r",17,17;"):
            if not re.search(p, txt):
                return "no SA entry like %s" % p
        return None
    base = b.case("sa_groups", "sa", reach=sa)
    return [base, with_flags(base, "sa_groups_hard_clips", MD | CS)]


def _tune(make, measure, want, lo=1, hi=100000):
    """the parameter n in [lo, hi] (and name length 1..6) for which measure(make(n, name length)) == want; measure is non-decreasing in n"""
    for nl in range(1, 7):
        a, z = lo, hi
        while a <= z:
            mid = (a + z) // 2
            v = measure(make(mid, nl))
            if v == want:
                return make(mid, nl)
            if v < want:
                a = mid + 1
            else:
                z = mid - 1
    raise ValueError("no filler reaches %d" % want)


def framing_cases():
    rng = np.random.default_rng(51)
    T = [rseq(rng, 140000), rseq(rng, 5000)]
    sc = [("=", 40), ("X", 1), ("=", 30), ("I", 2), ("=", 20)]
    out = []

    def tail_filler(n, nl):          # two small records, then an unmapped filler read of n bases at the end of the stream
        b = Builder(T, seed=1)
        b.read().rec(0, 10, sc).read().rec(1, 10, sc, rev=True).unmapped(rseq(np.random.default_rng(n), n), "f" * nl)
        return b
    for k in (1, 2):
        for d in (-1, 0, 1):
            want = k * BAM_BLK + d
            b = _tune(tail_filler, lambda b: len(stream_of(b.case("", "")).raw), want)
            out.append(b.case("framing_total_%dblk%+d" % (k, d), "framing", reach=need(lambda s, c, want=want: len(s.raw) == want, "stream length")))
    for d in (1, 2, 3, 5, 39):
        want = BAM_BLK + d
        b = _tune(tail_filler, lambda b: len(stream_of(b.case("", "")).raw), want)
        out.append(b.case("framing_last_block_%d" % d, "framing", stored_last=True, reach=need(lambda s, c, want=want: len(s.raw) == want, "stream length")))

    def head_filler(n, nl):          # a mapped filler read first (perfect match of n bases at 0), then the record whose start is aimed at
        b = Builder(T, seed=2)
        b.read(name="g" * nl).rec(0, 0, [("=", n)]).read(name="x" * 40).rec(0, 70000, sc, rev=True).read().rec(1, 5, sc)
        return b
    # the second record starts exactly on a block start / so that the boundary falls inside its block_size, behind l_read_name,
    # inside n_cigar_op, inside l_seq
    for d, what in ((0, "on_block_start"), (2, "in_block_size"), (13, "after_l_read_name"), (17, "in_n_cigar_op"), (22, "in_l_seq"), (35, "in_fixed_part_end")):
        want = BAM_BLK - d
        b = _tune(head_filler, lambda b: stream_of(b.case("", "")).offsets[1], want, hi=65000)
        out.append(b.case("framing_record_%s" % what, "framing", reach=need(lambda s, c, want=want: s.offsets[1] == want and len(s.recs) == 3, "record offset")))
    # a header of several blocks: whole blocks inside the header (no first record), with and without records behind it
    nt = 2600
    TS = [rseq(rng, 300) for _ in range(nt)]
    names = ["contig_%05d_of_a_fragmented_assembly_with_long_names" % i for i in range(nt)]
    b = Builder(TS, names, seed=3)
    b.read().rec(0, 3, [("=", 100)]).read().rec(nt - 1, 150, [("=", 100), ("X", 1), ("=", 49)], rev=True).unmapped("ACGTN", "u")
    big_head = need(lambda s, c: s.head_len > 3 * BAM_BLK, "header of more than three blocks")
    base = b.case("framing_long_header", "framing", reach=all_of(big_head, need(lambda s, c: len(s.recs) == 3, "records")))
    b = Builder(TS, names, seed=4)
    b.unmapped("ACGT", "u")
    out += [base, b.case("framing_long_header_no_records", "framing", flags=ALL | NO_UNMAPPED, reach=all_of(big_head, need(lambda s, c: not s.recs, "no records")))]
    return out


def deflate_cases():
    rng = np.random.default_rng(61)
    T = [rseq(rng, 90000)]
    out = []
    two = [("X", 50), ("=", 78)]          # 128 bases: SEQ + QUAL = 192 bytes; cs of 153 characters: tags of 196 bytes with cs only
    one = [("=", 128)]                    # SEQ + QUAL = 192 bytes, short tags

    def dense(n2, n1, n0=0):
        b = Builder(T, seed=n2)
        for i in range(n2):
            b.read(name="r%02x" % (i % 256)).rec(0, 100 + 130 * i, two, rev=bool(i & 1))
        for i in range(n1):
            b.read(name="s%02x" % i).rec(0, 80000 + 130 * i, one)
        for i in range(n0):
            b.read(name="t%02x" % i).rec(0, 85000 + 10 * i, [("=", 60)])
        return b
    b = dense(400, 0)
    out.append(b.case("deflate_300_switches", "deflate", flags=CS | SOFT, reach=need(lambda s, c: max(switch_candidates(s)[0]) >= 300, "300 candidate switches in a block")))
    for want in (254, 255, 256, 257):
        b = dense(want // 2, want % 2, 5)
        out.append(b.case("deflate_%d_switches" % want, "deflate", flags=CS | SOFT, reach=need(
            lambda s, c, want=want: switch_candidates(s)[0] == [want], "exactly %d candidate switches in the block" % want)))
    # fields of 191 and 192 bytes, each of the three kinds
    b = Builder(T, seed=2)
    for i, (nl, n, rgl) in enumerate(((150, 127, 0), (151, 128, 1), (150, 128, 1), (151, 127, 0))):
        for j in range(3):
            b.read(name="n" * nl).rec(0, 1000 * i + 100 * j, [("X", 44), ("=", 9 + j % 2), ("X", 1), ("=", n - 54 - j % 2)], rev=bool(j & 1))
    base = b.case("deflate_fields_191_192", "deflate", flags=CS | SOFT, rg=None)

    def fields(s, c):
        a = set(r["p_seq"] - r["off"] for r in s.recs); bq = set(r["p_tags"] - r["p_seq"] for r in s.recs); t = set(r["l_tags"] for r in s.recs)
        return None if a == {191, 192} and bq == {191, 192} and t >= {191, 192} else "field lengths %s %s %s" % (sorted(a), sorted(bq), sorted(t))
    # tags: 43 bytes of fixed tags + cs; the RG tag (4 + its length) trims them to 191 and 192
    for rgl in range(1, 30):
        c = with_flags(base, "deflate_fields_191_192", CS | SOFT, rg=("g" * rgl, "s", "l"), reach=fields)
        if fields(stream_of(c), c) is None:
            break
    out.append(c)
    # runs of equal bytes in SEQ (homopolymers: 2 r bases = r bytes; N runs) and in QUAL (l_seq), starting anywhere in a 64-byte piece
    runs = (2, 3, 4, 63, 64, 65, 66, 200)
    parts, pos, p = [], [], 0
    for k, r in enumerate(runs * 2):
        base_ = "ACGTN"[k % 5] if k < 8 else "N"
        o1, o2 = ("C", "G") if base_ in "AN" else ("A", "T")
        # an even number of bases before the run, so that it fills whole bytes; its neighbours differ from it
        parts.append(rseq(rng, 9 + 2 * (k % 4)) + o1 + base_ * (2 * r) + o2 + rseq(rng, 6))
        pos.append((p, len(parts[-1]))); p += len(parts[-1])
    TR = ["".join(parts) + rseq(rng, 4000)]
    b = Builder(TR, seed=3)
    for k, (p0, n) in enumerate(pos):
        b.read(name="h%d" % k).rec(0, p0, [("=", n)])
    q = 0
    for n in runs:
        for nl in range(1, 41):
            b.read(name=("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMN" * 2)[:1 + (nl * nl) % 41]).rec(0, p + 5 * q, [("=", n)], rev=bool(q & 1)); q += 1

    def runs_reach(s, c):
        seq_runs, qual_at = set(), set()
        for r in s.recs:
            seq_runs |= set(byte_runs(s.raw[r["p_seq"]:r["p_qual"]]))
            if r["l_seq"] in runs:
                qual_at.add(r["p_qual"] % DEFL_PIECE)
        if not seq_runs >= set(runs):
            return "SEQ runs %s" % sorted(set(runs) - seq_runs)
        if set(r["l_seq"] for r in s.recs) < set(runs) or len(qual_at) != DEFL_PIECE:
            return "QUAL runs start at %d of 64 piece offsets" % len(qual_at)
        return None
    out.append(b.case("deflate_runs", "deflate", reach=runs_reach))
    # a run cut by a table switch: the last tag of a record (s2:i) ends in the byte the next record's block_size begins with,
    # and that record's first field is long enough to switch the table
    def cut(sub):
        b = Builder(T, seed=4)
        for i in range(6):
            b.read(name="k%d" % i).rec(0, 100 + i, [("=", 128)], subsc=sub)
            b.read(name="w" * 170).rec(0, 100 + i, [("=", 128)], rev=True, subsc=sub)
        return b.case("deflate_run_cut_by_switch", "deflate", flags=SOFT)
    c0 = cut(0)
    s0 = stream_of(c0)
    lowbyte = (s0.recs[1]["size"] - 4) & 255
    c = cut(int(np.array(lowbyte * 0x01010101, np.uint32).astype(np.int32)))

    def cut_reach(s, c):
        cand = [p for p in switch_candidates(s)[1] if s.raw[p - 3:p] == s.raw[p:p + 1] * 3]
        return None if len(cand) >= 5 else "runs crossing a table switch: %d" % len(cand)
    c["reach"] = cut_reach
    out.append(c)
    return out


def cases(big=True):
    return walk_cases() + layout_cases() + sort_cases(big) + sa_cases() + framing_cases() + deflate_cases()


# ---- every case through the writers (needs the engine; tests/test_gpu_bam_edges.py and `--engine`) -------------------------
def first_difference(got, s):
    """where two streams part, in terms of the reference's records"""
    k = next((i for i in range(min(len(got), len(s.raw))) if got[i] != s.raw[i]), min(len(got), len(s.raw)))
    where = "in the header" if k < s.head_len else "past the last record"
    for r in s.recs:
        if r["off"] <= k < r["off"] + r["size"]:
            f = "fixed part" if k < r["off"] + 36 else "name" if k < r["p_cig"] else "CIGAR" if k < r["p_seq"] else "SEQ" if k < r["p_qual"] else "QUAL" if k < r["p_tags"] else "tags"
            where = "record %s (input %s, %d:%d) %s, byte %d of %d" % (s.recs.index(r), r["idx"], r["tid"], r["pos"], f, k - r["off"], r["size"])
    return "lengths %d / %d, first difference at %d: %s: %r / %r" % (len(got), len(s.raw), k, where, got[max(0, k - 12):k + 12], s.raw[max(0, k - 12):k + 12])


def slice_masks(s, n):
    """emit masks over the input records for pretended ranks: [(label, [mask per rank], sorted)].  `sorted`: the ranks hold
    consecutive ranges of the coordinate order, as the N-rank writer is specified; the alternating split is not such a
    partition -- its file holds every rank's records in coordinate order, one rank after the other, and has no index."""
    order = [r["idx"] for r in s.recs if r["idx"] is not None]

    def mask(idx):
        m = np.zeros(n, np.uint8); m[list(idx)] = 1
        return m
    h, t1, t2 = len(order) // 2, len(order) // 3, 2 * len(order) // 3
    return [("halves", [mask(order[:h]), mask(order[h:])], True),
            ("thirds_middle_empty", [mask(order[:t1 + (t2 - t1)]), mask([]), mask(order[t2:])], True),
            ("first_rank_empty", [mask([]), mask(order)], True),
            ("alternating", [mask(range(0, n, 2)), mask(range(1, n, 2))], False)]


def run_case(engine, c, tmp, say=None):
    """-> list of differences (empty: every writer's file equals the reference stream and index)"""
    import ctypes as C
    from telr_amd.fasta import concat
    from telr_amd.presets import preset
    bad = []
    s = stream_of(c)
    tl = [len(t) for t in c["targets"]]
    want_index = br.bai_reference(s, tl)
    fl = c["flags"]
    kw = dict(md=bool(fl & MD), cs=bool(fl & CS), softclip=bool(fl & SOFT), rg=c["rg"], cmdline="t")
    un = not fl & NO_UNMAPPED
    ix = engine.index(c["targets"], preset("map-ont")[0])
    qset = engine.seqset(c["reads"])
    r = ix.result_from_arrays(c["alns"], c["cigars"])

    def check(tag, path, index=True, want=None):
        try:
            got, blocks = br.read_bgzf(path)
            if got != (s.raw if want is None else want):
                bad.append("%s %s: %s" % (c["name"], tag, first_difference(got, s) if want is None else "differs from the ranks' records in their order"))
                return None
            if index:
                br.compare_bai(open(path + ".bai", "rb").read(), blocks, want_index)
            return blocks
        except (AssertionError, KeyError, ValueError, IndexError, OSError, zlib.error) as e:
            bad.append("%s %s: %s: %s" % (c["name"], tag, type(e).__name__, str(e)[:300]))
            return None
    from telr_amd._lib import TelrError

    def attempt(what, f):          # a writer's error return is a difference of its own; the other writers still run
        try:
            f()
        except TelrError as e:
            bad.append("%s %s: %s" % (c["name"], what, str(e)[:300]))

    def device():
        for level in (0, 1):
            p = os.path.join(tmp, "dev%d.bam" % level)
            ix.write_bam_device(r, qset, c["qnames"], c["tnames"], p, index=True, level=level, unmapped=un, **kw)
            blocks = check("device level %d" % level, p)
            if blocks and c["stored_last"] and level == 1 and blocks[-2][3] != 0:
                bad.append("%s: the short last block is not a stored block (BTYPE %d)" % (c["name"], blocks[-2][3]))
            if blocks and level == 0 and any(b[3] != 0 for b in blocks[:-1]):
                bad.append("%s: level 0 wrote a block that is not stored" % c["name"])

    def host():          # (the wrapper has no switch for TELR_SAM_NO_UNMAPPED: the C entry is called as it calls it)
        p = os.path.join(tmp, "host.bam")
        qb, qo, ql = concat(c["reads"]); tb, to, tlen = concat(c["targets"])
        qb = np.ascontiguousarray(qb, np.uint8); tb = np.ascontiguousarray(tb, np.uint8)
        rg = (None, None, None) if c["rg"] is None else tuple(x.encode() for x in c["rg"])
        engine._chk(engine.L.telr_write_bam(r, len(ql), ix._cstr_array(c["qnames"]), qb.ctypes.data, qo.ctypes.data, ql.ctypes.data, len(tlen), ix._cstr_array(c["tnames"]),
                                            tb.ctypes.data, to.ctypes.data, tlen.ctypes.data, fl, rg[0], rg[1], rg[2], b"t", p.encode(), 1, 1), "telr_write_bam")
        check("host", p)

    def ranks(label, masks, in_order, level=1):          # (telr_write_bam_slice codes deflate blocks only: level 0 is an argument error)
        p = os.path.join(tmp, "slice_%s_%d.bam" % (label, level))
        open(p, "wb").close()
        off, ent, n_un, v_end = 0, [], 0, 0
        for k, m in enumerate(masks):
            last = k == len(masks) - 1
            seg = ix.write_bam_slice(r, qset, c["qnames"], c["tnames"], m, with_header=k == 0, level=level, unmapped=un and last, **kw)
            try:
                info = ix.segment_info(seg)
                if info["mapped_records"] != int(m.sum()):
                    bad.append("%s slice %s rank %d: %d records for %d marked" % (c["name"], label, k, info["mapped_records"], int(m.sum())))
                ix.segment_write(seg, p, off, last)
                e = ix.segment_entries(seg, off)
                ent.append(e[:4]); v_end = e[4]; n_un += info["unmapped_reads"]; off += info["bytes"]
            finally:
                ix.segment_free(seg)
        if in_order:
            ix.bai_write(p + ".bai", *[np.concatenate([e[i] for e in ent]) for i in range(4)], v_end, n_un, tl)
            check("slices %s" % label, p)
        else:
            parts = [s.raw[:s.head_len]]
            for m in masks:
                parts += [s.raw[x["off"]:x["off"] + x["size"]] for x in s.recs if x["idx"] is not None and m[x["idx"]]]
            parts += [s.raw[x["off"]:x["off"] + x["size"]] for x in s.recs if x["idx"] is None]
            check("slices %s" % label, p, index=False, want=b"".join(parts))
    try:
        attempt("device", device)
        attempt("host", host)
        for label, masks, in_order in slice_masks(s, len(c["alns"])):
            attempt("slices " + label, lambda: ranks(label, masks, in_order))
    finally:
        ix.free_raw(r)
        qset.free(); ix.free()
    if say:
        say("%-34s %s" % (c["name"], "ok" if not bad else "DIFFERS"))
    return bad


def run_all(engine, cs, tmp, say=None):
    bad = []
    for c in cs:
        err = check_case(c)
        assert err is None, (c["name"], err)          # a malformed record never reaches a kernel
        bad += run_case(engine, c, tmp, say)
    return bad


if __name__ == "__main__" and "--engine" in sys.argv:
    import tempfile
    import torch  # noqa: F401  (first: the process binds to its HIP runtime)
    from telr_amd.aligner import Engine
    eng = Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        bad = run_all(eng, cases(), tmp, print)
    print("\n".join(bad[:60]))
    print("bam edges ok" if not bad else "bam edges: %d differences" % len(bad))
    sys.exit(1 if bad else 0)

if __name__ == "__main__":
    bad = 0
    for c in cases():
        err = check_case(c)
        s = stream_of(c)
        miss = err or (c["reach"](s, c) if c["reach"] else None)
        bad += bool(miss)
        print("%-34s %-8s %6d records %9d bytes  %s" % (c["name"], c["group"], len(s.recs), len(s.raw), "reached" if not miss else "MISSED: " + miss))
    print("%s" % ("all cases reach their edge" if not bad else "%d cases miss" % bad))
    sys.exit(1 if bad else 0)
