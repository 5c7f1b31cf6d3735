"""Hand-built records aimed at the caps and branch points of the two consensus kernels (k_poa_window, poa.hip.h; k_pile_count /
k_pile_call, pileup.hip.h), without the mapper: one record per piece, covering its window exactly (ts = w0, te = w1), on either
strand, with a valid CIGAR (M, I / D runs of at most 30).  The host cut then hands the kernel exactly the aligned bases.

Every case is a dict: name, targets, reads, alns (ALN_DTYPE), cigars, `poa` / `pile` (which consensus it is aimed at), `md`
(the min_depth values it is run at: 1, 3 and its own boundary) and `reach`: a function of the oracle's per-window statistics
(tor_poa_stats, oracle/binding.py POA_STATS) and of the case, returning None when the case reached its edge, else what it
missed.  tests/test_consensus_reference.py checks the oracle against plain references on these cases, and
tests/test_gpu_consensus_edges.py the kernels against the oracle.

usage: python tests/consensus_edges.py   (prints every case with what it reached)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

from telr_amd._abi import ALN_DTYPE

W = 200                  # POA_W
SEGMAX = 400             # POA_SEGMAX
MAXSEG = 64              # POA_MAXSEG
MAXNODE = 2048           # POA_MAXNODE
MAXIN = 8                # POA_MAXIN
RING = 16                # POA_RING
KMAX = 8                 # CONS_KMAX
MAXDEL = 30              # CONS_MAXDEL
M, I, D = (lambda n: n << 4), (lambda n: n << 4 | 1), (lambda n: n << 4 | 2)

_COMP = {ord(a): b for a, b in zip("ACGTNacgtn", "TGCANtgcan")}


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rseq(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def other(b, k=1):
    """a base different from b (the k-th one after it)"""
    i = "ACGT".find(b.upper())
    return "ACGT"[(max(i, 0) + k) % 4]


def merge_ops(ops):
    out = []
    for op, n in ops:
        if n <= 0:
            continue
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return out


def edit(seg, subs=None, ins=None, dels=None):
    """the draft segment with substitutions {col: base}, insertions {col: bases, inserted before col (col = len: after the
    last)} and deletions {col: length}; -> (piece, CIGAR words).  The caller keeps every I / D run at most 30."""
    subs, ins, dels = subs or {}, ins or {}, dels or {}
    out, ops, p = [], [], 0
    while p <= len(seg):
        if p in ins:
            out.append(ins[p]); ops.append((1, len(ins[p])))
        if p == len(seg):
            break
        if p in dels:
            ops.append((2, dels[p])); p += dels[p]
            continue
        out.append(subs.get(p, seg[p])); ops.append((0, 1)); p += 1
    return "".join(out), [n << 4 | op for op, n in merge_ops(ops)]


def stretch_cigar(L, m):
    """a valid CIGAR of m query bases over L target bases: M with the difference spread as I / D runs of at most 30, starting
    and ending with M when there is room"""
    k, op = abs(m - L), 1 if m > L else 2
    nrun = -(-k // 30)
    span = L if op == 1 else L - k
    if nrun and span < nrun + 1:
        raise ValueError("no room for %d runs in %d columns" % (nrun, span))
    ops, done = [], 0
    for r in range(nrun):
        at = (r + 1) * span // (nrun + 1)
        ops.append((0, at - done)); done = at
        ops.append((op, min(30, k - 30 * r)))
    ops.append((0, span - done))
    return [n << 4 | o for o, n in merge_ops(ops)]


class Builder:
    """records over targets; read i = the aligned bases (on the alignment strand) with optional flanks"""

    def __init__(self, targets):
        self.targets = list(targets)
        self.reads, self.recs = [], []

    def rec(self, tid, ts, aligned, cig, rev=False, left="", right="", flags=1):
        full = left + aligned + right
        q = revcomp(full) if rev else full
        qs = len(right) if rev else len(left)
        a = np.zeros(1, ALN_DTYPE)
        a["qid"] = len(self.reads); a["tid"] = tid; a["qlen"] = len(q); a["qs"] = qs; a["qe"] = qs + len(aligned)
        a["ts"] = ts; a["te"] = ts + sum(c >> 4 for c in cig if (c & 15) in (0, 2)); a["flags"] = flags | (8 if rev else 0)
        a["n_cigar"] = len(cig); a["mapq"] = 60
        assert sum(c >> 4 for c in cig if (c & 15) in (0, 1)) == len(aligned)
        assert int(a["te"][0]) <= len(self.targets[tid]), (ts, cig)
        self.reads.append(q); self.recs.append((a, list(cig)))
        return self

    def case(self, name, poa=True, pile=True, md=(1, 3), reach=None, note=""):
        alns, cigs = [], []
        for a, c in self.recs:
            a = a.copy(); a["cigar_off"] = len(cigs); cigs += c; alns.append(a)
        alns = np.concatenate(alns) if alns else np.zeros(0, ALN_DTYPE)
        return dict(name=name, targets=self.targets, reads=self.reads, alns=alns, cigars=np.array(cigs, np.uint32),
                    poa=poa, pile=pile, md=tuple(sorted(set((1, 3) + tuple(md)))), reach=reach, note=note)


def windows(tlens):
    """(tid, w0, w1) of every window, in the order of tor_poa_stats"""
    return [(t, w0, min(w0 + W, L)) for t, L in enumerate(tlens) for w0 in range(0, L, W)]


# ---- reach predicates on the oracle's window statistics --------------------------------------------------------------------
def need(pred, what):
    def f(ws, case):
        return None if pred(ws, case) else what
    return f


def all_of(*fs):
    def f(ws, case):
        for g in fs:
            r = g(ws, case)
            if r:
                return r
        return None
    return f


def any_w(key, test):
    return lambda ws, c: any(test(w[key]) for w in ws if w["ran"])


# ---- POA cases ---------------------------------------------------------------------------------------------------------------
def _plain_reads(rng, b, tid, w0, w1, count, strands=(False, True), subs_every=0):
    seg = b.targets[tid][w0:w1].upper().replace("N", "A")
    for i in range(count):
        subs = {}
        if subs_every:
            c = int(rng.integers(0, w1 - w0)); subs[c] = other(seg[c], 1 + i % 3)
        p, cg = edit(seg, subs=subs)
        b.rec(tid, w0, p, cg, rev=strands[i % len(strands)])


def poa_cases(rng):
    cases = []
    # several targets, last windows of 1, 2, 63, 64, 65, 127, 128, 129 and 199 bases (sweep batches of 64 ranks: n = 64k - 1,
    # 64k, 64k + 1 before the first piece), a few substitutions on both strands
    lasts = (1, 2, 63, 64, 65, 127, 128, 129, 199)
    tg = [rseq(rng, W + r) for r in lasts]
    b = Builder(tg)
    for t, L in enumerate(len(x) for x in tg):
        for (tid, w0, w1) in windows([L]):
            _plain_reads(rng, b, t, w0, w1, 4, subs_every=1)
    cases.append(b.case("last_windows", reach=need(lambda ws, c: sorted({w["L"] for w in ws if w["ran"]}) == sorted({W} | set(lasts)),
                                                   "a last window did not run")))
    # lower-case and N draft bases; a read with an N (does not vote)
    t = rseq(rng, 400)
    t = t[:30] + t[30:90].lower() + "NN" + t[92:250] + "N" + t[251:]
    b = Builder([t])
    for (tid, w0, w1) in windows([len(t)]):
        seg = t[w0:w1].upper().replace("N", "C")
        for i in range(5):
            p, cg = edit(seg, subs={7 + i: other(seg[7 + i])})
            if i == 4:
                p = p[:50] + "N" + p[51:]
            b.rec(0, w0, p, cg, rev=bool(i & 1))
    cases.append(b.case("lower_and_n_draft", md=(4, 5), reach=need(lambda ws, c: all(w["voting"] == 4 and w["offered"] == 5 for w in ws),
                                                                  "N piece not offered / left out")))
    # band clamp: pieces with m < 63, m = 63 / 64 / 65 (hi = m + 1 - 64 at 0, 1, 2), zero-length pieces in a 1-base window
    for L, ms in ((120, (60, 62, 63, 64, 65)), (W, (100, 101, 127, 128, 129)), (65, (33, 40, 62, 63, 64))):
        t = rseq(rng, L)
        b = Builder([t])
        for k, m in enumerate(ms):
            for s in range(3):
                p = (t * 3)[:m] if m <= L else t + rseq(rng, m - L)
                if m < L:
                    p, cg = edit(t, dels={(L // 2) - (L - m) // 2 + (s % 2): L - m} if L - m <= 30 else None)
                    if L - m > 30:
                        p = rseq(rng, m); cg = stretch_cigar(L, m)
                else:
                    cg = stretch_cigar(L, m)
                b.rec(0, 0, p, cg, rev=bool(s & 1))
        cases.append(b.case("band_clamp_L%d" % L, reach=need(lambda ws, c, ms=ms: ws[0]["seg_min"] == min(ms) and ws[0]["seg_max"] == max(ms),
                                                             "the piece lengths did not vote")))
    # zero-length pieces: a 1-base last window deleted by every record (multi-window records, both strands)
    t = rseq(rng, W + 1)
    b = Builder([t])
    for s in range(4):
        b.rec(0, 0, t[:W], [M(W), D(1)], rev=bool(s & 1))
    cases.append(b.case("zero_length_pieces", md=(4, 5), reach=need(lambda ws, c: ws[1]["ran"] and ws[1]["seg_max"] == 0 and ws[1]["voting"] == 4,
                                                                    "no zero-length piece voted")))
    # pieces from W / 2 to 400 bases: dl = 0, 1 and 2 (rows of kind 3 because lo moves by 2 per column)
    t = rseq(rng, W)
    b = Builder([t])
    for m in (100, 150, 199, 201, 300, 399, 400):
        p = rseq(rng, m) if m != W else t
        b.rec(0, 0, p, stretch_cigar(W, m), rev=m % 2 == 1)
    cases.append(b.case("piece_lengths", reach=all_of(need(any_w("seg_max", lambda x: x == 400), "no 400-base piece"),
                                                      need(any_w("seg_min", lambda x: x == 100), "no 100-base piece"),
                                                      need(any_w("kind3", lambda x: x > 0), "no row of kind 3"),
                                                      need(any_w("kind1", lambda x: x > 0), "no row of kind 1"))))
    # the ring: an insertion of 15 / 16 / 17 / 18 bases before one column -> the column's draft predecessor 16 / 17 / 18 / 19
    # ranks back (16 is the last one read from the ring in LDS).  A homopolymer of a base the draft lacks around the column: a
    # random insertion is often split into several (linear gaps)
    for k in (15, 16, 17, 18):
        t = rseq(rng, W)
        t = t[:80] + "".join("CGT"[(i * 7 + k) % 3] for i in range(20)) + t[100:]
        b = Builder([t])
        for s in range(2):
            p, cg = edit(t, ins={90: "A" * k})
            b.rec(0, 0, p, cg, rev=bool(s & 1))
        for s in range(4):                              # the draft's path again: a row whose predecessor is that far back
            b.rec(0, 0, t, [M(W)], rev=bool(s & 1))
        far = k + 1 > RING
        cases.append(b.case("ring_ins%d" % k, reach=need(lambda ws, c, far=far: (ws[0]["far_rows"] > 0) == far and ws[0]["kind2"] + ws[0]["kind3"] > 0,
                                                         "far rows %s expected" % ("some" if far else "none"))))
    # in-degree: deletions of 1 .. 10 bases that all end in front of the same column give it 11 distinct predecessors: the 9th
    # and later are dropped, and their sources' out-edges are not counted; six more pieces with the 9th predecessor's deletion
    # would outweigh the draft's edge if it had been kept
    def indeg(t):
        b = Builder([t])
        for k in list(range(1, 11)) + [8] * 6:
            p, cg = edit(t, dels={100 - k: k})
            b.rec(0, 0, p, cg, rev=bool(k & 1))
        for s in range(3):
            b.rec(0, 0, t, [M(W)])
        return b
    cases.append(search(rng, indeg, "in_degree_cap", all_of(need(lambda ws, c: ws[0]["max_in"] == MAXIN, "in-degree cap not reached"),
                                                            need(lambda ws, c: ws[0]["dropped_in"] >= 6, "the 9th predecessor's edges kept"))))
    # walk back: longest diagonal run of exactly 63 / 64 / 65 steps (one-base deletions every R + 1 columns), and runs broken by
    # the second predecessor (later pieces follow the deletion edges)
    for R in (63, 64, 65):
        def runs(t, R=R):
            b = Builder([t])
            dl = {c: 1 for c in range(R, W - 1, R + 1)}
            for s in range(4):
                p, cg = edit(t, dels=dl)
                b.rec(0, 0, p, cg, rev=bool(s & 1))
            return b
        cases.append(search(rng, runs, "walk_run_%d" % R, all_of(need(lambda ws, c, R=R: ws[0]["diag_run"] == R, "longest run is not %d" % R),
                                                                 need(lambda ws, c: ws[0]["diag_k1"] > 0, "no diagonal step from a second predecessor"))))
    # voting pieces: 70 records with every 6th carrying an N: the first 64 clean ones vote; min_depth exactly met or missed
    t = rseq(rng, W)
    b = Builder([t])
    for i in range(80):
        p, cg = edit(t, subs={int(rng.integers(0, W)): "ACGT"[i % 4]})
        if i % 6 == 5:
            p = p[:20] + "N" + p[21:]
        b.rec(0, 0, p, cg, rev=bool(i & 1))
    cases.append(b.case("maxseg_with_n", md=(64, 65), reach=all_of(need(lambda ws, c: ws[0]["voting"] == MAXSEG, "not 64 voting pieces"),
                                                                   need(lambda ws, c: ws[0]["offered"] > MAXSEG, "no N piece offered"))))
    t = rseq(rng, W)
    b = Builder([t])
    for i in range(5):
        p, cg = edit(t, subs={50: "ACGT"[(("ACGT".find(t[50])) + 1) % 4]})
        b.rec(0, 0, p, cg, rev=bool(i & 1))
    cases.append(b.case("min_depth_edge", md=(5, 6), reach=need(lambda ws, c: ws[0]["voting"] == 5, "not 5 voting pieces")))
    # heaviest-bundle ties: two alternative bases with equal counts (equal edge weight, equal score); pieces that begin / end
    # one base off so that startc / endc tie
    t = rseq(rng, W)
    b = Builder([t])
    for i in range(4):
        p, cg = edit(t, subs={80: other(t[80], 1 + (i & 1)), 120: other(t[120], 1 + (i >> 1))})
        b.rec(0, 0, p, cg, rev=bool(i & 1))
    cases.append(b.case("bundle_weight_ties"))
    t = rseq(rng, 2 * W)
    b = Builder([t])
    for i in range(4):
        # the first window's piece loses its last base / the second's its first: startc and endc tie with the draft's
        if i < 2:
            b.rec(0, 0, t[:W - 1] + t[W:2 * W], [M(W - 1), D(1), M(W)])
        else:
            b.rec(0, 0, t[:W] + t[W + 1:], [M(W), D(1), M(W - 1)], rev=True)
    cases.append(b.case("start_end_ties"))
    # the node cap: random pieces add many nodes; then the last piece sized so that n + m = 2048 (merged) or 2049 (left out)
    # dead cells: three pieces lack 41 draft bases and carry 8 bases no node has right behind the gap (new nodes of columns
    # 101-108 whose only predecessor is column 59); a 400-base piece then puts those rows' bands 84 columns right of their
    # predecessor's, so every candidate lies outside a band: rows of cells at exactly -32000, and chains of them
    t = rseq(rng, W)
    t = t[:59] + "A" + "".join("CGT"[x] for x in rng.integers(0, 3, 60)) + t[120:]
    short, long_ = t[:60] + "A" * 8 + t[109:], "".join(x + x for x in t)
    b = Builder([t])
    for s in range(3):
        b.rec(0, 0, short, stretch_cigar(W, len(short)), rev=bool(s & 1))
    b.rec(0, 0, long_, stretch_cigar(W, SEGMAX))
    for s in range(2):
        b.rec(0, 0, t, [M(W)], rev=bool(s & 1))
    cases.append(b.case("dead_cells", reach=need(lambda ws, c: ws[0]["best_min"] == -32000, "no cell at -32000")))
    cases += node_cap_cases(rng)
    return cases


def oracle_stats(case, min_depth=1):
    from oracle import binding as ob
    return ob.consensus(case["alns"], case["cigars"], case["reads"], case["targets"], min_depth=min_depth, poa=True, stats=True)[1]


def search(rng, make, name, reach, tries=200, **kw):
    """make(draft) -> Builder, on fresh random drafts until the oracle shows the case reaches its edge (whether a deletion or a
    run lands where it is aimed depends on the draft's bases around it)"""
    for _ in range(tries):
        c = make(rseq(rng, W)).case(name, reach=reach, **kw)
        if reach(oracle_stats(c), c) is None:
            return c
    raise AssertionError("%s: no draft in %d reaches the edge" % (name, tries))


def node_cap_cases(rng):
    t = rseq(rng, W)
    pieces = []

    def nodes(ps):
        b = Builder([t])
        for p in ps:
            b.rec(0, 0, p, stretch_cigar(W, len(p)))
        return oracle_stats(b.case("probe"))[0]["nodes"]
    n = W
    while n < MAXNODE - SEGMAX:
        pieces.append(rseq(rng, min(SEGMAX, MAXNODE - 100 - n)))
        n = nodes(pieces)
    assert MAXNODE - SEGMAX <= n <= MAXNODE - W // 2, n
    out = []
    for extra, merged in ((0, True), (1, False)):
        m = MAXNODE + extra - n
        b = Builder([t])
        for k, p in enumerate(pieces + [rseq(rng, m), t]):
            b.rec(0, 0, p, stretch_cigar(W, len(p)), rev=bool(k & 1))
        last = len(pieces)

        def reach(ws, c, last=last, m=m, extra=extra, merged=merged):
            w = ws[0]
            if w["nbefore"][last] + m != MAXNODE + extra:
                return "n + m = %d" % (w["nbefore"][last] + m)
            if (w["capped"] == 0) != merged:
                return "capped %d" % w["capped"]
            return None
        out.append(b.case("node_cap_%d" % (MAXNODE + extra), md=(1,), reach=reach))
    return out


# ---- pile-up cases -----------------------------------------------------------------------------------------------------------
def pile_cases(rng):
    cases = []
    # 64 CIGAR ops per trip: n_cigar 63 / 64 / 65 / 129; M runs of 31 / 32 / 33 on both strands, with query offsets of every
    # residue mod 32 on the alignment strand and on the stored strand (the 32-base fetch)
    for nop in (63, 64, 65, 129):
        t = rseq(rng, 1200)
        b = Builder([t])
        for s in range(4):
            ops, p, ti, q = [], [], 7 * s, []
            while len(ops) < nop - 1:
                ops.append(M(3 + (len(ops) % 5))); q.append(t[ti:ti + 3 + (len(ops) - 1) % 5]); ti += 3 + (len(ops) - 1) % 5
                if len(ops) < nop - 1:
                    if len(ops) % 4 == 1:
                        ins = rseq(rng, 1 + len(ops) % 3); ops.append(I(len(ins))); q.append(ins)
                    else:
                        ops.append(D(1 + len(ops) % 2)); ti += 1 + (len(ops) - 1) % 2
            ops.append(M(5)); q.append(t[ti:ti + 5])
            b.rec(0, 7 * s, "".join(q), ops, rev=bool(s & 1), left=rseq(rng, s), right=rseq(rng, 3 - s))
        cases.append(b.case("pile_ncigar_%d" % nop, poa=False, reach=need(lambda ws, c, nop=nop: int(c["alns"]["n_cigar"].max()) == nop, "n_cigar")))
    t = rseq(rng, 300)
    b = Builder([t])
    for L in (31, 32, 33):
        for rev in (False, True):
            for off in range(32):                     # the query offset on the alignment strand (left) and on the stored one (right)
                ts = 10 + (off * 7 + L) % 250
                sub = t[ts:ts + L]
                sub = sub[:L // 2] + other(sub[L // 2]) + sub[L // 2 + 1:]
                b.rec(0, ts, sub, [M(L)], rev=rev, left=rseq(rng, off), right=rseq(rng, (5 * off + 3) % 32))
    cases.append(b.case("pile_m_runs", poa=False))
    # inserted bases: I of 7 / 8 / 9 (CONS_KMAX), an I at ts (not counted), an I after the target's last base
    t = rseq(rng, 120)
    b = Builder([t])
    for k, at in ((7, 20), (8, 50), (9, 80)):
        ins = rseq(rng, k)
        for s in range(3):
            b.rec(0, at - 10, t[at - 10:at] + ins + t[at:at + 10], [M(10), I(k), M(10)], rev=bool(s & 1))
    for s in range(3):
        b.rec(0, 100, "GGG" + t[100:110], [I(3), M(10)], rev=bool(s & 1))
        b.rec(0, 110, t[110:120] + "TTTT", [M(10), I(4)], rev=not (s & 1))
    cases.append(b.case("pile_insertions", poa=False))
    # D of 30 / 31 (CONS_MAXDEL); 2 del == cov (kept) and 2 del > cov (dropped)
    t = rseq(rng, 200)
    b = Builder([t])
    for L, at in ((30, 20), (31, 110)):
        for s in range(3):
            b.rec(0, at - 10, t[at - 10:at] + t[at + L:at + L + 10], [M(10), D(L), M(10)], rev=bool(s & 1))
    for s in range(4):                                    # column 180: two deletions of four
        if s < 2:
            b.rec(0, 170, t[170:180] + t[181:190], [M(10), D(1), M(9)], rev=bool(s & 1))
        else:
            b.rec(0, 170, t[170:190], [M(20)], rev=bool(s & 1))
    for s in range(3):                                    # column 160: two of three
        if s < 2:
            b.rec(0, 150, t[150:160] + t[161:170], [M(10), D(1), M(9)], rev=bool(s & 1))
        else:
            b.rec(0, 150, t[150:170], [M(20)])
    cases.append(b.case("pile_deletions", poa=False))
    # 2 insn == cov (not emitted) against a strict majority; base-count ties against the draft base and between two others;
    # coverage min_depth - 1 / min_depth; reads with N bases
    t = rseq(rng, 100)
    b = Builder([t])
    for s in range(4):
        ins = "A" if s < 2 else ""
        p = t[10:30] + ins + t[30:40]
        b.rec(0, 10, p, [M(20), I(1), M(10)] if ins else [M(30)], rev=bool(s & 1))
    for s in range(4):                                    # column 60: 2 x draft, 2 x other; column 70: 2 x X, 2 x Y
        subs = {60: other(t[60])} if s < 2 else {}
        subs[70] = other(t[70], 1 + (s & 1))
        seg = t[50:80]
        p = "".join(subs.get(50 + i, seg[i]) for i in range(30))
        if s == 3:
            p = p[:5] + "N" + p[6:]
        b.rec(0, 50, p, [M(30)], rev=bool(s & 1))
    cases.append(b.case("pile_ties", poa=False, md=(4, 5)))
    # many short targets: target boundaries inside one 256-thread block of k_pile_call
    tg = [rseq(rng, n) for n in (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 7, 1, 300)]
    b = Builder(tg)
    for tid, x in enumerate(tg):
        for s in range(3):
            if len(x) >= 3:
                p = x[:1] + other(x[1]) + x[2:]
                b.rec(tid, 0, p, [M(len(x))], rev=bool(s & 1))
            else:
                b.rec(tid, 0, x + "C", [M(len(x)), I(1)], rev=bool(s & 1))
    cases.append(b.case("pile_short_targets", poa=True))
    return cases


def cases(seed=11):
    rng = np.random.default_rng(seed)
    return poa_cases(rng) + pile_cases(rng)


def resident_case(seed=23):
    """four records on two short targets, for the consumers of a result's CIGAR array that take it resident on the device or
    upload it (telr_consensus_build, telr_depth_medians): a record without ops, one of a single op, one of 65 words (two steps
    of a 64-words-per-step walk) and one of 64 words exactly; every read differs from its target, so the votes show"""
    rng = np.random.default_rng(seed)
    t0, t1 = rseq(rng, 700), rseq(rng, 400)
    b = Builder([t0, t1])
    b.rec(0, 5, "", [], left=rseq(rng, 40))
    x = t1[30:150]
    b.rec(1, 30, x[:60] + other(x[60]) + x[61:], [M(120)])
    seg = t0[100:270]
    piece, cig = edit(seg, subs={2: other(seg[2])}, ins={5 + 10 * k: "A" for k in range(16)}, dels={10 + 10 * k: 1 for k in range(16)})
    assert len(cig) == 65
    b.rec(0, 100, piece, cig)
    seg = t0[300:465]
    piece, cig = edit(seg, subs={2: other(seg[2])}, ins={5 + 10 * k: "C" for k in range(16)}, dels={10 + 10 * k: 1 for k in range(15)})
    cig = cig[:-1] + [M((cig[-1] >> 4) - 2), M(2)]                  # (63 words as merged: the last M run as two words)
    assert len(cig) == 64 and cig[-2] >> 4 > 0
    b.rec(0, 300, piece, cig, rev=True)
    return b.case("resident_or_uploaded", poa=False)


def run_all(engine, cs=None):
    """every case through telr_poa_build / telr_consensus_build against tor_poa / tor_consensus at each of its min_depth
    values -> (comparisons, list of differences)"""
    from oracle import binding as ob
    from telr_amd.presets import preset
    io, _ = preset("map-ont")
    n, bad = 0, []
    for c in cs or cases():
        ix = engine.index(c["targets"], io)
        qset = engine.seqset(c["reads"])
        r = ix.result_from_arrays(c["alns"], c["cigars"])
        try:
            for md in c["md"]:
                for poa in (False, True):
                    if not (c["poa"] if poa else c["pile"]):
                        continue
                    got = ix.consensus(r, qset, min_depth=md, poa=poa)
                    want = ob.consensus(c["alns"], c["cigars"], c["reads"], c["targets"], min_depth=md, poa=poa)
                    n += 1
                    if got != want:
                        bad.append("%s %s min_depth %d: targets %s differ" % (c["name"], "poa" if poa else "pile-up", md,
                                                                            [i for i in range(len(got)) if got[i] != want[i]]))
        finally:
            ix.free_raw(r); qset.free(); ix.free()
    return n, bad


if __name__ == "__main__":
    if "--engine" in sys.argv:          # one process per TELR_AB switch (tests/test_gpu_consensus_edges.py)
        import torch  # noqa: F401      (the engine binds to torch's HIP runtime, as in tests/conftest.py)
        from telr_amd.aligner import Engine
        n, bad = run_all(Engine(0))
        print("\n".join(bad[:40]))
        print("consensus edges %s: %d comparisons, %d differ" % ("ok" if not bad else "FAILED", n, len(bad)))
        sys.exit(1 if bad else 0)
    from oracle import binding as ob
    for c in cases():
        if c["poa"]:
            _, ws = ob.consensus(c["alns"], c["cigars"], c["reads"], c["targets"], min_depth=1, poa=True, stats=True)
            miss = c["reach"](ws, c) if c["reach"] else None
            agg = {k: max(w[k] for w in ws) for k in ("voting", "nodes", "max_in", "dropped_in", "far_rows", "kind3", "diag_run", "capped")}
            print("%-22s %s %s" % (c["name"], "MISSED " + miss if miss else "ok", agg))
        else:
            print("%-22s pile-up, %d records" % (c["name"], len(c["alns"])))
