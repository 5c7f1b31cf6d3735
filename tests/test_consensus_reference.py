"""The two consensus oracles (tor_consensus, tor_poa) against int64 references in Python, on the hand-built edge cases of tests/consensus_edges.py; the reach of every POA case from tor_poa_stats; whether any cell of
the oracle's banded DP falls below the int16 range (the dead-cell rule); and the host check both HIP consensus builds run on
their records before any launch (telr_debug_check_records).  CPU only; tests/test_gpu_consensus_edges.py holds the kernels
against the oracle on the same cases.

The pile-up reference is written from DESIGN 3.12 and the comments of pileup.hip.h.  The POA reference is NOT independent of
the oracle: it restates tor_poa's algorithm step for step (the same ring search, the same `behind` bookkeeping, the same
anchor-ordered insertion into the order), in unbounded integers.  It catches int16 truncation and C slips in the oracle, not a
misreading of DESIGN 3.13 that both share."""
import ctypes as C

import numpy as np
import pytest

import consensus_edges as ce
from oracle import binding as ob
from telr_amd._abi import ALN_DTYPE, TELR_E_ARG, TELR_OK

NT4 = {c: i for i, c in enumerate("ACGT")}
NT4.update({c.lower(): i for c, i in list(NT4.items())})
POA_M, POA_X, POA_G, BAND, DEAD = 3, -5, -4, 64, -32000


@pytest.fixture(scope="module")
def cases():
    return ce.cases()


def _code(c):
    return NT4.get(c, 4)


def _aligned(case, a):
    """the read of record a on its alignment strand, as codes 0..4"""
    q = [_code(c) for c in case["reads"][int(a["qid"])]]
    if a["flags"] & 8:
        q = [3 - b if b < 4 else 4 for b in q[::-1]]
    return q


def _ops(case, a):
    return [(int(c) & 15, int(c) >> 4) for c in case["cigars"][int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]]


def _primary(case):
    return [a for a in case["alns"] if not a["flags"] & 6]


# ---- pile-up, spec 3.12 ------------------------------------------------------------------------------------------------------
def pileup_reference(case, min_depth):
    out = []
    cells = []
    for tid, t in enumerate(case["targets"]):
        L = len(t)
        base = np.zeros((L, 4), np.int64); dele = np.zeros(L, np.int64); nq = np.zeros(L, np.int64)
        insn = np.zeros((L, ce.KMAX), np.int64); insb = np.zeros((L, ce.KMAX, 4), np.int64)
        for a in _primary(case):
            if a["tid"] != tid:
                continue
            q = _aligned(case, a)
            qi, ti = int(a["qlen"] - a["qe"]) if a["flags"] & 8 else int(a["qs"]), int(a["ts"])
            for op, n in _ops(case, a):
                if op == 0:
                    for x in range(n):
                        b = q[qi + x]
                        if b < 4:
                            base[ti + x, b] += 1
                        else:
                            nq[ti + x] += 1
                    qi += n; ti += n
                elif op == 2:
                    if n <= ce.MAXDEL:
                        dele[ti:ti + n] += 1
                    ti += n
                else:
                    if ti > int(a["ts"]):                  # an insertion in front of the first aligned base hangs on nothing
                        for x in range(min(n, ce.KMAX)):
                            insn[ti - 1, x] += 1
                            if q[qi + x] < 4:
                                insb[ti - 1, x, q[qi + x]] += 1
                    qi += n
        s = []
        for p in range(L):
            d = _code(t[p]); draft = "ACGTN"[d]
            cov = int(base[p].sum() + dele[p] + nq[p])
            if cov < min_depth:
                s.append(draft)
                continue
            if 2 * dele[p] <= cov:
                bv = int(base[p].max())
                if bv == 0:
                    s.append(draft)
                elif d < 4 and base[p, d] == bv:
                    s.append(draft)
                else:
                    s.append("ACGT"[int(np.argmax(base[p]))])
            for k in range(ce.KMAX):
                if 2 * insn[p, k] <= cov:
                    break
                s.append("ACGT"[int(np.argmax(insb[p, k]))] if insb[p, k].max() > 0 else "N")
        out.append("".join(s))
        cells.append(dict(base=base, dele=dele, nq=nq, insn=insn))
    return out, cells


# ---- window POA, spec 3.13: the oracle's algorithm, step for step, in Python integers ------------------------------------------
def window_pieces(case, tid, w0, w1):
    """the pieces of window [w0, w1) in record order: the query bases between the offsets where the target reaches w0 / w1"""
    out, offered = [], 0
    for a in _primary(case):
        if a["tid"] != tid or a["ts"] > w0 or a["te"] < w1:
            continue
        if len(out) == ce.MAXSEG:
            break
        qi, ti, qa, qb, big = int(a["qlen"] - a["qe"]) if a["flags"] & 8 else int(a["qs"]), int(a["ts"]), -1, -1, False
        for op, n in _ops(case, a):
            if op == 1:
                big |= n > 30 and w0 < ti <= w1
                qi += n
                continue
            if qa < 0 and w0 < ti + n:
                qa = qi + (w0 - ti) if op == 0 else qi
            big |= op == 2 and n > 30 and ti < w1 and ti + n > w0
            if w1 < ti + n:
                qb = qi + (w1 - ti) if op == 0 else qi
                break
            qi += n if op == 0 else 0
            ti += n
        if qb < 0:
            qb = qi
        if big or qa < 0 or not (w1 - w0) // 2 <= qb - qa <= ce.SEGMAX:
            continue
        offered += 1
        p = _aligned(case, a)[qa:qb]
        if max(p, default=0) < 4:
            out.append(p)
    return out, offered


class Graph:
    def __init__(self, draft):
        L = len(draft)
        self.L = L
        self.base = list(draft)
        self.ins = [[] if v == 0 else [v - 1] for v in range(L)]          # in-edges in the order they were made
        self.w = [[] if v == 0 else [1] for v in range(L)]
        self.nout = [1 if v < L - 1 else 0 for v in range(L)]
        self.ring = list(range(L)); self.order = list(range(L)); self.col = list(range(L))
        self.startc = [int(v == 0) for v in range(L)]; self.endc = [int(v == L - 1) for v in range(L)]

    def edge(self, u, v):
        if u in self.ins[v]:
            self.w[v][self.ins[v].index(u)] += 1
        elif len(self.ins[v]) < ce.MAXIN:
            self.ins[v].append(u); self.w[v].append(1); self.nout[u] += 1

    def add(self, seq, st):
        n, nodes = len(seq), len(self.base)
        rank = [0] * nodes
        for r, v in enumerate(self.order):
            rank[v] = r + 1
        lo = [max(0, min((self.col[v] + 1) * n // self.L - BAND // 2, n + 1 - BAND)) for v in self.order]
        H = {}

        def cell(row, j):
            if row == 0:
                return j * POA_G
            jj = j - lo[row - 1]
            return DEAD if jj < 0 or jj >= BAND or j > n else H[row - 1][jj]
        for r, v in enumerate(self.order):
            preds = [rank[u] for u in self.ins[v]] or [0]
            row = [DEAD] * BAND
            for j in range(lo[r], min(lo[r] + BAND - 1, n) + 1):
                best = DEAD
                for pr in preds:
                    best = max(best, cell(pr, j) + POA_G)
                    if j > 0:
                        best = max(best, cell(pr, j - 1) + (POA_M if seq[j - 1] == self.base[v] and seq[j - 1] < 4 else POA_X))
                if j > lo[r]:
                    best = max(best, row[j - 1 - lo[r]] + POA_G)
                st["min"] = min(st["min"], best); st["max"] = max(st["max"], best)
                row[j - lo[r]] = best
            H[r] = row
        endv, endsc = -1, -32768
        for v in range(nodes):
            if not self.nout[v]:
                sc = cell(rank[v], n)
                if sc > endsc:
                    endv, endsc = v, sc
        path, v, j = [], endv, n
        while v >= 0 or j > 0:
            if v < 0:
                path.append((-1, j - 1)); j -= 1
                continue
            cur = cell(rank[v], j)
            preds = self.ins[v] or [-1]
            moved = False
            if j > 0:
                sc = POA_M if seq[j - 1] == self.base[v] and seq[j - 1] < 4 else POA_X
                for p in preds:
                    if cell(rank[p] if p >= 0 else 0, j - 1) + sc == cur:
                        path.append((v, j - 1)); v, j, moved = p, j - 1, True
                        break
            if not moved:
                for p in preds:
                    if cell(rank[p] if p >= 0 else 0, j) + POA_G == cur:
                        v, moved = p, True
                        break
            if not moved:
                path.append((-1, j - 1)); j -= 1
        # merge, start -> end; new nodes go behind the node they are aligned to / behind the last old node of the column before
        prev, behind, new = -1, -1, []
        for x, jj in reversed(path):
            b = seq[jj]
            u = -1
            if x >= 0:
                s_ = x
                while True:
                    if self.base[s_] == b:
                        u = s_
                        break
                    s_ = self.ring[s_]
                    if s_ == x:
                        break
            if u < 0:
                u = len(self.base)
                self.base.append(b); self.ins.append([]); self.w.append([]); self.nout.append(0); self.startc.append(0); self.endc.append(0)
                self.col.append(self.col[x] if x >= 0 else self.col[prev] if prev >= 0 else 0)
                self.ring.append(u)
                new.append((u, rank[x] - 1 if x >= 0 else behind))
                if x >= 0:
                    self.ring[u] = self.ring[x]; self.ring[x] = u
            if x >= 0:
                m, s_ = rank[x] - 1, self.ring[x]
                while s_ != x:
                    if s_ < nodes:
                        m = max(m, rank[s_] - 1)
                    s_ = self.ring[s_]
                behind = m
            if prev >= 0:
                self.edge(prev, u)
            else:
                self.startc[u] += 1
            prev = u
        if prev >= 0:
            self.endc[prev] += 1
        order, k = [], 0
        while k < len(new) and new[k][1] < 0:
            order.append(new[k][0]); k += 1
        for i, v in enumerate(self.order):
            order.append(v)
            while k < len(new) and new[k][1] == i:
                order.append(new[k][0]); k += 1
        self.order = order

    def consensus(self):
        score, bp = {}, {}
        for v in self.order:
            bw, bs, b = -1, -1, -1
            for u, w in zip(self.ins[v], self.w[v]):
                if w > bw or (w == bw and score[u] > bs):
                    bw, bs, b = w, score[u], u
            bp[v] = b; score[v] = bs + bw if b >= 0 else 0
        endv = startv = -1
        for v in range(len(self.base)):
            if endv < 0 or self.endc[v] > self.endc[endv] or (self.endc[v] == self.endc[endv] and score[v] > score[endv]):
                endv = v
            if startv < 0 or self.startc[v] > self.startc[startv]:
                startv = v
        s, v = [], endv
        while v >= 0:
            s.append("ACGTN"[self.base[v]])
            if v == startv:
                break
            v = bp[v]
        return "".join(reversed(s))


def poa_reference(case, min_depth):
    out, st = [], {"min": 1 << 40, "max": -(1 << 40)}
    for tid, t in enumerate(case["targets"]):
        s = []
        for (_, w0, w1) in ce.windows([len(t)]):
            pieces, _ = window_pieces(case, tid, w0, w1)
            if len(pieces) < min_depth:
                s.append("".join("ACGTN"[_code(c)] for c in t[w0:w1]))
                continue
            g = Graph([_code(c) for c in t[w0:w1]])
            for p in pieces:
                if len(g.base) + len(p) <= ce.MAXNODE:
                    g.add(p, st)
            s.append(g.consensus())
        out.append("".join(s))
    return out, st


# ---- the tests ---------------------------------------------------------------------------------------------------------------
def test_pile_up_reference_equals_the_oracle(cases):
    for c in cases:
        if not c["pile"]:
            continue
        for md in c["md"]:
            want, _ = pileup_reference(c, md)
            assert ob.consensus(c["alns"], c["cigars"], c["reads"], c["targets"], min_depth=md) == want, (c["name"], md)


def test_pile_up_cases_reach_their_edges(cases):
    byname = {c["name"]: c for c in cases}
    _, cells = pileup_reference(byname["pile_deletions"], 1)
    cv = cells[0]["base"].sum(1) + cells[0]["dele"] + cells[0]["nq"]
    assert (2 * cells[0]["dele"] == cv)[cv > 0].any() and (2 * cells[0]["dele"] > cv).any()
    assert cells[0]["dele"][20:50].max() == 3 and cells[0]["dele"][110:141].max() == 0          # D 30 votes, D 31 does not
    _, cells = pileup_reference(byname["pile_insertions"], 1)
    assert cells[0]["insn"][:, ce.KMAX - 1].max() == 3                                            # the 8th inserted column
    _, cells = pileup_reference(byname["pile_ties"], 1)
    cv = cells[0]["base"].sum(1) + cells[0]["dele"] + cells[0]["nq"]
    assert (2 * cells[0]["insn"][:, 0] == cv)[cv > 0].any() and cells[0]["nq"].max() == 1
    for nop in (63, 64, 65, 129):
        assert int(byname["pile_ncigar_%d" % nop]["alns"]["n_cigar"].max()) == nop
    assert {31, 32, 33} <= {int(c) >> 4 for c in byname["pile_m_runs"]["cigars"]}


def test_poa_cases_reach_their_edges(cases):
    missed = []
    for c in cases:
        if c["poa"] and c["reach"]:
            r = c["reach"](ce.oracle_stats(c), c)
            if r:
                missed.append((c["name"], r))
    assert not missed, missed


SLOW = ("node_cap_2048", "node_cap_2049")


def test_poa_reference_equals_the_oracle(cases):
    for c in cases:
        if not c["poa"] or c["name"] in SLOW:
            continue
        for md in c["md"]:
            want, _ = poa_reference(c, md)
            got = ob.consensus(c["alns"], c["cigars"], c["reads"], c["targets"], min_depth=md, poa=True)
            assert got == want, (c["name"], md)


def test_poa_window_statistics_agree_with_the_reference(cases):
    """pieces offered / voting per window and the cell range from the oracle's tor_poa_stats against the reference"""
    for c in cases:
        if not c["poa"] or c["name"] in SLOW:
            continue
        ws = ce.oracle_stats(c)
        k = 0
        for tid, t in enumerate(c["targets"]):
            for (_, w0, w1) in ce.windows([len(t)]):
                pieces, offered = window_pieces(c, tid, w0, w1)
                assert (ws[k]["voting"], ws[k]["offered"]) == (len(pieces), offered), (c["name"], k)
                k += 1
        _, st = poa_reference(c, 1)
        assert min(w["best_min"] for w in ws if w["ran"]) == st["min"] and max(w["best_max"] for w in ws if w["ran"]) == st["max"], c["name"]


def test_dead_cells_never_leave_int16(cases):
    """the int16 wrap of a chain of dead cells: every stored cell is floored at -32000 (the oracle's `best` starts there, the
    kernel floors a cell's candidate before the row's gap chain), so no cell `best` is ever below -32768 before it is stored.
    `dead_cells` stores rows and chains of cells at exactly -32000 (the GPU test holds the kernel's strings to the oracle's
    there); every other case, the 2,048-node graphs included, keeps its cells live"""
    lo, hi = 1 << 40, -(1 << 40)
    for c in cases:
        if c["poa"]:
            for w in ce.oracle_stats(c):
                if w["ran"] and w["merged"]:
                    lo, hi = min(lo, w["best_min"]), max(hi, w["best_max"])
    assert lo == -32000 and hi <= 3 * ce.SEGMAX, (lo, hi)
    live = min(w["best_min"] for c in cases if c["poa"] and c["name"] != "dead_cells" for w in ce.oracle_stats(c) if w["ran"] and w["merged"])
    assert live > -4 * (ce.MAXNODE + ce.SEGMAX), live


# ---- the record check of both consensus builds ---------------------------------------------------------------------------
def _check(alns, cigars, qlens, tlens):
    from telr_amd import _lib
    L = _lib.lib()
    alns = np.ascontiguousarray(alns, dtype=ALN_DTYPE); cigars = np.ascontiguousarray(cigars, dtype=np.uint32)
    ql = np.ascontiguousarray(qlens, dtype=np.int32); tl = np.ascontiguousarray(tlens, dtype=np.int32)
    fb = C.c_int64(-2)
    rc = L.telr_debug_check_records(alns.ctypes.data, len(alns), cigars.ctypes.data, len(cigars), ql.ctypes.data, len(ql),
                                    tl.ctypes.data, len(tl), C.byref(fb))
    return rc, fb.value


def test_record_check_rejects_every_malformed_record(cases):
    for c in cases:                                       # every hand-built record passes
        rc, fb = _check(c["alns"], c["cigars"], [len(r) for r in c["reads"]], [len(t) for t in c["targets"]])
        assert (rc, fb) == (TELR_OK, -1), c["name"]
    M, I, D = ce.M, ce.I, ce.D
    good = np.zeros(3, ALN_DTYPE)
    good["qlen"] = 50; good["flags"] = 1
    good[0]["qid"], good[0]["tid"], good[0]["qs"], good[0]["qe"], good[0]["ts"], good[0]["te"] = 0, 0, 5, 45, 10, 48
    good[1]["qid"], good[1]["tid"], good[1]["qs"], good[1]["qe"], good[1]["ts"], good[1]["te"] = 1, 1, 0, 50, 0, 52
    good[2]["qid"], good[2]["tid"], good[2]["n_cigar"] = 0, 1, 0                      # no CIGAR: votes nothing, passes
    cig = [M(20), I(2), M(18)] + [M(10), D(4), M(30), I(2), M(8)]
    good["cigar_off"] = (0, 3, 8); good["n_cigar"] = (3, 5, 0)
    good[2]["ts"], good[2]["te"], good[2]["qs"], good[2]["qe"] = 3, 100, 0, 50         # (its extent is still checked)
    qlens, tlens = [50, 50], [60, 100]
    assert _check(good, cig, qlens, tlens) == (TELR_OK, -1)

    def bad(k, **kw):
        a = good.copy(); cg = list(cig)
        for f, v in kw.items():
            if f == "cig":
                cg = v
            else:
                a[k][f] = v
        return k, _check(a, cg, qlens, tlens)
    rejects = {
        "ts < 0": bad(0, ts=-1, te=37), "ts > te": bad(1, ts=53), "te > tlen": bad(0, ts=23, te=61),
        "tid < 0": bad(1, tid=-1), "tid >= nt": bad(1, tid=2), "qid < 0": bad(0, qid=-1), "qid >= nq": bad(0, qid=2),
        "qs < 0": bad(0, qs=-1, qe=39), "qs > qe": bad(2, qs=20, qe=10), "qe > qlen": bad(0, qs=11, qe=51),
        "qlen != the query's": bad(0, qlen=48), "M + D != te - ts": bad(0, te=47), "M + I != qe - qs": bad(0, qe=44),
        "op S": bad(0, cig=[M(20), 2 << 4 | 4, M(18)] + cig[3:]), "op =": bad(0, cig=[M(20), I(2), 18 << 4 | 7] + cig[3:]),
        "op X": bad(0, cig=[M(20), I(2), 18 << 4 | 8] + cig[3:]), "op N": bad(1, cig=cig[:3] + [M(10), 4 << 4 | 3, M(30), I(2), M(8)]),
        "CIGAR past the array": bad(1, n_cigar=6), "cigar_off < 0": bad(1, cigar_off=-1), "n_cigar < 0": bad(1, n_cigar=-1),
    }
    for what, (k, (rc, fb)) in rejects.items():
        assert (rc, fb) == (TELR_E_ARG, k), (what, rc, fb)
