"""The stretch between the per-problem DP results and a record's numbers and CIGAR, aimed at its kernel edges: the retry pass
(k_retry_collect: one ballot-ranked append per wave; k_retry_build: the wide band or "kind 4 = nothing to redo"; k_retry_merge),
the per-chain sums (k_chain_stats: a 64-lane strided sum, the convex-cost rounding, the reach of the end extensions), DpRes.mcols of
every trace-back walk, CIGAR stitching (k_stitch_count: 64 problems per iteration of one wave, three carries across iterations;
k_stitch_write: eight lanes per problem) and the per-class accounts (k_dp_account).

Two kinds of cases, each a dict with a `name`, the input of one call of a tap and `reach`, a function of the REFERENCE's output
that asserts the edge the case is built for is there (no case needs the engine to know whether it hit its edge):

  stitch cases  (Engine.debug_stitch)  hand-made per-problem results and CIGAR words; the reference is ref_stitch
  align cases   (Engine.debug_align)   real sequences, chains of DP problems; the reference is ref_align, made of the oracle's
                                       per-problem DP (tor_debug_dp) and a plain restatement of the retry rule, the stitching and
                                       the sums of the oracle's align_chain

tests/test_align_ref.py holds the references to hand-derived results and to the oracle's own align_chain and checks every reach on
the CPU; tests/test_gpu_align_edges.py holds the two taps to the references.  All comparisons are exact."""
import numpy as np

import dp_edges as D
from backtrack_edges import _fill_band, _fill_band_wide, _even_lo
from telr_amd.aligner import Engine
from telr_amd.presets import preset
from telr_amd._abi import N_DPCLS

WAVE = 64                   # problems per iteration of k_stitch_count, lanes per ballot of k_retry_collect
M, I, DEL = 0, 1, 2
DP_DMAX = D.DP_DMAX
ADAPT_MAX_STEPS = D.ADAPT_MAX_STEPS


def op(ln, code):
    return (int(ln) << 4) | int(code)


# ---------------------------------------------------------------------------------------------------------------------
# stitching, restated


def forward_ops(words, is_left):
    """a problem's ops in forward order: the raw buffer holds them end to start of the DP problem, which IS left to right on the
    forward sequences for a left extension (its DP runs down from the chain's start)"""
    w = [int(x) for x in words]
    return w if is_left else w[::-1]


def ref_stitch(case, trace=False):
    """-> per chain a dict {dp, mlen, blen, l_bi, l_bj, r_bi, r_bj, n_cigar, cigar}.  trace: also `skips` (problems of the chain
    whose first op merged into an earlier problem's tail) and `gone` (problems that wrote nothing although they had ops)"""
    S = int(case["cx_scale"])
    out = []
    for k in range(len(case["has_left"])):
        p0, p1 = int(case["p_off"][k]), int(case["p_off"][k + 1])
        cig, skips, gone = [], [], []
        for x in range(p0, p1):
            ops = forward_ops(case["cigars"][x], x == p0 and case["has_left"][k])
            if not ops:
                continue                                            # an empty problem: as if it were not there
            before = len(cig)
            for z, w in enumerate(ops):
                if cig and (cig[-1] & 0xf) == (w & 0xf):
                    cig[-1] += (w >> 4) << 4
                    if z == 0:
                        skips.append(x - p0)
                else:
                    cig.append(w)
            if len(cig) == before:
                gone.append(x - p0)
        pr = [[int(v) for v in case["prob"][x]] for x in range(p0, p1)]
        sc = sum(r[0] for r in pr)
        r = dict(dp=(sc + S // 2) // S if S > 0 else sc, mlen=sum(r[3] for r in pr), blen=sum(r[1] + r[2] - r[4] for r in pr),
                 l_bi=pr[0][1], l_bj=pr[0][2], r_bi=pr[-1][1], r_bj=pr[-1][2], n_cigar=len(cig), cigar=np.array(cig, np.uint32))
        if trace:
            r.update(skips=skips, gone=gone, score_sum=sc)
        out.append(r)
    return out


# ---- building stitch cases ----------------------------------------------------------------------------------------------


class Stitch:
    """chains added one by one; a chain is a list of problems, a problem a list of (length, op code) in FORWARD order"""

    def __init__(self, name, cx_scale=0, seed=0):
        self.name, self.cx_scale = name, cx_scale
        self.rng = np.random.default_rng(seed)
        self.p_off, self.has_left, self.prob, self.cigars = [0], [], [], []

    def chain(self, problems, has_left=0, scores=None, score_sum=None):
        rng = self.rng
        n = len(problems)
        assert n >= 1
        if scores is None:
            scores = [int(v) for v in rng.integers(-40, 200, n)]
        if score_sum is not None:                                   # the last problem makes the sum
            scores = list(scores[:-1]) + [score_sum - sum(scores[:-1])]
        for x, ops in enumerate(problems):
            words = [op(ln, c) for ln, c in ops]
            for a, b in zip(words, words[1:]):
                assert (a & 0xf) != (b & 0xf), "the trace-back never leaves equal neighbours inside a problem"
            self.cigars.append(np.array(words if (x == 0 and has_left) else words[::-1], np.uint32))
            mcols = sum(ln for ln, c in ops if c == M)
            bi = mcols + sum(ln for ln, c in ops if c == I)
            bj = mcols + sum(ln for ln, c in ops if c == DEL)
            if not ops and x in (0, n - 1) and rng.random() < 0.5:
                bi = bj = 0                                         # (an extension that came back empty)
            elif not ops:
                bi, bj = int(rng.integers(0, 5)), int(rng.integers(0, 5))      # the sums take every problem, with ops or not
            self.prob.append((scores[x], bi, bj, int(rng.integers(0, mcols + 1)), mcols))
        self.p_off.append(self.p_off[-1] + n)
        self.has_left.append(int(has_left))
        return self

    def done(self, reach, note=""):
        return dict(name=self.name, note=note, kind="stitch", cx_scale=self.cx_scale, p_off=np.array(self.p_off, np.int32),
                    has_left=np.array(self.has_left, np.int32), prob=np.array(self.prob, np.int32).reshape(-1, 5), cigars=self.cigars,
                    reach=reach)


def rand_ops(rng, n, first=None, last=None):
    """n ops, neighbours different, first / last code as asked"""
    if n == 0:
        return []
    while True:
        codes = [int(rng.integers(0, 3)) if first is None else first]
        while len(codes) < n:
            codes.append(int((codes[-1] + rng.integers(1, 3)) % 3))
        if last is None or codes[-1] == last:
            break
        if n == 1:
            assert first is None or first == last
            codes = [last]
            break
        if n == 2 and first is not None and first == last:
            raise AssertionError("two different neighbours cannot share a code")
    return [(int(rng.integers(1, 40)), c) for c in codes]


def rand_chain(rng, P, p_empty=0.0, max_ops=3):
    return [[] if rng.random() < p_empty else rand_ops(rng, int(rng.integers(1, max_ops + 1))) for _ in range(P)]


def total_ops(case):
    return int(sum(len(c) for c in case["cigars"]))


def _crossings(ref):
    """window boundaries a merge crossed: the indices 64, 128, ... among a chain's skips"""
    return [[s for s in r["skips"] if s % WAVE == 0 and s > 0] for r in ref]


# The names are written out so that a test file can list its cases without building them: building the align cases asks the library
# for its DP limits, and the library is loaded inside a test (after the engine fixture has loaded torch's HIP runtime), never at import.
STITCH_NAMES = ("st_counts", "st_counts_sparse", "st_one_op_130_left0", "st_one_op_130_left1", "st_runs_62_65", "st_empty_tail_then_merge",
                "st_empties", "st_skip_and_owner", "st_nine_pairs", "st_left_direction", "st_writer_lanes", "st_chains_1", "st_chains_2",
                "st_chains_300", "st_sums_cx0", "st_sums_cx10", "st_sums_cx20")
ALIGN_NAMES = ("al_counts", "al_empty_ext", "al_retry_0", "al_retry_1", "al_retry_63", "al_retry_64", "al_retry_65", "al_retry_257",
               "al_retry_at_63_64_255_256", "al_retry_lane_63_only", "al_retry_lane_0_of_block_1", "al_retry_steps_edge",
               "al_retry_nothing_to_redo", "al_retry_class_change", "al_classes_map-ont", "al_classes_ext63-z400", "al_classes_ext127-z400",
               "al_classes_ext511-z400", "al_convex_ngmlr-ont", "al_convex_ngmlr-pacbio", "al_accounts_255", "al_accounts_256", "al_accounts_257")
STITCH_P = (1, 2, 63, 64, 65, 127, 128, 129, 200)
OPCOUNTS = (1, 7, 8, 9, 16, 17, 70)
CX_SCALES = (0, 10, 20)
_STITCH = None


def stitch_cases():
    global _STITCH
    if _STITCH is not None:
        return _STITCH
    C = []

    # problem counts on both sides of the 64-problem window, with and without a left extension
    b = Stitch("st_counts", seed=11)
    for P in STITCH_P:
        for hl in (0, 1):
            b.chain(rand_chain(b.rng, P, max_ops=2), hl)

    def reach(ref, case):
        assert sorted(set(np.diff(case["p_off"]))) == sorted(STITCH_P)
        assert any(_crossings(ref)[k] for k in range(len(ref))), "no merge across a window boundary"
        assert any(r["gone"] for r in ref) and any(r["skips"] for r in ref)
        assert 200 <= total_ops(case) <= 4000
    C.append(b.done(reach, "1 .. 200 problems per chain"))

    b = Stitch("st_counts_sparse", seed=12)
    for P in STITCH_P:
        for hl in (0, 1):
            b.chain(rand_chain(b.rng, P, p_empty=0.3, max_ops=3), hl)

    def reach(ref, case):
        empty = np.array([len(c) == 0 for c in case["cigars"]])
        assert empty.any() and any(_crossings(ref)[k] for k in range(len(ref)))
    C.append(b.done(reach, "the same with three problems in ten empty"))

    # 130 problems of one op each, one code: the whole chain is one op, the first problem's tail collects the other 129
    for hl in (0, 1):
        b = Stitch("st_one_op_130_left%d" % hl, seed=13)
        b.chain([[(int(b.rng.integers(1, 30)), M)] for _ in range(130)], hl)

        def reach(ref, case):
            assert ref[0]["n_cigar"] == 1 and ref[0]["skips"] == list(range(1, 130)) and ref[0]["gone"] == list(range(1, 130))
        C.append(b.done(reach, "extra of problem 0 collects across both window boundaries"))

    # runs of one-op problems over lanes 62 .. 65
    b = Stitch("st_runs_62_65", seed=14)
    for lead, follow in ((I, M), (M, M), (I, I), (M, DEL)):
        ch = rand_chain(b.rng, 62)
        ch[61] = rand_ops(b.rng, 2, last=lead)
        ch += [[(int(b.rng.integers(1, 9)), M)] for _ in range(4)]          # problems 62, 63, 64, 65
        ch.append(rand_ops(b.rng, 3, first=follow))
        ch += rand_chain(b.rng, 5)
        b.chain(ch, int(b.rng.integers(0, 2)))

    def reach(ref, case):
        got = [tuple(s for s in r["skips"] if 62 <= s <= 66) for r in ref]
        assert got == [(63, 64, 65, 66), (62, 63, 64, 65, 66), (63, 64, 65), (62, 63, 64, 65)], got
    C.append(b.done(reach, "the run starts an op of its own or merges on, and ends merged into or not"))

    # a window whose last problems are empty, then a merge: prev_code and owner come from the carries
    b = Stitch("st_empty_tail_then_merge", seed=15)
    for n_empty, tail_ops in ((4, 2), (1, 1), (63, 1), (10, 3)):
        ch = rand_chain(b.rng, 64 - n_empty - 1)
        ch.append(rand_ops(b.rng, tail_ops, last=DEL))
        ch += [[] for _ in range(n_empty)]
        ch.append([(7, DEL)] if tail_ops == 2 else rand_ops(b.rng, 2, first=DEL))       # problem 64
        ch += rand_chain(b.rng, 3)
        assert all(len(ch[x]) == 0 for x in range(64 - n_empty, 64)) and len(ch[64])
        b.chain(ch, n_empty & 1)

    def reach(ref, case):
        assert all(64 in r["skips"] for r in ref) and 64 in ref[0]["gone"] and 64 not in ref[1]["gone"]
    C.append(b.done(reach, "problem 64 merges into the last non-empty problem of the window before"))

    # empty problems: first, last, in the middle, a whole window of them (facing ops equal and unequal), a chain of nothing else
    b = Stitch("st_empties", seed=16)
    rng = b.rng
    b.chain([[]] + rand_chain(rng, 5), 1)                                            # 0: first (a left extension that came back empty)
    b.chain([[]] + rand_chain(rng, 5), 0)                                            # 1
    b.chain(rand_chain(rng, 5) + [[]], 0)                                            # 2: last
    b.chain([rand_ops(rng, 2, last=M), [], [], rand_ops(rng, 2, first=M)], 0)        # 3: in the middle, merging over them
    b.chain([rand_ops(rng, 2, last=M), [], rand_ops(rng, 2, first=I)], 1)            # 4
    for a, c in ((M, M), (M, I)):                                                    # 5, 6: problems 64 .. 127 empty = one whole iteration
        b.chain(rand_chain(rng, 63) + [rand_ops(rng, 2, last=a)] + [[] for _ in range(64)] + [rand_ops(rng, 3, first=c)] + rand_chain(rng, 2), 0)
    for a, c in ((I, I), (DEL, M)):                                                  # 7, 8: 64 empties across two iterations
        b.chain(rand_chain(rng, 9) + [rand_ops(rng, 1, last=a)] + [[] for _ in range(64)] + [rand_ops(rng, 1, first=c)] + rand_chain(rng, 2), 1)
    b.chain(rand_chain(rng, 3), 0)                                                   # 9
    b.chain([[], [], []], 1)                                                         # 10: nothing at all between two chains with ops
    b.chain(rand_chain(rng, 3), 0)                                                   # 11
    b.chain([[] for _ in range(130)], 0)                                             # 12: three iterations of nothing
    b.chain(rand_chain(rng, 2), 1)                                                   # 13

    def reach(ref, case):
        assert ref[3]["skips"] == [3] and ref[4]["skips"] == []
        assert 128 in ref[5]["skips"] and 128 not in ref[6]["skips"] and 74 in ref[7]["skips"] and 74 not in ref[8]["skips"]
        assert ref[10]["n_cigar"] == 0 and ref[12]["n_cigar"] == 0 and ref[9]["n_cigar"] > 0 and ref[11]["n_cigar"] > 0 and ref[13]["n_cigar"] > 0
    C.append(b.done(reach, "empties at every place; a zero in the offset scan"))

    # a merging problem with further ops stays an owner; a one-op problem that merges away, then a first op that differs
    b = Stitch("st_skip_and_owner", seed=17)
    b.chain([[(5, M), (2, I), (3, M)], [(4, M), (1, DEL), (6, M)], [(9, M)], [(2, M), (2, I)]], 0)
    b.chain([[(5, M), (2, I), (3, M)], [(4, M)], [(3, I), (8, M)], [(1, M)]], 1)

    def reach(ref, case):
        assert [op(5, M), op(2, I), op(7, M), op(1, DEL), op(17, M), op(2, I)] == list(ref[0]["cigar"]) and ref[0]["gone"] == [2]
        assert [op(5, M), op(2, I), op(7, M), op(3, I), op(9, M)] == list(ref[1]["cigar"]) and ref[1]["skips"] == [1, 3]
    C.append(b.done(reach, "skip = 1 and still an owner; a problem that writes nothing before one that does"))

    # all nine boundary pairs
    b = Stitch("st_nine_pairs", seed=18)
    for a in (M, I, DEL):
        for c in (M, I, DEL):
            for hl in (0, 1):
                b.chain([rand_ops(b.rng, 2, last=a), rand_ops(b.rng, 2, first=c)], hl)

    def reach(ref, case):
        assert [r["n_cigar"] for r in ref] == [3 if a == c else 4 for a in range(3) for c in range(3) for _ in range(2)]
    C.append(b.done(reach, "M / I / D facing M / I / D"))

    # the read direction of a left extension
    b = Stitch("st_left_direction", seed=19)
    asym = [(5, M), (2, I), (7, M)]
    b.chain([asym, [(3, DEL), (4, M)]], 1)
    b.chain([asym, [(3, DEL), (4, M)]], 0)
    b.chain([asym], 1)
    b.chain([[(5, M), (2, I), (7, DEL)], [(3, DEL), (4, M)]], 1)          # forwards the tail is D (merges), backwards it would be M

    def reach(ref, case):
        want = [op(5, M), op(2, I), op(7, M), op(3, DEL), op(4, M)]
        assert list(ref[0]["cigar"]) == want and list(ref[1]["cigar"]) == want and ref[3]["n_cigar"] == 4
        # the stored words of the two first problems are each other's reverse
        assert list(case["cigars"][0]) == list(case["cigars"][2][::-1]) == [op(5, M), op(2, I), op(7, M)]
    C.append(b.done(reach, "5M 2I 7M stored forwards (left extension) and backwards"))

    # the eight-lane writer: problems of 1 .. 70 ops, first op kept or merged away, read forwards and backwards
    b = Stitch("st_writer_lanes", seed=20)
    for n in OPCOUNTS:
        for hl in (0, 1):
            first = rand_ops(b.rng, n)
            b.chain([first, rand_ops(b.rng, n), rand_ops(b.rng, n, first=M if n != 2 else None), [(3, M)]], hl)
            b.chain([rand_ops(b.rng, 2, last=I), rand_ops(b.rng, n, first=I), [(2, I)] if n == 1 else rand_ops(b.rng, 2)], hl)

    def reach(ref, case):
        assert set(OPCOUNTS) <= set(len(c) for c in case["cigars"])
        merged = {len(case["cigars"][int(case["p_off"][k]) + s]) for k, r in enumerate(ref) for s in r["skips"]}
        assert set(OPCOUNTS) <= merged
    C.append(b.done(reach, "1, 7, 8, 9, 16, 17, 70 ops with skip 0 and 1"))

    # chains per call
    for n in (1, 2, 300):
        b = Stitch("st_chains_%d" % n, seed=21 + n)
        for _ in range(n):
            b.chain(rand_chain(b.rng, int(b.rng.integers(1, 6)), p_empty=0.15), int(b.rng.integers(0, 2)))

        def reach(ref, case, n=n):
            assert len(ref) == n
        C.append(b.done(reach, "%d chains in one call" % n))

    # the sums and the rounding of the convex-cost score
    for S in CX_SCALES:
        b = Stitch("st_sums_cx%d" % S, cx_scale=S, seed=30 + S)
        U = S if S else 10
        targets = [-7 * U - 3, -3 * U - 1, -3 * U, -U - U // 2 - 1, -U - U // 2, -U, -U // 2 - 1, -U // 2, -U // 2 + 1, -1, 0, 1,
                   U // 2 - 1, U // 2, U // 2 + 1, U - 1, U, U + U // 2 - 1, U + U // 2, 2 * U, 7 * U + 3, 100 * U, 100 * U + U // 2 - 1]
        for t in targets:
            for P in (1, 3, 70, 130):
                b.chain(rand_chain(b.rng, P, max_ops=1 if P > 3 else 3), int(b.rng.integers(0, 2)), score_sum=t)

        def reach(ref, case, S=S, targets=targets):
            sums = [r["score_sum"] for r in ref]
            assert sums == [t for t in targets for _ in range(4)]
            if S:
                assert {-S // 2, -1, 0, S // 2 - 1, S // 2, S, 2 * S, -S} <= set(sums) and min(sums) < -S
                assert [r["dp"] for r in ref if r["score_sum"] == -S // 2][0] == 0 and [r["dp"] for r in ref if r["score_sum"] == -S // 2 - 1][0] == -1
                assert [r["dp"] for r in ref if r["score_sum"] == S // 2 - 1][0] == 0 and [r["dp"] for r in ref if r["score_sum"] == S // 2][0] == 1
            else:
                assert [r["dp"] for r in ref] == sums
        C.append(b.done(reach, "score sums at the rounding edges, 1 .. 130 problems per chain"))

    assert tuple(c["name"] for c in C) == STITCH_NAMES
    _STITCH = C
    return C


def stitch_case(name):
    return stitch_cases()[STITCH_NAMES.index(name)]


def assert_stitch_same(got, ref, name):
    """got: Engine.debug_stitch's dict; ref: ref_stitch's list"""
    for f in ("dp", "mlen", "blen", "l_bi", "l_bj", "r_bi", "r_bj", "n_cigar"):
        want = np.array([r[f] for r in ref], np.int64)
        bad = np.flatnonzero(got[f].astype(np.int64) != want)
        assert len(bad) == 0, "%s: %s of chain %d is %d, the reference %d (%d chains differ)" % (name, f, bad[0], got[f][bad[0]], want[bad[0]], len(bad))
    for k, r in enumerate(ref):
        assert np.array_equal(got["cigars"][k], r["cigar"]), "%s: CIGAR of chain %d: %s, the reference %s" % (
            name, k, cigar_str(got["cigars"][k]), cigar_str(r["cigar"]))


def cigar_str(c, limit=40):
    s = "".join("%d%s" % (int(w) >> 4, "MID?"[min(int(w) & 0xf, 3)]) for w in c[:limit])
    return s + ("... (%d ops)" % len(c) if len(c) > limit else "")


# ---------------------------------------------------------------------------------------------------------------------
# from a problem list to the record's numbers, restated over the oracle's per-problem DP


def wide_row(row, mo):
    """the second-pass row of a flagged fill, or None when there is nothing to redo (k_retry_build's kind 4)"""
    m, n = int(row[4]), int(row[5])
    W, W2, dl = _fill_band(m, n, mo), _fill_band_wide(m, n, mo), n - m
    lo, hi = _even_lo(min(dl, 0) - W2), max(dl, 0) + W2
    if not (W2 > W and hi - lo + 1 <= DP_DMAX):
        return None
    r = np.array(row, np.int32)
    r[6], r[7], r[8] = lo, hi, 0
    return r


def oracle_dp(qs, ts, mo, rows, threads=8):
    """binding.debug_dp over chunks of the list on a few threads (the C call releases the GIL), cells included"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import binding as ob
    cut = np.linspace(0, len(rows), min(threads, max(1, len(rows) // 16)) + 1).astype(int)
    with ThreadPoolExecutor(len(cut) - 1) as ex:
        parts = list(ex.map(lambda k: ob.debug_dp(qs, ts, mo, rows[cut[k]:cut[k + 1]]), range(len(cut) - 1)))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("score", "bi", "bj", "touched", "cells")}
    out["cigars"] = [c for p in parts for c in p["cigars"]]
    return out


def ref_align(qs, ts, mo, chains, prob_off, rows):
    """-> dict: `chains` (per chain a dict qs, qe, ts, te, mlen, blen, dp_score, n_cigar, cigar), `probs` (dict of per-problem arrays
    cls, retried, score, bi, bj, mlen, mcols, nops, cells, and first: what the narrow pass alone gave as (score, cigar) for a problem
    that was redone, else None), n_retry"""
    rows = np.ascontiguousarray(rows, np.int32).reshape(-1, 12)
    chains = np.asarray(chains, np.int32).reshape(-1, 7)
    npb = len(rows)
    lim = Engine.dp_limits(mo)
    r1 = oracle_dp(qs, ts, mo, rows)
    steps = rows[:, 4].astype(np.int64) + rows[:, 5]
    flagged = (rows[:, 8] == 0) & (r1["touched"] != 0) & (steps <= ADAPT_MAX_STEPS)
    score, bi, bj, cells = (r1[f].astype(np.int64).copy() for f in ("score", "bi", "bj", "cells"))
    cig = list(r1["cigars"])
    first = [None] * npb
    redo = [(x, wide_row(rows[x], mo)) for x in np.flatnonzero(flagged)]
    redo = [(x, w) for x, w in redo if w is not None]
    if redo:
        r2 = oracle_dp(qs, ts, mo, np.array([w for _, w in redo], np.int32))
        for k, (x, _) in enumerate(redo):
            first[x] = (int(score[x]), cig[x])
            score[x], bi[x], bj[x], cig[x] = r2["score"][k], r2["bi"][k], r2["bj"][k], r2["cigars"][k]
            cells[x] += int(r2["cells"][k])
    P = dict(retried=flagged.astype(np.int64), score=score, bi=bi, bj=bj, cells=cells, first=first, cigars=cig,
             nops=np.array([len(c) for c in cig], np.int64), cls=np.zeros(npb, np.int64), mlen=np.zeros(npb, np.int64),
             mcols=np.array([sum(int(w) >> 4 for w in c if (int(w) & 0xf) == M) for c in cig], np.int64))
    views = []
    for x in range(npb):
        qa, ta = D._dp_view(qs, ts, rows[x])
        views.append((qa, ta))
        has_n = bool((qa == 4).any() or (ta == 4).any())
        P["cls"][x] = D.expect_class(int(rows[x, 8]), int(rows[x, 7]) - int(rows[x, 6]) + 1, int(steps[x]), lim, has_n)
        ml, ci, cj = D.mlen_of(cig[x], qa, ta)
        assert (ci, cj) == (int(bi[x]), int(bj[x])), "oracle: problem %d's CIGAR spans (%d, %d), its result says (%d, %d)" % (x, ci, cj, bi[x], bj[x])
        P["mlen"][x] = ml
    S = int(mo.cx_scale)
    out = []
    for k, (qid, tid, rev, cqs, cqe, crs, cre) in enumerate(tuple(int(v) for v in c) for c in chains):
        p0, p1 = int(prob_off[k]), int(prob_off[k + 1])
        qlen, tlen = len(qs[qid]), len(ts[tid])
        has_left, has_right = cqs > 0 and crs > 0, cqe < qlen and cre < tlen
        words, fq, ft = [], [], []                                  # the stitched CIGAR and the bases it walks, forwards on the chain's strand
        for x in range(p0, p1):
            left = x == p0 and has_left
            qa, ta = views[x]
            qa, ta = qa[:int(bi[x])], ta[:int(bj[x])]
            fq.append(qa[::-1] if left else qa)
            ft.append(ta[::-1] if left else ta)
            for w in (cig[x][::-1] if left else cig[x]):            # (the tap's CIGARs run start to end of the DP problem)
                w = int(w)
                if words and (words[-1] & 0xf) == (w & 0xf):
                    words[-1] += (w >> 4) << 4
                else:
                    words.append(w)
        q0, r0, q1, r1_ = cqs, crs, cqe, cre
        if has_left:
            q0, r0 = cqs - int(bi[p0]), crs - int(bj[p0])
        if has_right:
            q1, r1_ = cqe + int(bi[p1 - 1]), cre + int(bj[p1 - 1])
        mlen, ci, cj = D.mlen_of(words, np.concatenate(fq), np.concatenate(ft))
        assert ci == sum(len(a) for a in fq) and cj == sum(len(a) for a in ft)
        dp = int(score[p0:p1].sum())
        out.append(dict(qs=qlen - q1 if rev else q0, qe=qlen - q0 if rev else q1, ts=r0, te=r1_, mlen=mlen, blen=sum(w >> 4 for w in words),
                        dp_score=(dp + S // 2) // S if S > 0 else dp, score_sum=dp, n_cigar=len(words), cigar=np.array(words, np.uint32)))
    return dict(chains=out, probs=P, n_retry=int(flagged.sum()))


def account(rows, P, n_cls=N_DPCLS):
    """k_dp_account restated on per-problem columns (a tap's own output or the reference's): per class problems, cells, bi + bj and
    the byte formula; last the sum of the target windows' bases"""
    acc = np.zeros(n_cls * 4 + 1, np.int64)
    rows = np.asarray(rows).reshape(-1, 12)
    for x in range(len(rows)):
        c = 0 if int(rows[x, 8]) >= 3 else int(P["cls"][x])
        n = int(rows[x, 5])
        acc[c * 4] += 1
        acc[c * 4 + 1] += int(P["cells"][x])
        acc[c * 4 + 2] += int(P["bi"][x]) + int(P["bj"][x])
        acc[c * 4 + 3] += (int(P["bi"][x]) + n + 3) // 4 + 4 * int(P["nops"][x]) + 32
        acc[n_cls * 4] += n
    return acc


# ---- building align cases ----------------------------------------------------------------------------------------------


def formula_fill(rng, mo, cont, m, n, A=None, B=None, tag=""):
    """a fill with the band telr_map gives it (k_segments_w): narrow, or wide at once above ADAPT_MAX_STEPS"""
    W = _fill_band_wide(m, n, mo) if m + n > ADAPT_MAX_STEPS else _fill_band(m, n, mo)
    lo, hi = D.fill_band(m, n, W)
    kind = 0 if hi - lo + 1 <= DP_DMAX else 3
    if A is None:
        A, B = D.content(rng, cont, m, n)
    return D.Prob(kind, m, n, lo, hi, 0, A, B, None, tag)


def small_fill(rng, mo, cont="err", lo=20, hi=60, tag=""):
    m = int(rng.integers(lo, hi + 1))
    n = m if cont in ("match", "mismatch", "homopolymer") else max(8, m + int(rng.integers(-4, 5)))
    return formula_fill(rng, mo, cont, m, n, tag=tag)


def detour(rng, m, g, run):
    """equal-length windows whose best path leaves the main diagonal by g and comes back: g extra query bases, `run` matching bases
    g diagonals off, then g extra target bases.  With g beyond the narrow band the first pass has to stay at its edge."""
    n = m
    a = (m - 2 * g - run) // 2
    assert a >= 4
    core = D._rand(rng, m - g)                       # what both windows share
    A = np.concatenate([core[:a], D._rand(rng, g), core[a:]])
    B = np.concatenate([core[:a + run], D._rand(rng, g), core[a + run:]])
    assert len(A) == m and len(B) == n
    return A.astype(np.uint8), B.astype(np.uint8)


def touches(mo, p):
    """does the oracle's path of this fill come within fill_margin of its band's edge (what flags it for the second pass)"""
    from oracle import binding as ob
    r = ob.debug_dp([p.A.tobytes()], [p.B.tobytes()], mo, [(0, 0, 0, 0, p.m, p.n, p.dlo, p.dhi, p.kind, 1, 1, 0)])
    return bool(r["touched"][0])


def touching_fill(rng, mo, m, n, g, run, tag):
    """a fill with telr_map's band around a detour of g diagonals that the oracle's path touches the band's edge on"""
    for _ in range(100):
        A, B = detour(rng, m, g, run)
        if n > m:
            B = np.concatenate([B, D._rand(rng, n - m)])
        p = formula_fill(rng, mo, None, m, n, A, B, tag=tag)
        if touches(mo, p):
            return p
    raise AssertionError("no touching fill for m %d n %d g %d" % (m, n, g))


def retry_fill(rng, mo, m=None, tag="retry"):
    """a fill whose detour fits the wide band but not the narrow one"""
    m = int(rng.integers(64, 90)) if m is None else m
    W, W2 = _fill_band(m, m, mo), _fill_band_wide(m, m, mo)
    assert W2 > W + 8
    g = W + 6
    return touching_fill(rng, mo, m, m, g, min(m - 2 * g - 8, 6 * g), tag)


class Align:
    """chains added one by one, each on a query and a target of its own: [left extension] fills [right extension], a few random bases
    between the windows and around them.  Problems are dp_edges.Prob (A, B: the windows in DP order)."""

    def __init__(self, name, mo, seed=0):
        self.name, self.mo = name, mo
        self.rng = np.random.default_rng(seed)
        self.qs, self.ts, self.chains, self.prob_off, self.rows, self.tags = [], [], [], [0], [], []

    def chain(self, fills, left=None, right=None, rev=0, pad=True):
        rng, mo = self.rng, self.mo
        k = len(self.chains)
        fl = lambda hi: D._rand(rng, int(rng.integers(0, hi + 1)) if pad else 0)
        Q, T, plan = [], [], []                          # strand-local query, target, (prob, strand-local q, t of DP base 0)
        qn = tn = 0

        def put(a, b):
            nonlocal qn, tn
            Q.append(a); T.append(b)
            qn += len(a); tn += len(b)
        if left is not None:
            put(fl(9), fl(9))
            put(left.A[::-1], left.B[::-1])              # its DP runs down from the chain's start
            plan.append((left, qn - 1, tn - 1))
        else:
            none = np.zeros(0, np.uint8)                 # qs = 0 or rs = 0: no left extension
            put(*((none, fl(9)) if rng.random() < 0.5 else (fl(9), none)))
        cqs, crs = qn, tn
        for x, p in enumerate(fills):
            if x:
                put(fl(7), fl(7))
            plan.append((p, qn, tn))
            put(p.A, p.B)
        cqe, cre = qn, tn
        if right is not None:
            plan.append((right, qn, tn))
            put(right.A, right.B)
            put(D._rand(rng, 1 + int(rng.integers(0, 9))), D._rand(rng, 1 + int(rng.integers(0, 9))))
        else:
            none = np.zeros(0, np.uint8)                 # qe = qlen or re = tlen: no right extension
            put(*((none, fl(9)) if rng.random() < 0.5 else (fl(9), none)))
        Qs = np.concatenate(Q).astype(np.uint8)
        Tt = np.concatenate(T).astype(np.uint8)
        qlen = len(Qs)
        self.qs.append((D._COMP[Qs][::-1] if rev else Qs).tobytes())
        self.ts.append(Tt.tobytes())
        for p, lq, lt in plan:
            if p.kind == 1:
                row = (k, qlen - 1 - lq if rev else lq, k, lt, p.m, p.n, p.dlo, p.dhi, 1, 1 if rev else -1, -1, rev)
            else:
                row = (k, qlen - 1 - lq if rev else lq, k, lt, p.m, p.n, p.dlo, p.dhi, p.kind, -1 if rev else 1, 1, rev)
            self.rows.append(row)
            self.tags.append(p.tag)
        if right is not None:
            assert cqe < qlen and cre < len(Tt)
        else:
            assert cqe == qlen or cre == len(Tt)
        assert (left is not None) == (cqs > 0 and crs > 0)
        self.chains.append((k, k, rev, cqs, cqe, crs, cre))
        self.prob_off.append(len(self.rows))
        return self

    def done(self, reach, note=""):
        return dict(name=self.name, note=note, kind="align", mo=self.mo, qs=self.qs, ts=self.ts, chains=np.array(self.chains, np.int32).reshape(-1, 7),
                    prob_off=np.array(self.prob_off, np.int32), rows=np.array(self.rows, np.int32).reshape(-1, 12), tags=self.tags, reach=reach)


def ext(rng, mo, kind, cont, m=None, n=None, tag="ext"):
    if m is None:
        m = int(rng.integers(20, 61))
        n = m if cont in ("match", "mismatch") else max(8, m + int(rng.integers(-4, 5)))
    return D.extension(rng, mo, kind, cont, 0, m=m, n=min(n, m + mo.ext_band), tag=tag)


def _mo(name, **kw):
    mo = preset(name)[1]
    for k, v in kw.items():
        assert hasattr(mo, k), k
        setattr(mo, k, v)
    return mo


def _tagged(case, tag):
    return np.array([t == tag for t in case["tags"]])


FILL_COUNTS = (1, 63, 64, 65, 129)
RETRY_COUNTS = (0, 1, 63, 64, 65, 257)
ACCOUNT_COUNTS = (255, 256, 257)
_ALIGN = None


def align_cases():
    global _ALIGN
    if _ALIGN is not None:
        return _ALIGN
    C = []

    # 1. problem counts and merges
    mo = _mo("map-ont")
    b = Align("al_counts", mo, seed=101)
    rng = b.rng
    for F in FILL_COUNTS:
        for v, (l, r) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            b.chain([small_fill(rng, mo, "err" if x % 3 else "match") for x in range(F)], ext(rng, mo, 1, "err") if l else None,
                    ext(rng, mo, 2, "err") if r else None, rev=(v + F) & 1)
    b.chain([small_fill(rng, mo, "match", tag="exact") for _ in range(130)], rev=0)
    b.chain([small_fill(rng, mo, "match", tag="exact") for _ in range(130)], rev=1)

    def reach(ref, case):
        n = np.diff(case["prob_off"])
        assert set(n) >= {1, 2, 3, 63, 64, 65, 66, 67, 129, 130, 131}
        for k in (-1, -2):
            assert ref["chains"][k]["n_cigar"] == 1 and (int(ref["chains"][k]["cigar"][0]) & 0xf) == M
        assert set(int(c[2]) for c in case["chains"]) == {0, 1}
        assert max(c["n_cigar"] for c in ref["chains"]) > 129           # a CIGAR longer than its chain has problems: ops inside problems too
    C.append(b.done(reach, "1 .. 129 fills with and without either extension; 130 exact fills are one M"))

    # 2. extensions that come back empty
    b = Align("al_empty_ext", mo, seed=102)
    rng = b.rng
    fills = lambda n: [small_fill(rng, mo, "match") for _ in range(n)]
    b.chain(fills(3), ext(rng, mo, 1, "mismatch"), ext(rng, mo, 2, "err"), rev=0)
    b.chain(fills(3), ext(rng, mo, 1, "err"), ext(rng, mo, 2, "mismatch"), rev=1)
    b.chain(fills(3), ext(rng, mo, 1, "mismatch"), ext(rng, mo, 2, "mismatch"), rev=0)
    b.chain(fills(1), ext(rng, mo, 1, "mismatch"), ext(rng, mo, 2, "mismatch"), rev=1)
    b.chain(fills(2), ext(rng, mo, 1, "mismatch"), None, rev=1)
    b.chain(fills(2), None, ext(rng, mo, 2, "mismatch"), rev=0)

    def reach(ref, case):
        P = ref["probs"]
        o = case["prob_off"]
        empty = lambda x: P["nops"][x] == 0 and P["bi"][x] == 0 and P["bj"][x] == 0
        want = [(1, 0), (0, 1), (1, 1), (1, 1), (1, None), (None, 1)]
        for k, (l, r) in enumerate(want):
            if l is not None:
                assert bool(empty(o[k])) == bool(l), (k, "left")
            if r is not None:
                assert bool(empty(o[k + 1] - 1)) == bool(r), (k, "right")
        for k in (2, 3):                                 # nothing added at either end: the record's interval is the chain's
            _, _, rev, cqs, cqe, crs, cre = (int(v) for v in case["chains"][k])
            qlen = len(case["qs"][k])
            c = ref["chains"][k]
            assert (c["qs"], c["qe"]) == ((qlen - cqe, qlen - cqs) if rev else (cqs, cqe)) and (c["ts"], c["te"]) == (crs, cre)
        assert int(o[4] - o[3]) == 3
    C.append(b.done(reach, "left, right, both; one fill between two empty extensions"))

    # 3. the retry pass
    def retry_case(name, total, flagged_at, seed, mo=mo, per_chain=50, note=""):
        b = Align(name, mo, seed=seed)
        rng = b.rng
        probs = [retry_fill(rng, mo) if x in flagged_at else small_fill(rng, mo, "match", 24, 40, tag="plain") for x in range(total)]
        for a in range(0, total, per_chain):
            b.chain(probs[a:a + per_chain], rev=(a // per_chain) & 1)

        def reach(ref, case, flagged_at=flagged_at):
            P = ref["probs"]
            assert list(np.flatnonzero(P["retried"])) == sorted(flagged_at) and ref["n_retry"] == len(flagged_at)
            for x in flagged_at:                         # the second pass changed the alignment
                assert P["first"][x] is not None and P["first"][x][0] < P["score"][x] and not np.array_equal(P["first"][x][1], P["cigars"][x])
        return b.done(reach, note)
    for n in RETRY_COUNTS:
        C.append(retry_case("al_retry_%d" % n, max(n, 3), set(range(n)), 110 + n, note="%d problems on the retry list" % n))
    C.append(retry_case("al_retry_at_63_64_255_256", 300, {63, 64, 255, 256}, 120, note="flagged lanes at the wave and block edges of k_retry_collect"))
    C.append(retry_case("al_retry_lane_63_only", 130, {63}, 121, note="a wave whose only flagged lane is the last"))
    C.append(retry_case("al_retry_lane_0_of_block_1", 258, {256}, 122, note="the first lane of the second block alone"))

    b = Align("al_retry_steps_edge", mo, seed=123)
    rng = b.rng
    over = touching_fill(rng, mo, 500, 501, _fill_band_wide(500, 501, mo) - 1, 200, "1001")       # a detour along the edge of the wide band
    b.chain([retry_fill(rng, mo, 500, tag="1000"), small_fill(rng, mo, "match")], rev=0)
    b.chain([over, small_fill(rng, mo, "match")], rev=1)
    b.chain([retry_fill(rng, mo, 500, tag="1000")], rev=1)

    def reach(ref, case):
        P, rows = ref["probs"], case["rows"]
        a, o = _tagged(case, "1000"), _tagged(case, "1001")
        assert a.sum() == 2 and o.sum() == 1
        assert np.all(rows[a, 4] + rows[a, 5] == 1000) and np.all(P["retried"][a] == 1) and all(P["first"][x] is not None for x in np.flatnonzero(a))
        x = int(np.flatnonzero(o)[0])
        assert rows[x, 4] + rows[x, 5] == 1001 and P["retried"][x] == 0 and P["first"][x] is None
        assert rows[x, 7] - max(0, rows[x, 5] - rows[x, 4]) == _fill_band_wide(500, 501, case["mo"]) > _fill_band(500, 501, case["mo"])
        from oracle import binding as ob
        assert ob.debug_dp(case["qs"], case["ts"], case["mo"], rows[x:x + 1])["touched"][0] == 1      # it would have been flagged
    C.append(b.done(reach, "m + n = 1000 is redone, 1001 has the wide band at once and is not"))

    mo_nb = _mo("map-ont", bw=_fill_band(70, 70, mo))
    b = Align("al_retry_nothing_to_redo", mo_nb, seed=124)
    rng = b.rng
    for k in range(3):
        b.chain([small_fill(rng, mo_nb, "match"), touching_fill(rng, mo_nb, 70 + k, 70 + k, 11, 30, "kind4"), small_fill(rng, mo_nb, "err")], rev=k & 1)

    def reach(ref, case):
        P, t = ref["probs"], _tagged(case, "kind4")
        for x in np.flatnonzero(t):
            m, n = int(case["rows"][x, 4]), int(case["rows"][x, 5])
            assert _fill_band_wide(m, n, case["mo"]) == _fill_band(m, n, case["mo"]) == case["mo"].bw
            assert P["retried"][x] == 1 and P["first"][x] is None and wide_row(case["rows"][x], case["mo"]) is None
        assert ref["n_retry"] >= 3
    C.append(b.done(reach, "bw so small that W2 == W: flagged, on the list, kind 4, the first result stands"))

    b = Align("al_retry_class_change", mo, seed=125)
    p = retry_fill(b.rng, mo, 80)
    b.chain([p], rev=0)
    W2 = _fill_band_wide(80, 80, mo)
    lo, hi = D.fill_band(80, 80, W2)
    b.chain([D.Prob(0, 80, 80, lo, hi, 0, p.A, p.B, None, "wide")], rev=0)        # the wide row alone, on a copy of the sequences

    def reach(ref, case):
        P = ref["probs"]
        assert P["retried"][0] == 1 and P["first"][0] is not None and P["retried"][1] == 0
        assert np.array_equal(wide_row(case["rows"][0], case["mo"])[4:9], case["rows"][1][4:9])
        assert P["cls"][0] != P["cls"][1]                # (the tap reports the class of the FIRST pass; the second row is the retry's)
        assert P["score"][0] == P["score"][1] and np.array_equal(P["cigars"][0], P["cigars"][1])
    C.append(b.done(reach, "the retry runs in another DP class than the first pass"))

    # 4. mcols / blen in every DP class
    C.extend(class_cases())

    # 5. convex cost
    for name in ("ngmlr-ont", "ngmlr-pacbio"):
        cmo = _mo(name)
        b = Align("al_convex_" + name, cmo, seed=130 + len(name))
        rng = b.rng
        for k in range(48):
            cont = ("err", "mismatch", "match", "bandedge", "tandem", "homopolymer")[k % 6]
            F = (1, 2, 3, 70)[k % 4] if k < 40 else 1
            fills = [small_fill(rng, cmo, cont if x % 2 == 0 else "err", 8 if cont == "mismatch" else 20, 14 if cont == "mismatch" else 60) for x in range(F)]
            b.chain(fills, ext(rng, cmo, 1, "err") if k % 3 == 0 else None, ext(rng, cmo, 2, "err") if k % 5 == 0 else None, rev=k & 1)

        def reach(ref, case):
            S = int(case["mo"].cx_scale)
            assert S >= 2
            sums = np.array([c["score_sum"] for c in ref["chains"]])
            res = sums % S
            assert (sums > 0).any() and (sums < 0).any()
            for sign in (sums > 0, sums < 0):            # on either side of zero: rounded down, rounded up
                assert ((res > 0) & (res < S // 2) & sign).any() and ((res >= S // 2) & sign).any(), sorted(zip(sums, res))
        C.append(b.done(reach, "the records' scores come back from 1/S units, rounding included"))

    # 6. accounts
    for n in ACCOUNT_COUNTS:
        b = Align("al_accounts_%d" % n, mo, seed=140 + n)
        rng = b.rng
        left = n
        while left:
            F = min(left, int(rng.integers(1, 40)))
            l = ext(rng, mo, 1, "err", tag="x") if left - F >= 2 and rng.random() < 0.5 else None
            r = ext(rng, mo, 2, "err", tag="x") if left - F - (l is not None) >= 1 and rng.random() < 0.5 else None
            b.chain([small_fill(rng, mo, ("err", "match", "bandedge")[x % 3], 12, 40) for x in range(F)], l, r, rev=int(rng.integers(0, 2)))
            left -= F + (l is not None) + (r is not None)

        def reach(ref, case, n=n):
            assert len(case["rows"]) == n and len(set(ref["probs"]["cls"])) >= 2
        C.append(b.done(reach, "%d problems in the call: k_dp_account's last block" % n))

    assert tuple(c["name"] for c in C) == ALIGN_NAMES
    _ALIGN = C
    return C


def align_case(name):
    return align_cases()[ALIGN_NAMES.index(name)]


def class_cases():
    """chains that hold a problem of every DP class: map-ont reaches all but the wider extension classes, three extension bands of
    dp_edges.scoring_sets() the rest"""
    want = set(range(N_DPCLS))
    seen, out = set(), []
    sets = {name: mo for name, mo, _ in D.scoring_sets()}
    for name in ("map-ont", "ext63-z400", "ext127-z400", "ext511-z400"):
        mo = sets[name]
        lim = Engine.dp_limits(mo)
        b = Align("al_classes_" + name, mo, seed=150 + len(out))
        rng = b.rng
        probs = []
        if name == "map-ont":
            for Dw in sorted(set(D.UPPER_D.values())):
                if Dw <= DP_DMAX:
                    probs.append(D.fill(rng, Dw, "err", 0, tag="D%d" % Dw))
                    probs.append(D.fill(rng, Dw, "bandedge", 0, tag="D%d" % Dw))
            for Dw in D.PACKED_FILL_D + D.WIDE_FILL_D:                   # an N takes a fill out of the packed classes
                probs.append(D.fill(rng, Dw, "err", 0, tag="N"))
                probs[-1].B[probs[-1].n // 2] = ord("N")
            probs.append(D.fill(rng, 2000, "err", 0, tag="D2000"))
            probs.append(D.fill(rng, DP_DMAX + 1, "err", 0, tag="kind3"))
            probs.append(D.fill(rng, DP_DMAX + 1, "bandedge", 0, tag="kind3"))
            for ins in (True, False):
                probs.append(D.longgap(rng, mo, 0, ins, "err"))
            # the nibble cell and the tag8 cell on both sides of their step bounds
            for key, Ds in (("tb4_steps", (16, 20)), ("tag8_steps", (24, 64, 128))):
                L = lim[key]
                if L and L + 2 <= 6000:
                    for Dw in Ds:
                        for steps in (min(L, 400), L + 1):
                            probs.append(D.fill_steps(rng, Dw, steps, "err", 0, tag="%s:%d" % (key, steps)))
        exts = []
        for cont in ("err", "nrich", "match"):
            for kind in (1, 2):
                m = int(rng.integers(60, 200))
                e = D.extension(rng, mo, kind, "err" if cont == "nrich" else cont, 0, m=m, n=min(int(rng.integers(60, 200)), m + mo.ext_band), tag="ext")
                if cont == "nrich":
                    e.A[e.m // 2] = ord("N")
                exts.append(e)
        if not probs:
            probs = [small_fill(rng, mo, "err") for _ in range(6)]
        # every chain: [left] two of the problems [right]
        k = 0
        pairs = [(exts[i], exts[i + 1]) for i in range(0, len(exts), 2)]
        for a in range(0, len(probs), 2):
            l, r = pairs[k % len(pairs)] if k < 2 * len(pairs) else (None, None)
            if l is not None:
                l, r = _copy(l), _copy(r)
            b.chain(probs[a:a + 2], l, r, rev=k & 1)
            k += 1
        case = b.done(None, "one problem at least of every class the set reaches")
        cls = _classes_of(case, lim)
        new = set(cls) - seen
        seen |= set(cls)

        def reach(ref, case, new=frozenset(new)):
            got = set(int(c) for c in ref["probs"]["cls"])
            assert new <= got, sorted(new - got)
            kinds = set(int(v) for v in case["rows"][:, 8])
            if case["name"] == "al_classes_map-ont":
                assert {0, 1, 2, 3, 5} <= kinds
                lim = Engine.dp_limits(case["mo"])
                steps = case["rows"][:, 4] + case["rows"][:, 5]
                P = ref["probs"]
                for c, bit in ((17, 1), (10, 2)):        # the nibble cell: the class's problems of at most tb4_steps steps
                    if lim["tb4_mask"] & bit:
                        assert ((P["cls"] == c) & (steps <= lim["tb4_steps"])).any()
                if lim["tag8_steps"]:
                    two = np.isin(P["cls"], (11, 12, 13, 14, 15, 16, 22))
                    assert (two & (steps <= lim["tag8_steps"])).any() and (two & (steps > lim["tag8_steps"])).any()
                assert set(D.INTERLEAVED) <= got
            # M columns and gaps both: mcols is not bi, not bj, not blen
            P = ref["probs"]
            assert ((P["mcols"] < P["bi"]) & (P["mcols"] < P["bj"]) & (P["mcols"] > 0)).any()
        case["reach"] = reach
        out.append(case)
    assert seen >= want, "classes without a problem: %s" % sorted(want - seen)
    return out


def _copy(p):
    return D.Prob(p.kind, p.m, p.n, p.dlo, p.dhi, p.strand, p.A.copy(), p.B.copy(), p.npos, p.tag)


def _classes_of(case, lim):
    out = []
    for row in case["rows"]:
        qa, ta = D._dp_view(case["qs"], case["ts"], row)
        out.append(D.expect_class(int(row[8]), int(row[7]) - int(row[6]) + 1, int(row[4]) + int(row[5]), lim, bool((qa == 4).any() or (ta == 4).any())))
    return out


_REF = {}


def ref_of(case):
    """the reference's output of a case, computed once"""
    if case["name"] not in _REF:
        _REF[case["name"]] = ref_stitch(case, trace=True) if case["kind"] == "stitch" else \
            ref_align(case["qs"], case["ts"], case["mo"], case["chains"], case["prob_off"], case["rows"])
    return _REF[case["name"]]


CHAIN_FIELDS = ("qs", "qe", "ts", "te", "mlen", "blen", "dp_score", "n_cigar")
PROB_FIELDS = ("cls", "retried", "score", "bi", "bj", "mlen", "mcols", "nops", "cells")


def assert_align_same(got, ref, name):
    """got: Engine.debug_align's dict; ref: ref_align's"""
    assert got["n_retry"] == ref["n_retry"], "%s: %d problems on the retry list, the reference %d" % (name, got["n_retry"], ref["n_retry"])
    for f in PROB_FIELDS:
        a, w = got["probs"][f].astype(np.int64), np.asarray(ref["probs"][f], np.int64)
        bad = np.flatnonzero(a != w)
        assert len(bad) == 0, "%s: %s of problem %d is %d, the reference %d (%d problems differ)" % (name, f, bad[0], a[bad[0]], w[bad[0]], len(bad))
    for f in CHAIN_FIELDS:
        a, w = got["chains"][f].astype(np.int64), np.array([c[f] for c in ref["chains"]], np.int64)
        bad = np.flatnonzero(a != w)
        assert len(bad) == 0, "%s: %s of chain %d is %d, the reference %d (%d chains differ)" % (name, f, bad[0], a[bad[0]], w[bad[0]], len(bad))
    for k, c in enumerate(ref["chains"]):
        assert np.array_equal(got["cigars"][k], c["cigar"]), "%s: CIGAR of chain %d: %s, the reference %s" % (
            name, k, cigar_str(got["cigars"][k]), cigar_str(c["cigar"]))
