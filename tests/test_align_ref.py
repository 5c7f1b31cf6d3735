"""The references tests/test_gpu_align_edges.py holds the engine's stitch and align taps to, checked on the CPU: ref_stitch gives the
hand-derived results of a few chains written out here; ref_align -- the oracle's per-problem DP (tor_debug_dp) with the retry rule,
the stitching and the sums restated in Python -- reproduces the records of the oracle's own align_chain on mapped reads; and every
case of tests/align_edges.py reaches the edge it is built for, computed from the references alone."""
import numpy as np
import pytest

from telr_amd._abi import MF_CIGAR
from telr_amd.presets import preset
import align_edges as E
import backtrack_edges as B
import dp_edges as D

STITCH, ALIGN = E.STITCH_NAMES, E.ALIGN_NAMES
M, I, DEL, op = E.M, E.I, E.DEL, E.op


def _case(chains, cx_scale=0):
    """chains: [(has_left, [(score, bi, bj, mlen, mcols, [stored words])])]"""
    p_off, prob, cigars = [0], [], []
    for _, ps in chains:
        for p in ps:
            prob.append(p[:5]); cigars.append(np.array(p[5], np.uint32))
        p_off.append(len(prob))
    return dict(cx_scale=cx_scale, p_off=p_off, has_left=[hl for hl, _ in chains], prob=prob, cigars=cigars)


def test_ref_stitch_on_hand_derived_chains():
    # storage order is end to start of the DP problem.  Chain 0: a left extension stored 5M 2I 7M reads 5M 2I 7M; the fill stored
    # 4M 3D reads 3D 4M; the right extension stored 2I 6M reads 6M 2I: 5M 2I 7M 3D 10M 2I.
    c0 = (1, [(10, 14, 12, 11, 12, [op(5, M), op(2, I), op(7, M)]), (-3, 4, 7, 4, 4, [op(4, M), op(3, DEL)]), (7, 8, 6, 5, 6, [op(2, I), op(6, M)])])
    # chain 1: the same words without a left extension: the first problem reads 7M 2I 5M, and 5M + 3D do not merge
    c1 = (0, [c0[1][0], c0[1][1]])
    # chain 2: one-op problems fold into the first; the empty problems (an extension with bi = bj = 0, a fill without ops that
    # still has bi, bj) are skipped by the CIGAR and not by the sums
    c2 = (1, [(0, 0, 0, 0, 0, []), (5, 3, 3, 2, 3, [op(3, M)]), (1, 2, 1, 0, 0, []), (6, 4, 4, 4, 4, [op(4, M)]), (-20, 9, 2, 2, 2, [op(2, M), op(7, I)]),
              (0, 0, 0, 0, 0, [])])
    ref = E.ref_stitch(_case([c0, c1, c2]), trace=True)
    assert [E.cigar_str(r["cigar"]) for r in ref] == ["5M2I7M3D10M2I", "7M2I5M3D4M", "7M7I2M"]
    assert [(r["dp"], r["mlen"], r["blen"]) for r in ref] == [(14, 20, 14 + 12 - 12 + 4 + 7 - 4 + 8 + 6 - 6), (7, 15, 21), (-8, 8, 0 + 3 + (2 + 1) + 4 + (9 + 2 - 2) + 0)]
    assert [(r["l_bi"], r["l_bj"], r["r_bi"], r["r_bj"]) for r in ref] == [(14, 12, 8, 6), (14, 12, 4, 7), (0, 0, 0, 0)]
    assert ref[0]["skips"] == [2] and ref[0]["gone"] == [] and ref[2]["skips"] == [3] and ref[2]["gone"] == [3]
    # blen of consistent problems is the length of the stitched CIGAR
    assert ref[0]["blen"] == sum(int(w) >> 4 for w in ref[0]["cigar"]) == 29


def test_ref_stitch_rounds_convex_scores_down_to_the_floor():
    for S, sums, want in ((10, (-16, -15, -6, -5, -1, 0, 4, 5, 14, 15, 20), (-2, -1, -1, 0, 0, 0, 0, 1, 1, 2, 2)),
                          (20, (-31, -30, -11, -10, 9, 10, 29, 30, 400), (-2, -1, -1, 0, 0, 1, 1, 2, 20))):
        ref = E.ref_stitch(_case([(0, [(a, 1, 1, 1, 1, [op(1, M)]), (s - a, 1, 1, 1, 1, [op(1, M)])]) for s in sums for a in (0, 7)], cx_scale=S))
        assert [r["dp"] for r in ref] == [w for w in want for _ in range(2)]
    ref = E.ref_stitch(_case([(0, [(-7, 1, 1, 1, 1, [op(1, M)])])], cx_scale=0))
    assert ref[0]["dp"] == -7


@pytest.mark.parametrize("name", STITCH)
def test_stitch_case_reaches_its_edge(name):
    case = E.stitch_case(name)
    case["reach"](E.ref_of(case), case)
    # the problems' numbers are those of their ops: blen is the length of the CIGAR unless an empty problem brings bi, bj of its own
    for k, r in enumerate(E.ref_of(case)):
        p0, p1 = case["p_off"][k], case["p_off"][k + 1]
        loose = sum(int(case["prob"][x][1]) + int(case["prob"][x][2]) for x in range(p0, p1) if len(case["cigars"][x]) == 0)
        assert r["blen"] - loose == sum(int(w) >> 4 for w in r["cigar"])


@pytest.mark.parametrize("name", ALIGN)
def test_align_case_reaches_its_edge(name):
    case = E.align_case(name)
    ref = E.ref_of(case)
    case["reach"](ref, case)
    # what the engine derives from per-problem numbers, the reference recounts from the final CIGAR: the two agree on the oracle
    P, o = ref["probs"], case["prob_off"]
    for k, c in enumerate(ref["chains"]):
        sl = slice(int(o[k]), int(o[k + 1]))
        assert c["blen"] == int((P["bi"][sl] + P["bj"][sl] - P["mcols"][sl]).sum()) and c["mlen"] == int(P["mlen"][sl].sum())
    assert np.all(P["cells"][case["rows"][:, 8] < 3] > 0)


def test_every_listed_edge_has_a_case():
    st = E.stitch_cases()
    per_chain = np.concatenate([np.diff(c["p_off"]) for c in st])
    assert set(E.STITCH_P) | {130} <= set(per_chain)
    assert {1, 2, 300} <= set(len(c["has_left"]) for c in st) and set(E.CX_SCALES) == set(c["cx_scale"] for c in st)
    assert set(E.OPCOUNTS) <= set(len(w) for c in st for w in c["cigars"])
    assert all(set(c["has_left"]) == {0, 1} for c in st if len(c["has_left"]) > 2)
    al = E.align_cases()
    assert set(E.RETRY_COUNTS) <= set(E.ref_of(c)["n_retry"] for c in al)
    assert set(E.ACCOUNT_COUNTS) <= set(len(c["rows"]) for c in al)
    seen = set()
    for c in al:
        seen |= set(int(v) for v in E.ref_of(c)["probs"]["cls"])
    assert seen == set(range(E.N_DPCLS))
    fills = np.concatenate([[int((c["rows"][a:b, 8] != 1).sum() - (c["rows"][a:b, 8] == 2).sum()) for a, b in zip(c["prob_off"], c["prob_off"][1:])] for c in al])
    assert set(E.FILL_COUNTS) | {130} <= set(fills)
    assert {10, 20} <= set(int(c["mo"].cx_scale) for c in al)


# ---- ref_align against the oracle's own align_chain --------------------------------------------------------------------------


def _reads(seed, n_reads=36):
    rng = np.random.default_rng(seed)
    ts = [D._rand(rng, 24000), D._rand(rng, 9000)]
    qs = []
    for k in range(n_reads):
        t = ts[k % 2]
        ln = int(rng.integers(500, 2600))
        a = int(rng.integers(0, len(t) - ln)) if k % 7 else (0 if k % 14 else len(t) - ln)        # some reads reach a target's end
        q = D._mutate(rng, t[a:a + ln], float(rng.uniform(0.03, 0.12)))
        if k % 5 == 0:                                   # an insertion the chain has to bridge or break at
            c = len(q) // 2
            q = np.concatenate([q[:c], D._rand(rng, int(rng.integers(30, 400))), q[c:]])
        if k % 3 == 0:                                   # soft ends: the extensions stop inside the read
            q = np.concatenate([D._rand(rng, int(rng.integers(5, 80))), q, D._rand(rng, int(rng.integers(5, 80)))])
        if k & 1:
            q = D._COMP[q][::-1]
        qs.append(np.ascontiguousarray(q).tobytes())
    return qs, [t.tobytes() for t in ts]


@pytest.mark.parametrize("name", ["map-ont", "ngmlr-ont", "ngmlr-pacbio"])
def test_ref_align_reproduces_the_oracles_records(name):
    from oracle import binding as ob
    io, mo = preset(name)
    assert mo.flags & MF_CIGAR
    qs, ts = _reads(7 + len(name))
    o = ob.OracleIndex(ts, io).map(qs, mo, debug=True)
    goff, tlen = B.targets([len(t) for t in ts])
    bt = ob.debug_backtrack(o["anchors"], o["anchor_off"].astype(np.int32), o["f"], o["p"], np.array([len(q) for q in qs], np.int32), goff, tlen, mo)
    kept = bt["kept"]
    keys = [tuple(int(v) for v in kept[k, (0, 4, 1, 2, 3)]) for k in range(len(kept))]
    alns = o["alns"]
    assert len(alns) >= 30
    # the kept chains the records came from, by (query, target, chain score, anchors, strand); ambiguous ones are left out
    pick, recs = [], []
    for r in alns:
        key = (int(r["qid"]), int(r["tid"]), int(r["score"]), int(r["cnt"]), 1 if int(r["flags"]) & 8 else 0)
        if keys.count(key) == 1:
            pick.append(keys.index(key)); recs.append(r)
    assert len(pick) >= len(alns) - 2
    chains = kept[pick][:, (0, 4, 3, 7, 8, 5, 6)]         # {qid, tid, rev, qs, qe, rs, re}
    rows = np.concatenate([bt["probs"][bt["prob_off"][k]:bt["prob_off"][k + 1]] for k in pick])
    prob_off = np.concatenate([[0], np.cumsum([bt["prob_off"][k + 1] - bt["prob_off"][k] for k in pick])])
    ref = E.ref_align(qs, ts, mo, chains, prob_off, rows)
    for r, c in zip(recs, ref["chains"]):
        want = tuple(int(r[f]) for f in ("qs", "qe", "ts", "te", "mlen", "blen", "dp_score", "n_cigar"))
        assert tuple(c[f] for f in E.CHAIN_FIELDS) == want, (name, int(r["qid"]))
        assert np.array_equal(c["cigar"], o["cigars"][int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])])
    # the reads gave the reference something to do
    kinds = set(int(v) for v in rows[:, 8])
    assert {0, 1, 2} <= kinds and ref["n_retry"] > 0 and set(int(v) for v in chains[:, 2]) == {0, 1}
    assert any(P is not None for P in ref["probs"]["first"])
    # and the oracle's counters are the sums of the per-problem columns over ALL kept chains' problems
    if len(pick) == len(kept):
        assert int(ref["probs"]["cells"].sum()) == o["counters"]["dp_cells"] and len(rows) == o["counters"]["dp_problems"]
