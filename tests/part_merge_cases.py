"""Cases of the multi-part merge, shared by tests/test_part_merge_ref.py (the plain-Python definition against answers
derived by hand) and tests/test_gpu_part_index.py (telr_merge_parts against the definition, bit for bit), and the two small genomes of
the split-against-unsplit experiments.

A case: name, parts = [(alns, cigars)], tid_maps, n_queries, opt (overrides of the map-ont options), and -- hand cases only -- expect =
the merged records as (qid, part, rank, class, parent, subsc, n_sub) tuples in output order."""
import numpy as np

import part_merge_ref as ref
from telr_amd import synth
from telr_amd._abi import ALN_DTYPE, MF_CIGAR
from telr_amd.presets import preset

P, S, U, R = ref.F_PRIMARY, ref.F_SECONDARY, ref.F_SUPPL, ref.F_REV
QLEN = 20000


def options(**kw):
    _, mo = preset("map-ont")
    mo = mo.copy()
    mo.flags |= MF_CIGAR
    for k, v in kw.items():
        setattr(mo, k, v)
    return mo


def rec(qid, qs, qe, dp, flags=P, parent=0, score=None, subsc=0, n_sub=0, tid=0, n_cigar=0):
    r = np.zeros((), ALN_DTYPE)
    r["qid"], r["tid"], r["qlen"], r["qs"], r["qe"] = qid, tid, QLEN, qs, qe
    r["tlen"], r["ts"], r["te"] = 50000, 100 + qs, 100 + qe
    r["mlen"], r["blen"] = max(0, qe - qs - 7), qe - qs + 5
    r["score"] = dp - 11 if score is None else score
    r["dp_score"], r["cnt"], r["subsc"], r["n_sub"], r["parent"], r["flags"], r["n_cigar"] = dp, 23, subsc, n_sub, parent, flags, n_cigar
    r["mapq"] = 17                                       # (every kept record's is computed afresh)
    return r


def part(recs, rng=None, lead=0, gap=0):
    """records -> (alns, cigars): every record's n_cigar words placed behind `lead` unreferenced words, `gap` more between records"""
    rng = np.random.default_rng(len(recs) + lead) if rng is None else rng
    alns = np.array(recs, dtype=ALN_DTYPE) if len(recs) else np.zeros(0, ALN_DTYPE)
    off = lead
    for a in alns:
        a["cigar_off"] = off
        off += int(a["n_cigar"]) + gap
    return alns, rng.integers(0, 1 << 32, size=off + 3, dtype=np.uint64).astype(np.uint32)


def case(name, parts, n_queries, expect=None, tid_maps=None, **opt):
    if tid_maps is None:                                   # part p holds the global targets 2p, 2p + 1
        tid_maps = [np.array([2 * p, 2 * p + 1], np.int32) for p in range(len(parts))]
    return dict(name=name, parts=parts, tid_maps=tid_maps, n_queries=n_queries, opt=opt, expect=expect)


def signature(c, alns):
    """the merged records of case c as (qid, part, rank, class, parent, subsc, n_sub): part and rank read off (tid, ts, dp_score, qs, qe)"""
    where = {}
    for p, (a, _) in enumerate(c["parts"]):
        rank, last = 0, -1
        for r in a:
            rank = rank + 1 if r["qid"] == last else 0
            last = r["qid"]
            key = (int(r["qid"]), int(c["tid_maps"][p][r["tid"]]), int(r["qs"]), int(r["qe"]), int(r["dp_score"]), int(r["score"]))
            assert key not in where, "hand cases keep their records distinguishable"
            where[key] = (p, rank)
    return [(int(r["qid"]),) + where[(int(r["qid"]), int(r["tid"]), int(r["qs"]), int(r["qe"]), int(r["dp_score"]), int(r["score"]))] +
            (int(r["flags"]) & ref.CLASS, int(r["parent"]), int(r["subsc"]), int(r["n_sub"])) for r in alns]


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------
# 0.8f = 0.800000011920929; (float)1000 * 0.8f = 800.0000119 rounds to 800.0 in float32: a secondary of 800 is kept (>=), one of 799 is not
HAND = [
    case("overlapping primaries, the worse one kept at pri_ratio exactly",
         [part([rec(0, 100, 3100, 1000, n_cigar=3)], lead=1), part([rec(0, 200, 3000, 800, flags=P | R, n_cigar=2)], lead=3)], 1,
         expect=[(0, 0, 0, P, 0, 789, 1), (0, 1, 0, S, 0, 0, 0)], pri_ratio=0.8),
    case("overlapping primaries, the worse one dropped one below pri_ratio",
         [part([rec(0, 100, 3100, 1000, n_cigar=3)], lead=1), part([rec(0, 200, 3000, 799, n_cigar=2)], lead=3)], 1,
         expect=[(0, 0, 0, P, 0, 788, 1)], pri_ratio=0.8),
    case("the worse one in the FIRST part",
         [part([rec(0, 200, 3000, 900, n_cigar=2)]), part([rec(0, 100, 3100, 1000, n_cigar=3)])], 1,
         expect=[(0, 1, 0, P, 0, 889, 1), (0, 0, 0, S, 0, 0, 0)]),
    case("best_n cuts the third and fourth secondary",
         [part([rec(0, 0, 2000, 1000), rec(0, 10, 1990, 990, flags=S)]), part([rec(0, 20, 1980, 995), rec(0, 30, 1970, 985, flags=U, parent=1)]),
          part([rec(0, 40, 1960, 980)])], 1,
         expect=[(0, 0, 0, P, 0, 984, 3), (0, 1, 0, S, 0, 0, 0), (0, 0, 1, S, 0, 0, 0)], best_n=2, tid_maps=[np.array([0], np.int32)] * 3),
    case("disjoint primaries: PRIMARY + SUPPL",
         [part([rec(0, 0, 2000, 700, flags=P | R, subsc=50, n_sub=2)]), part([rec(0, 2000, 5000, 900, subsc=40, n_sub=1)])], 1,
         expect=[(0, 1, 0, P, 0, 40, 1), (0, 0, 0, U, 1, 50, 2)]),
    case("a tie in dp_score: part, then rank",
         [part([rec(0, 0, 1000, 500, score=401), rec(0, 5000, 6000, 500, flags=U, parent=1, score=402)]),
          part([rec(0, 10, 1010, 500, score=403), rec(0, 5010, 6010, 500, flags=U, parent=1, score=404)])], 1,
         expect=[(0, 0, 0, P, 0, 403, 1), (0, 0, 1, U, 1, 404, 1), (0, 1, 0, S, 0, 0, 0), (0, 1, 1, S, 1, 0, 0)]),
    # A (part 0) counted its secondary B there: subsc 777 (B's score), n_sub 1.  C (part 1) adds one; B does not count again.
    case("no double count: the part's own secondary is in what the primary had",
         [part([rec(0, 0, 3000, 1000, subsc=777, n_sub=1), rec(0, 50, 2950, 950, flags=S, parent=0, score=777)]), part([rec(0, 100, 2900, 900, score=600)])], 1,
         expect=[(0, 0, 0, P, 0, 777, 2), (0, 0, 1, S, 0, 0, 0), (0, 1, 0, S, 0, 0, 0)]),
    # D (part 1) outranks A: A becomes D's secondary and B's first own parent is now D, another part's: both count for D
    case("no double count, the converse: a better record of another part takes both",
         [part([rec(0, 0, 3000, 1000, subsc=777, n_sub=1), rec(0, 50, 2950, 950, flags=S, parent=0, score=777)]), part([rec(0, 100, 2900, 1100, score=1200)])], 1,
         expect=[(0, 1, 0, P, 0, 989, 2), (0, 0, 0, S, 0, 0, 0), (0, 0, 1, S, 0, 0, 0)]),
    # the secondary's part-level parent has rank 1, its parent here has rank 0: same part, but not the one that counted it
    case("no double count applies to the part-level parent only",
         [part([rec(0, 0, 3000, 1000, subsc=0, n_sub=0), rec(0, 2000, 6000, 900, flags=U, parent=1, subsc=333, n_sub=1),
                rec(0, 2500, 3000, 800, flags=S, parent=1, score=333)])], 1,
         expect=[(0, 0, 0, P, 0, 333, 1), (0, 0, 1, U, 1, 333, 1), (0, 0, 2, S, 0, 0, 0)], tid_maps=[np.array([0], np.int32)]),
    case("secondary = 0",
         [part([rec(0, 100, 3100, 1000)]), part([rec(0, 200, 3000, 990)])], 1, expect=[(0, 0, 0, P, 0, 979, 1)], secondary=0),
    case("queries with records in one part only, and with none",
         [part([rec(0, 0, 1000, 500, n_cigar=4), rec(3, 0, 1000, 400, n_cigar=1)], lead=5), part([rec(1, 0, 900, 300, n_cigar=5), rec(3, 10, 990, 450, n_cigar=0)], lead=2)], 5,
         expect=[(0, 0, 0, P, 0, 0, 0), (1, 1, 0, P, 0, 0, 0), (3, 1, 0, P, 0, 389, 1), (3, 0, 0, S, 0, 0, 0)]),
]


# ---- where the kernels can go wrong -----------------------------------------------------------------------------------------------------
def _raw_pool(rng, qid, n, n_cigars):
    """n records of one query: short intervals in a few clumps, scores from a small set (ties), CIGAR lengths from n_cigars in turn"""
    out = []
    for i in range(n):
        c = int(rng.integers(0, 12)) * 1500
        s = c + int(rng.integers(0, 900)); ln = int(rng.integers(40, 700))
        out.append(rec(qid, s, min(QLEN, s + ln), int(rng.choice([300, 320, 320, 350, 400, 400, 520, 800])) + int(rng.integers(0, 3)),
                       flags=P | (R if rng.integers(0, 2) else 0), score=int(rng.integers(100, 900)), tid=int(rng.integers(0, 2)),
                       n_cigar=int(n_cigars[(qid + i) % len(n_cigars)])))
    return out


def _selected(recs_by_q, n_queries, mo):
    """a part as a map call would leave it: the definition itself applied to the raw records of ONE part"""
    raw = [r for q in sorted(recs_by_q) for r in recs_by_q[q]]
    for q in recs_by_q:
        for i, r in enumerate(recs_by_q[q]):
            r["parent"] = i
    alns, _ = ref.merge([part(raw)], [np.arange(2, dtype=np.int32)], n_queries, mo)
    return list(alns)


def pooled(name, pools, n_parts, n_cigars=(0, 1, 3, 4, 5), seed=1, lead=(1, 3, 6), empty_part=None, **opt):
    """pools[q] = the number of pooled records of query q, dealt to the parts in turn"""
    rng = np.random.default_rng(seed)
    mo = options(best_n=1000, **{k: v for k, v in opt.items() if k != "best_n"})          # parts that keep every secondary within pri_ratio
    by_part = [dict() for _ in range(n_parts)]
    live = [p for p in range(n_parts) if p != empty_part]
    for q, n in enumerate(pools):
        raw = _raw_pool(rng, q, n, n_cigars)
        for i, r in enumerate(raw):
            by_part[live[i % len(live)]].setdefault(q, []).append(r)
    parts = [part(_selected(by_part[p], len(pools), mo), rng=rng, lead=lead[p % len(lead)], gap=p) for p in range(n_parts)]
    return case(name, parts, len(pools), **opt)


EDGE = [
    pooled("pools of 0 1 2 63 64 65 130, two parts", [0, 1, 2, 63, 64, 65, 130, 0], 2, best_n=5),
    pooled("pools of 0 1 2 63 64 65 130, three parts, every secondary kept", [130, 65, 64, 63, 2, 1, 0], 3, best_n=1000, pri_ratio=0.1, seed=2),
    pooled("pools of 64 65 130 200, one part", [64, 65, 130, 200], 1, best_n=1000, pri_ratio=0.1, seed=3),
    pooled("CIGARs of 0 1 3 4 5 63 64 65 1000 words at odd offsets", [9, 18, 27, 5], 2, n_cigars=(0, 1, 3, 4, 5, 63, 64, 65, 1000), best_n=50, pri_ratio=0.1, seed=4),
    pooled("CIGARs, three parts, aligned and unaligned sources", [12, 7, 30], 3, n_cigars=(1000, 65, 64, 63, 5, 4, 3, 1, 0), best_n=50, pri_ratio=0.1, seed=5, lead=(4, 1, 7)),
    pooled("an empty part among three", [3, 70, 0, 9], 3, empty_part=1, seed=6),
    pooled("kept behind dropped: best_n 1 and secondary 0", [20, 40, 66], 2, best_n=1, seed=7),
    pooled("no secondaries", [20, 40, 66], 2, secondary=0, seed=8),
    pooled("mask_level 0.9", [30, 129], 2, mask_level=0.9, pri_ratio=0.5, seed=9),
    case("zero queries, two empty parts", [part([]), part([])], 0),
    case("zero parts", [], 4),
    case("queries without a record", [part([]), part([])], 7),
]
CASES = HAND + EDGE


# ---- the two genomes of the split-against-unsplit experiments ---------------------------------------------------------------------------
LENGTHS = (20000, 15000, 25000, 12000)
CUTS = {2: [0, 0, 1, 1], 4: [0, 1, 2, 3]}


def genome(repeats=False):
    """-> (targets, reads) as lists of str: four random targets and 80 reads of about 3,000 bases; repeats: three copies of one 3,000-base
    family (3 % substitutions each) planted in every target"""
    rng = np.random.default_rng(7)
    g = [synth.random_seq(rng, n) for n in LENGTHS]
    if repeats:
        fam = synth.random_seq(rng, 3000)
        for t in g:
            for k in range(3):
                at = 500 + k * (len(t) - 4000) // 2
                t[at:at + 3000] = synth.mutate(rng, fam, sub=0.03, ins=0.0, dele=0.0)
    reads, _ = synth.simulate_reads(rng, g, 80, 3000)
    return [bytes(t).decode() for t in g], [bytes(r).decode() for r in reads]


def max_part_bases(part_of):
    """a max_bases under which telr_part_plan cuts LENGTHS exactly into part_of (the extent of the largest part, plus one)"""
    ext = {}
    for t, p in enumerate(part_of):
        ext[p] = ref.extent_next(ext.get(p, 0), LENGTHS[t])
    return max(ext.values()) + 1


PRIMARY_FIELDS = ("tid", "qs", "qe", "ts", "te", "dp_score", "mapq")
