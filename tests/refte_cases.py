"""Hand-built record arrays for telr_annotate_hits (tests/test_refte_ref.py holds the plain-Python definition to them, tests/test_gpu_refte.py
the engine).  Every case names the edge it claims; `expect` is the hand-derived feature list (tid, start, end, family, strand, score,
n_hits) where it is short enough to write down, `n_expect` the hand-derived number of features otherwise.

The engine's segmented scan gives a lane sixteen consecutive hits, a wave 1,024, a workgroup a tile of 4,096, and combines the tiles'
totals in a second launch: the sizes 15 / 16 / 17, 1,023 / 1,024 / 1,025, 4,095 / 4,096 / 4,097 and 8,193 are its steps; 63 / 64 / 65 and
255 / 256 / 257 are those of a scan with one hit per lane."""
import numpy as np

from telr_amd._abi import ALN_DTYPE, TILE_DTYPE

PRIMARY, SECONDARY, REV = 1, 2, 8


def rec(qid, qs, qe, family=0, rev=0, score=100, mapq=60, flags=None):
    return dict(qid=qid, qs=qs, qe=qe, tid=family, dp_score=score, mapq=mapq, flags=(PRIMARY | (REV if rev else 0)) if flags is None else flags)


def records(rows, shuffle=None):
    a = np.zeros(len(rows), ALN_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            a[i][k] = v
        a[i]["qlen"] = 0
    if shuffle is not None and len(a) > 1:
        a = a[np.random.RandomState(shuffle).permutation(len(a))]
    return a


def one_tile(length, n_targets=1):
    """every target of `length` bases as ONE tile (qid = the target)"""
    return np.array([(t, 0, length) for t in range(n_targets)], TILE_DTYPE), [length] * n_targets


def case(name, claim, rows, tiles_tl, n_families=1, opt=None, expect=None, n_expect=None, shuffle=None):
    tiles, tl = tiles_tl
    return dict(name=name, claim=claim, alns=records(rows, shuffle), tiles=tiles, target_len=np.array(tl, np.int32), n_families=n_families,
                opt=dict(opt or {}), expect=expect, n_expect=len(expect) if expect is not None else n_expect)


def _cases():
    out = []
    T = one_tile(3000000)
    out.append(case("no records", "0 records", [], T, expect=[]))
    out.append(case("one record", "1 record", [rec(0, 500, 900, score=321)], T, expect=[(0, 500, 900, 0, 0, 321, 1)]))
    out.append(case("all ineligible", "secondary; mapq below; qe - qs = min_len - 1",
                    [rec(0, 0, 500, flags=SECONDARY), rec(0, 1000, 1500, mapq=9), rec(0, 2000, 2099)], T, opt=dict(min_mapq=10), expect=[]))
    out.append(case("just eligible", "mapq = min_mapq and qe - qs = min_len are hits; a secondary reverse record is not",
                    [rec(0, 1000, 1500, mapq=10, score=7), rec(0, 2000, 2100, score=8), rec(0, 5000, 6000, flags=SECONDARY | REV)], T, opt=dict(min_mapq=10),
                    expect=[(0, 1000, 1500, 0, 0, 7, 1), (0, 2000, 2100, 0, 0, 8, 1)]))
    # the running maximum: [0,100) [10,20) [50,60) [100,110)
    rm = [rec(0, 0, 100, score=4), rec(0, 10, 20, score=3), rec(0, 50, 60, score=2), rec(0, 100, 110, score=1)]
    out.append(case("running maximum, join_gap 0", "M is the maximum end of ALL earlier hits: [10,20) and [50,60) lie inside [0,100); the previous hit's end gives three or more",
                    rm, T, opt=dict(min_len=10, join_gap=0), expect=[(0, 0, 100, 0, 0, 4, 3), (0, 100, 110, 0, 0, 1, 1)], shuffle=1))
    out.append(case("running maximum, join_gap 1", "book-ended [100,110) joins under join_gap 1", rm, T, opt=dict(min_len=10, join_gap=1),
                    expect=[(0, 0, 110, 0, 0, 4, 4)], shuffle=2))
    # start against M = 2000
    for gap in (0, 1, 50):
        for d in (-1, 0, 1, 49, 50):
            joined = 2000 + d < 2000 + gap
            exp = [(0, 1000, max(2000, 2000 + d + 300), 0, 0, 100, 2)] if joined else [(0, 1000, 2000, 0, 0, 100, 1), (0, 2000 + d, 2300 + d, 0, 0, 100, 1)]
            out.append(case("start = M%+d, join_gap %d" % (d, gap), "a new feature iff start >= M + join_gap", [rec(0, 1000, 2000), rec(0, 2000 + d, 2300 + d)], T,
                            opt=dict(join_gap=gap), expect=exp))
    out.append(case("identical duplicates", "equal hits are one feature", [rec(0, 100, 300, score=5)] * 3, T, expect=[(0, 100, 300, 0, 0, 5, 3)]))
    T2 = one_tile(5000, 2)
    rows = [rec(t, 1000, 2000, family=f, rev=s, score=10 * t + 3 * f + s) for t in (0, 1) for f in (0, 1) for s in (0, 1)]
    out.append(case("never joined", "the same interval on both strands, in two families, on two targets", rows, T2, n_families=2,
                    expect=[(t, 1000, 2000, f, s, 10 * t + 3 * f + s, 1) for t in (0, 1) for f in (0, 1) for s in (0, 1)], shuffle=3))
    out.append(case("score maximum in the middle", "a feature's score is the maximum of its hits', wherever it sits",
                    [rec(0, 100, 400, score=5), rec(0, 300, 700, score=900), rec(0, 600, 1000, score=7), rec(0, 2000, 2200, score=901)], T,
                    expect=[(0, 100, 1000, 0, 0, 900, 3), (0, 2000, 2200, 0, 0, 901, 1)], shuffle=4))
    # one long hit, K short disjoint ones inside it, one more inside it far behind them, one outside
    for K in (15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193):
        # (the feature's score maximum sits on its FIRST hit: it reaches the feature's last hit only through the same carry)
        rows = [rec(0, 0, 2000000, score=500)] + [rec(0, 1000 + 200 * i, 1100 + 200 * i, score=i % 40) for i in range(K)]
        rows += [rec(0, 1900000, 1900100, score=60), rec(0, 2000000, 2000100, score=70)]
        out.append(case("long hit over %d short ones" % K, "the maxima of end and of score are carried across %d hits: a lane, a wave, a workgroup, a tile of the totals' pass" % K,
                        rows, T, expect=[(0, 0, 2000000, 0, 0, 500, K + 2), (0, 2000000, 2000100, 0, 0, 70, 1)], shuffle=100 + K))
    # a run boundary exactly behind hit B - 1: the earlier run's maximum exceeds every end of the later run
    # With more than a tile of later hits the carry into a tile of the later run comes from the last EARLIER TILE that holds a head (the later
    # run's first hit), not from the first tile on: 4,096 + 5,000 puts that head on a tile's first hit, 5,000 + 9,000 in a tile's middle.
    for B, later in ((16, 20), (64, 20), (256, 20), (1024, 20), (4096, 20), (4096, 5000), (5000, 9000)):
        rows = [rec(0, 0, 2000000, family=0)] + [rec(0, 1000 + 200 * i, 1100 + 200 * i, family=0) for i in range(B - 1)]
        rows += [rec(0, 1000 + 200 * i, 1100 + 200 * i, family=1, score=i) for i in range(later)]
        exp = sorted([(0, 0, 2000000, 0, 0, 100, B)] + [(0, 1000 + 200 * i, 1100 + 200 * i, 1, 0, i, 1) for i in range(later)], key=lambda f: (f[0], f[1], f[2], f[3], f[4]))
        out.append(case("run boundary at %d|%d" % (B - 1, B) + ("" if later == 20 else ", %d later hits" % later),
                        "a carry that ignores the head flag, or that is taken from the first tile on, joins the later run's hits", rows, T, n_families=2, expect=exp,
                        shuffle=200 + B + later))
    for n in (4095, 4096, 4097):
        out.append(case("%d single-hit features" % n, "the scan's size steps", [rec(0, 200 * i, 200 * i + 100, score=i) for i in range(n)], T,
                        expect=[(0, 200 * i, 200 * i + 100, 0, 0, i, 1) for i in range(n)], shuffle=300 + n))
    # tile offsets: target of 10,000 bases, tile 4,096, stride 2,048 -> tiles at 0, 2,048, 4,096 and 6,144 (the last 3,856 bases long)
    tiles = np.array([(0, 0, 4096), (0, 2048, 4096), (0, 4096, 4096), (0, 6144, 3856)], TILE_DTYPE)
    rows = [rec(3, 3000, 3856, score=11), rec(1, 2100, 2552, score=12), rec(2, 52, 504, score=13)]
    out.append(case("tile offsets", "a hit in the last tile ends at the target's last base; one copy seen from two tiles is one feature", rows, (tiles, [10000]),
                    expect=[(0, 4148, 4600, 0, 0, 13, 2), (0, 9144, 10000, 0, 0, 11, 1)]))
    return out


CASES = _cases()
SMALL = [c for c in CASES if c["expect"] is not None and len(c["alns"]) <= 8]


# ---- the planted reference: three random families, copies of them planted into a random 60,000-base reference --------------------------
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
PLANT_SEED = 11
PLANT_TILE, PLANT_STRIDE = 8192, 4096


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def planted(seed=PLANT_SEED):
    """-> dict(ref, lib_names, lib_seqs, plants): plants = [(start, end, family, strand)] ascending.  Full-length copies, 5'-truncated ones
    (cut at 1,000 and 2,500), copies with 3 / 5 / 10 % substitutions on both strands (none within 50 bases of a copy's ends: a substitution
    at an end base is clipped by any local alignment and would move the end), a copy across the start of tile 1 (4,096), two book-ended
    copies of one family.  The reference base next to a truncated end is set to differ from the consensus base that would continue the copy."""
    import random
    rng = random.Random(seed)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    lib_names, lib_seqs = ["famA", "famB", "famC"], [rand(3000), rand(5000), rand(1200)]
    ref = list(rand(60000))
    #        start  family cut   strand  substitutions
    spec = [(2000, 0, 0, 0, 0.0), (7000, 1, 0, 1, 0.0), (14000, 0, 1000, 0, 0.0), (18000, 1, 2500, 1, 0.0), (23000, 2, 0, 0, 0.05),
            (26000, 2, 0, 1, 0.10), (30000, 0, 0, 1, 0.03), (36000, 2, 0, 0, 0.0), (37200, 2, 0, 0, 0.0), (42000, 1, 0, 0, 0.0), (50000, 0, 0, 0, 0.10)]
    plants = []
    for start, fam, cut, strand, sub in spec:
        copy = list(lib_seqs[fam][cut:])
        for i in range(50, len(copy) - 50):
            if rng.random() < sub:
                copy[i] = rng.choice([c for c in "ACGT" if c != copy[i]])
        copy = "".join(copy)
        if cut:                                      # the base that would continue the copy to its 5' side
            before = lib_seqs[fam][cut - 1]
            if strand == 0:
                ref[start - 1] = rng.choice([c for c in "ACGT" if c != before])
            else:
                ref[start + len(copy)] = rng.choice([c for c in "ACGT" if c != _COMP[before]])
        ref[start:start + len(copy)] = revcomp(copy) if strand else copy
        plants.append((start, start + len(copy), fam, strand))
    assert len(ref) == 60000
    return dict(ref="".join(ref), lib_names=lib_names, lib_seqs=lib_seqs, plants=sorted(plants))


def planted_joined(plants):
    """the plants under join_gap 1: the two book-ended copies are one feature"""
    out = []
    for p in plants:
        if out and out[-1][2:] == p[2:] and out[-1][1] == p[0]:
            out[-1] = (out[-1][0], p[1]) + p[2:]
        else:
            out.append(p)
    return out
