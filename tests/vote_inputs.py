"""Inputs of tests/test_vote_ref.py, tests/test_gpu_vote_edges.py and tests/vote_child.py: small synthetic targets and queries that sit
on the fixed caps and alternative paths of the sub-read vote (k_seed_vote of telr_amd/csrc/kernels.hip.h) and on the tiers of the
anchor sort (telr_amd/csrc/segsort.hip.h).  Fixed seeds; every builder measures on the CPU what its test asserts -- from the oracle's
sketch and index dump, by brute force over them (Index.keys: the unvoted anchor keys) and with tests/vote_ref.py -- and asserts it
before it returns.  Nothing here comes from the engine.  min_mid_occ is raised so that no occurrence list is cut.

A case is a Case: targets, queries (every query is followed by its reverse complement unless stated), io, mo and `facts`, the
measured quantities.  What the kernel sees of a query is Index.profile: its minimizers in order, their occurrence counts, sub-reads
(last base // vote_len) and chunks (VOTE_MZ = 128 minimizers of a sub-read).

  stash_case()        one sub-read with 767, 768, 769 and several thousand hits (VOTE_HCAP = 768)
  stash_chunks_case() the same beyond the cap in a sub-read of two chunks (vote_len = 512)
  chunk_case(L)       w = 1: sub-reads of exactly L = 127, 128, 129 and 300 minimizers, survivors of both strands in several chunks
  trip_case()         chunks of 274, 511, 512, 513 and 1,316 hits: list starts on hits 31, 32, 63, 64, lists across a window and a
                      trip edge, a trip without a list start, singletons between long lists (the 512-hit trip, the 64-hit windows)
  geometry_case()     qlen around vote_len, 1 .. 7 sub-reads, sub-reads without minimizers and without hits
  subcap_case()       511, 512, 513 and 1,025 sub-reads of 32 bases (VOTE_SUBCAP = 512)
  threshold_case(o)   designed vote tables: the ceiling, a sum on and one below the threshold, the other strand, the fold, an alias
  width_case()        65,535 and 65,536 staged hits, all in ONE bin (16- and 32-bit counters);  wide_bin_case(): a bin of 118,400 votes
  tier_case(voted)    queries with EXACTLY 0 .. 20,481 anchors after seeding (voted = False) or after voting (True)"""
import functools

import numpy as np

from telr_amd import synth
from telr_amd.presets import preset
import vote_ref as VR

VOTE_HCAP, VOTE_MZ, VOTE_TRIP, VOTE_SUBCAP, VOTE_WAVES, LIM16 = 768, 128, 512, 512, 3, 65535
SEGSORT_CAP = 20480
TIER_COUNTS = (0, 1, 2, 3, 128, 129, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 20479, 20480, 20481)
NOCUT = 1_000_000


def _s(a):
    return bytes(np.asarray(a, np.uint8)).decode()


def _a(s):
    return np.frombuffer(s.encode(), np.uint8).copy()


def rc(s):
    return _s(synth.revcomp_arr(_a(s)))


def with_rc(qs):
    return [x for q in qs for x in (q, rc(q))]


def opts(vote_len=256, shift=5, vmin=3, frac=128, k=13, w=5):
    """ngmlr-ont with the vote's four options, (w,k), and no occurrence list cut"""
    io, mo = preset("ngmlr-ont")
    io.k, io.w = k, w
    mo.min_mid_occ = mo.max_mid_occ = NOCUT
    mo.vote_len, mo.vote_bin_shift, mo.vote_min, mo.vote_frac_q8 = vote_len, shift, vmin, frac
    return io, mo


def plain(mo):
    o = mo.copy(); o.vote_len = 0
    return o


class Case:
    def __init__(self, name, targets, queries, io, mo, **facts):
        self.name, self.targets, self.queries, self.io, self.mo, self.facts = name, targets, queries, io, mo, facts


class Index:
    """the oracle's index of the targets, dumped: per-occurrence hashes (sorted) and positions (reference position << 1 | strand)"""
    def __init__(self, targets, io):
        from oracle import binding as ob
        self.ob, self.io = ob, io
        self.oix = ob.OracleIndex(list(targets), io)
        self.h, self.y = self.oix.dump()
        assert (np.diff(self.h.astype(np.int64)) >= 0).all()

    def profile(self, q, vote_len):
        """-> dict: per minimizer of q in order h (hash), span, qpos (last base), z (strand), n (occurrences), lo (first occurrence),
        sub (sub-read)"""
        x, y = self.ob.sketch(q, self.io.k, self.io.w)
        h = x >> np.uint64(8)
        lo = np.searchsorted(self.h, h, side="left"); hi = np.searchsorted(self.h, h, side="right")
        qpos = (y >> 1).astype(np.int64)
        assert (np.diff(qpos) > 0).all()
        return dict(h=h, span=(x & np.uint64(0xff)).astype(np.int64), qpos=qpos, z=(y & 1).astype(np.int64), n=(hi - lo).astype(np.int64),
                    lo=lo.astype(np.int64), sub=qpos // vote_len)

    def hits(self, q):
        return int(self.profile(q, 1)["n"].sum())

    def keys(self, q):
        """the unvoted anchor keys of q by brute force, sorted"""
        p = self.profile(q, 1)
        m = np.repeat(np.arange(len(p["n"])), p["n"])
        occ = self.y[np.concatenate([np.arange(a, a + c) for a, c in zip(p["lo"], p["n"])]).astype(np.int64)] if len(m) else np.zeros(0, np.uint32)
        gp = (occ >> 1).astype(np.uint64); rev = ((occ & 1).astype(np.int64) ^ p["z"][m]).astype(np.uint64)
        qpos, span = p["qpos"][m], p["span"][m]
        qadj = np.where(rev == 1, len(q) - (qpos + 1 - span) - 1, qpos).astype(np.uint64)
        return np.sort(rev << np.uint64(63) | gp << np.uint64(32) | qadj << np.uint64(8) | span.astype(np.uint64))

    def voted(self, q, mo):
        return VR.vote(self.keys(q), len(q), mo)


def sub_reads(p):
    """-> {sub-read: (g0, g1)}: its run of minimizers"""
    out = {}
    for s in np.unique(p["sub"]).tolist():
        g = np.nonzero(p["sub"] == s)[0]
        assert g[-1] - g[0] + 1 == len(g)
        out[s] = (int(g[0]), int(g[-1]) + 1)
    return out


def chunks(p):
    """-> [(sub-read, chunk number, list lengths of the chunk's minimizers (0 = no hits))] in the kernel's order"""
    out = []
    for s, (g0, g1) in sorted(sub_reads(p).items()):
        for c, gc in enumerate(range(g0, g1, VOTE_MZ)):
            out.append((s, c, p["n"][gc:min(g1, gc + VOTE_MZ)]))
    return out


def sub_hits(p):
    return {s: int(p["n"][g0:g1].sum()) for s, (g0, g1) in sub_reads(p).items()}


def survivor_chunks(ix, q, mo):
    """-> {sub-read: set of (chunk, forward qpos, rev)} of the survivors of q"""
    p = ix.profile(q, mo.vote_len)
    sv = ix.voted(q, mo)
    fq = VR.forward_qpos(sv, len(q)); rev = VR.fields(sv)[0]
    g = np.searchsorted(p["qpos"], fq)
    assert (p["qpos"][g] == fq).all()
    sr = sub_reads(p)
    out = {}
    for gi, f, r in zip(g.tolist(), fq.tolist(), rev.tolist()):
        s = int(p["sub"][gi])
        out.setdefault(s, set()).add(((gi - sr[s][0]) // VOTE_MZ, f, r))
    return out


def tune(make, measure, want, lo, hi):
    """the L in [lo, hi] with measure(make(L)) == want, for a measure that does not fall as L grows"""
    a, b = lo, hi
    assert measure(make(b)) >= want >= measure(make(a)), (want, measure(make(a)), measure(make(b)))
    while a < b:
        m = (a + b) // 2
        if measure(make(m)) >= want:
            b = m
        else:
            a = m + 1
    assert measure(make(a)) == want, (want, a, measure(make(a)))
    return make(a)


def _other(b):
    """a base that is not b"""
    return synth.BASES[(np.searchsorted(synth.BASES, b) + 1) % 4]


def _scatter(rng, g, seq, positions):
    for p in positions:
        g[p:p + len(seq)] = seq


# ---- the stash cap --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stash_genome():
    """-> (target, ra, rb).  40 kb; family FA (90 bases) 32 times and FB (90 bases) 150 times: 31 and 149 copies on a 200-base grid
    below 37 kb, and one copy of each at ra and rb in a clear stretch at the end, followed by unique sequence: the queries start there"""
    rng = np.random.default_rng(20270101)
    g = synth.random_seq(rng, 40_000)
    fa, fb = synth.random_seq(rng, 90), synth.random_seq(rng, 90)
    slots = 1000 + 200 * rng.permutation(180)
    pa, pb = np.sort(slots[:31]), np.sort(slots[31:180])
    _scatter(rng, g, fa, pa); _scatter(rng, g, fb, pb)
    ra, rb = 37_000, 38_000
    g[ra:ra + 90] = fa; g[rb:rb + 90] = fb
    return _s(g), ra, rb


@functools.lru_cache(maxsize=None)
def stash_case():
    t, ra, rb = _stash_genome()
    io, mo = opts()
    ix = Index([t], io)
    qs = [tune(lambda L: t[ra:ra + L], ix.hits, n, 13, 256) for n in (VOTE_HCAP - 1, VOTE_HCAP, VOTE_HCAP + 1)]
    qs.append(t[rb:rb + 250])
    qs = with_rc(qs)
    hits = []
    for q in qs:
        p = ix.profile(q, mo.vote_len)
        assert len(q) <= mo.vote_len and set(p["sub"].tolist()) == {0} and len(p["n"]) <= VOTE_MZ
        hits.append(int(p["n"].sum()))
    assert hits[:6] == [767, 767, 768, 768, 769, 769] and hits[6] == hits[7] > 2000, hits
    kept = [len(ix.voted(q, mo)) for q in qs]
    assert all(0 < k < h for k, h in zip(kept, hits))          # beyond the cap the second walk has hits to drop
    return Case("stash", [t], qs, io, mo, hits=hits, kept=kept)


@functools.lru_cache(maxsize=None)
def stash_chunks_case():
    t, ra, rb = _stash_genome()
    io, mo = opts(vote_len=512)
    ix = Index([t], io)
    qs = with_rc([t[rb:rb + 500], t[ra:ra + 500]])
    hits, nmz = [], []
    for q in qs:
        p = ix.profile(q, mo.vote_len)
        assert set(p["sub"].tolist()) == {0}
        hits.append(int(p["n"].sum())); nmz.append(len(p["n"]))
    assert min(nmz) > VOTE_MZ and hits[0] > 2000 and hits[2] > VOTE_HCAP, (hits, nmz)
    kept = [len(ix.voted(q, mo)) for q in qs]
    assert all(0 < k < h for k, h in zip(kept, hits))
    return Case("stash_chunks", [t], qs, io, mo, hits=hits, nmz=nmz, kept=kept)


# ---- the chunk cap --------------------------------------------------------------------------------------------------------------
CHUNK_LENS = (127, 128, 129, 300)


def _chunk_check(ix, x, mo):
    """what chunk_case claims of one query -> the number of multi-chunk sub-reads checked, or None if the query misses a claim"""
    V = mo.vote_len
    p = ix.profile(x, V)
    sr = sub_reads(p)
    full = [s for s in sr if 0 < s < (len(x) // V)]
    if not full or any(sr[s][1] - sr[s][0] != V for s in full):          # EXACTLY vote_len minimizers
        return None
    sc = survivor_chunks(ix, x, mo)
    hits = sub_hits(p)
    if len(ix.voted(x, mo)) >= sum(hits.values()):
        return None
    multi = 0
    if V > VOTE_MZ:
        for s in full:
            # survivors from chunk 0 and from the last chunk, on the stash path
            if hits[s] > VOTE_HCAP or not {c for c, _, _ in sc.get(s, ())} >= {0, (V - 1) // VOTE_MZ}:
                return None
            multi += 1
    # a sub-read whose survivors differ in strand (and qpos)
    return multi if [s for s in full if {r for _, _, r in sc.get(s, ())} == {0, 1}] else None


@functools.lru_cache(maxsize=None)
def chunk_case(vote_len):
    """w = 1 (every 13-mer a minimizer): a full sub-read holds exactly vote_len minimizers.  The query is la bases of locus A followed
    by the reverse complement of 1,200 - la bases of locus B, so the sub-read across the joint has survivors of both strands, in the
    query and in its reverse complement (la: the first of 560, 567, .. for which that holds); a 40-base family with five copies lies
    in A, its other copies lose the vote."""
    rng = np.random.default_rng(20270102)
    g = synth.random_seq(rng, 8000)
    nf = synth.random_seq(rng, 40)
    _scatter(rng, g, nf, (600, 1100, 3000, 5200, 7000))
    t = _s(g)
    io, mo = opts(vote_len=vote_len, frac=64, w=1)
    ix = Index([t], io)
    for la in range(560, 700, 7):
        qs = with_rc([t[1000:1000 + la] + rc(t[4000:4000 + 1200 - la])])
        multi = [_chunk_check(ix, x, mo) for x in qs]
        if None not in multi:
            break
    assert None not in multi
    return Case("chunk%d" % vote_len, [t], qs, io, mo, multi=sum(multi), la=la)


# ---- trips and windows ----------------------------------------------------------------------------------------------------------
TRIP_K, TRIP_LEN = 15, 128
# per sub-read 1 .. 5: the occurrence counts of the tokens at minimizer slots 0, 15, 30, ... (every other minimizer of the sub-read
# occurs once, at the query's own locus: a singleton list)
TRIP_DESIGN = ((31, 18, 100), (384,), (385,), (386,), (490, 700))
TRIP_CHUNK_HITS = (274, 511, 512, 513, 1316)


@functools.lru_cache(maxsize=None)
def trip_case():
    """k = 15, w = 1, vote_len = 128: sub-reads 1 .. 5 are one chunk of 128 minimizers each.  The query lies once in the target (every
    minimizer hits there: 128 votes on one diagonal); a token is a 15-mer of the query copied c - 1 more times into a dump zone, so its
    list holds c occurrences and the dump copies lose the vote."""
    rng = np.random.default_rng(20270103)
    k = TRIP_K
    qa = synth.random_seq(rng, TRIP_LEN * 6 + 40)
    dump = []
    for s, design in enumerate(TRIP_DESIGN, start=1):
        for i, c in enumerate(design):
            st = TRIP_LEN * s + 15 * i - (k - 1)
            tok = qa[st:st + k]
            # (a copy stands between two bases that differ from the token's neighbours in the query: the 15-mers next to it do not match)
            cp = np.concatenate([[_other(qa[st - 1])], tok, [_other(qa[st + k])]]).astype(np.uint8)
            dump += [cp] * (c - 1)
    g = np.concatenate([synth.random_seq(rng, 500), qa, synth.random_seq(rng, 500)] + dump + [synth.random_seq(rng, 500)])
    t, q = _s(g), _s(qa)
    io, mo = opts(vote_len=TRIP_LEN, k=k, w=1)
    ix = Index([t], io)
    p = ix.profile(q, TRIP_LEN)
    ch = [(s, c, n) for s, c, n in chunks(p) if 1 <= s <= 5]
    assert [(s, c) for s, c, _ in ch] == [(s, 0) for s in range(1, 6)] and all(len(n) == VOTE_MZ for _, _, n in ch)
    lists = [n for _, _, n in ch]
    for n, design in zip(lists, TRIP_DESIGN):
        want = np.ones(VOTE_MZ, np.int64); want[15 * np.arange(len(design))] = design
        assert (n == want).all(), (n, want)
    assert tuple(int(n.sum()) for n in lists) == TRIP_CHUNK_HITS                  # the per-chunk hit totals (prefix sums below)
    starts = [np.cumsum(n) - n for n in lists]
    ends = [np.cumsum(n) for n in lists]
    # chunk 1: lists start on hits 31, 32, 63, 64 of the first window; one list lies across the window edge at hit 128
    assert {31, 32, 63, 64} <= set(starts[0].tolist())
    assert any(a < 128 < e for a, e in zip(starts[0], ends[0]))
    # chunks 2 .. 4: 511, 512, 513 hits -- the last one's 513th hit is alone in a second trip
    # chunk 5: a 700-occurrence list from hit 504 to 1,204: across the trip edge at 512, and no list starts in the trip 512 .. 1,023
    s5, e5 = starts[4], ends[4]
    assert any(a < VOTE_TRIP < e for a, e in zip(s5, e5)) and not ((s5 >= VOTE_TRIP) & (s5 < 2 * VOTE_TRIP)).any() and (lists[4] > VOTE_TRIP).any()
    assert TRIP_CHUNK_HITS[4] > 2 * VOTE_TRIP and TRIP_CHUNK_HITS[4] > VOTE_HCAP >= TRIP_CHUNK_HITS[3]
    # singletons (the occurrence stored inline) between longer lists
    assert all((n == 1).any() and (n > 1).any() for n in lists)
    qs = with_rc([q])
    p2 = ix.profile(qs[1], TRIP_LEN)
    assert p2["n"].sum() == p["n"].sum()
    for x in qs:
        assert 0 < len(ix.voted(x, mo)) < ix.hits(x)
    return Case("trip", [t], qs, io, mo, chunk_hits=TRIP_CHUNK_HITS, prefix=[np.cumsum(n) for n in lists])


# ---- sub-read geometry ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geo_genome():
    """60 kb with a 120-base family every 2,000 bases (30 copies): a sub-read that lies partly in a copy drops the other copies"""
    rng = np.random.default_rng(20270104)
    g = synth.random_seq(rng, 60_000)
    fam = synth.random_seq(rng, 120)
    _scatter(rng, g, fam, range(1000, 60_000, 2000))
    return g


GEO_QLENS = (255, 256, 257, 300, 512, 768, 1024, 1792)          # vote_len - 1, vote_len, vote_len + 1, a non-multiple; 1, 2, 3, 4, 7 sub-reads


@functools.lru_cache(maxsize=None)
def geometry_case():
    g = _geo_genome()
    io, mo = opts()
    V = mo.vote_len
    qs = [_s(g[2950 + 2000 * i:2950 + 2000 * i + n]) for i, n in enumerate(GEO_QLENS)]
    # a sub-read without a minimizer: a run of N across all of it, at the start, in the middle and at the end of a read of six
    for a, b in ((0, 280), (500, 780), (1270, 1536)):
        x = g[20_950:20_950 + 1536].copy(); x[a:b] = ord("N")
        qs.append(_s(x))
    # a sub-read whose minimizers have no hits: bases 499 .. 781 are not in the target
    x = g[24_950:24_950 + 1536].copy(); x[499:781] = synth.random_seq(np.random.default_rng(20270105), 282)
    qs.append(_s(x))
    qs = with_rc(qs)
    ix = Index([_s(g)], io)
    nsub = [(len(q) + V - 1) // V for q in qs]
    assert {1, 2, 3, 4, 7} <= set(nsub) and [len(q) for q in qs[:16:2]] == list(GEO_QLENS)
    empty = []
    for q in qs[16:22]:
        p = ix.profile(q, V)
        miss = sorted(set(range(6)) - set(p["sub"].tolist()))
        assert len(miss) == 1
        empty.append(miss[0])
    assert empty == [0, 5, 2, 3, 5, 0]                                             # start, middle, end -- and where the reverse complement has them
    for q in qs[22:24]:
        p = ix.profile(q, V)
        h = sub_hits(p)
        assert set(h) == set(range(6)) and [s for s in h if h[s] == 0] in ([2], [3])
    edge = np.concatenate([ix.profile(q, V)["qpos"] % V for q in qs])
    assert 0 in edge and V - 1 in edge                                             # a minimizer's last base on the first / last base of a sub-read
    for q in qs:
        assert 0 < len(ix.voted(q, mo)) <= ix.hits(q)
    assert any(len(ix.voted(q, mo)) < ix.hits(q) for q in qs)
    return Case("geometry", [_s(g)], qs, io, mo, nsub=nsub)


SUBCAP_NSUB = (VOTE_SUBCAP - 1, VOTE_SUBCAP, VOTE_SUBCAP + 1, 2 * VOTE_SUBCAP + 1)


@functools.lru_cache(maxsize=None)
def subcap_case():
    """vote_len = 32: reads of 511, 512, 513 and 1,025 sub-reads (16 .. 33 kb), one of them ending inside its last sub-read"""
    g = _geo_genome()
    io, mo = opts(vote_len=32)
    qs = [_s(g[500 + 700 * i:500 + 700 * i + 32 * n - (5 if i == 2 else 0)]) for i, n in enumerate(SUBCAP_NSUB)]
    qs = with_rc(qs)
    nsub = [(len(q) + 31) // 32 for q in qs]
    assert nsub[::2] == list(SUBCAP_NSUB) and nsub[1::2] == list(SUBCAP_NSUB)
    ix = Index([_s(g)], io)
    for q in qs:
        p = ix.profile(q, 32)
        assert p["sub"].max() == (len(q) - 1) // 32                                   # the last sub-read holds a minimizer
        assert 0 < len(ix.voted(q, mo)) < ix.hits(q)
    return Case("subcap", [_s(g)], qs, io, mo, nsub=nsub)


# ---- threshold arithmetic -------------------------------------------------------------------------------------------------------
THR_K, THR_LEN, THR_STEP = 19, 512, 20
# per sub-read 1 .. 4 the loci: (first token, last token, rev, bin, region).  A locus holds the tokens first .. last of the sub-read
# at the query's spacing, so all its hits fall on ONE diagonal: last - first + 1 votes in `bin`; region m puts it m * (1024 << 5) bases
# further along the target (the same bin: an alias; every sub-read has three regions of its own)
THR_DESIGN = (
    # the ceiling (fullest 7: 128 * 7 / 256 = 3.5 -> 4), a sum on the threshold (4: single bin, and 1 + 2 + 1) and one below (3)
    ((0, 6, 0, 100, 0), (7, 10, 0, 300, 0), (11, 13, 0, 500, 0), (14, 15, 0, 700, 0), (16, 16, 0, 701, 1), (17, 17, 0, 699, 2)),
    # the other strand of the fullest diagonal: 3 votes there do not borrow the 8; 4 votes on the other strand elsewhere stay
    ((0, 7, 0, 200, 0), (8, 10, 1, 200, 1), (11, 14, 1, 600, 0)),
    # neighbours across the fold: 3 votes in bin 1023 and 3 in bin 0
    ((0, 7, 0, 400, 0), (8, 10, 0, 1023, 0), (11, 13, 0, 0, 1), (14, 16, 0, 512, 0)),
    # two loci 1024 << 5 bases apart with 2 votes each: one bin, 4 votes
    ((0, 7, 0, 50, 0), (8, 9, 0, 800, 0), (10, 11, 0, 800, 1), (12, 13, 0, 900, 0)),
)
THR_OPTS = ((3, 128), (6, 128), (1, 100))          # (vote_min, vote_frac_q8): the fraction decides; vote_min decides; 700 / 256 and 800 / 256


@functools.lru_cache(maxsize=None)
def _thr_seqs():
    rng = np.random.default_rng(20270106)
    k, shift = THR_K, 5
    qlen = THR_LEN * (len(THR_DESIGN) + 1)
    qa = synth.random_seq(rng, qlen)
    g = synth.random_seq(rng, 3 * len(THR_DESIGN) * (1024 << shift) + 4000)
    used = []
    for s, design in enumerate(THR_DESIGN, start=1):
        for (i0, i1, rev, b, m) in design:
            a = THR_LEN * s + THR_STEP * i0 - (k - 1); e = THR_LEN * s + THR_STEP * i1 - (k - 1) + k
            # the tokens with the base before, between and after them changed: only the tokens' own k-mers match
            seg = qa[a - 1:e + 1].copy()
            for j in [0, len(seg) - 1] + [THR_LEN * s + THR_STEP * i - (k - 1) + k - (a - 1) for i in range(i0, i1)]:
                seg[j] = _other(seg[j])
            d = 32 * b + 8 + (1024 << shift) * (3 * (s - 1) + m)
            P = ((a + d) if not rev else (d - e + qlen)) - 1
            if rev:
                seg = synth.revcomp_arr(seg)
            assert P >= 0 and all(P + len(seg) + k < u or P > v + k for u, v in used), (s, i0, P)
            g[P:P + len(seg)] = seg
            used.append((P, P + len(seg)))
    return _s(g), _s(qa)


@functools.lru_cache(maxsize=None)
def threshold_case(o=0):
    """-> Case; facts['fate'] = [(query, key, stays)] of every designed hit under THR_OPTS[o], from the measured tables"""
    t, q = _thr_seqs()
    vmin, frac = THR_OPTS[o]
    io, mo = opts(vote_len=THR_LEN, vmin=vmin, frac=frac, k=THR_K, w=1)
    ix = Index([t], io)
    keys = ix.keys(q)
    ids, tab, row = VR.tables(keys, len(q), mo)
    assert ids.tolist() == [1, 2, 3, 4]
    for s, design in enumerate(THR_DESIGN, start=1):
        want = np.zeros((2, VR.BINS), np.int64)
        for (i0, i1, rev, b, m) in design:
            want[rev, b] += i1 - i0 + 1
        assert (tab[s - 1] == want).all(), (s, np.nonzero(tab[s - 1]), np.nonzero(want))          # the designed table, nothing else
    thr, vmax = VR.thresholds(tab, mo)
    assert vmax.tolist() == [7, 8, 8, 8]
    s3 = VR.three(tab)
    rev, b = VR.fields(keys)[0], VR.bins(keys, 5)
    stays = s3[row, rev, b] >= thr[row]
    if o == 0:
        assert thr.tolist() == [4, 4, 4, 4] and (frac * 7) % 256 != 0
        # sub-read 1: 4 == threshold stays, 3 goes; of 1 + 2 + 1 only the middle bin reaches 4
        assert s3[0, 0, 300] == 4 and s3[0, 0, 500] == 3 and s3[0, 0, 700] == 4 and s3[0, 0, 701] == 3 and s3[0, 0, 699] == 3
        # sub-read 2: the fullest bin's other strand holds 3
        assert tab[1, 0, 200] == 8 and tab[1, 1, 200] == 3 and s3[1, 1, 200] == 3 and s3[1, 1, 600] == 4
        # sub-read 3: bins 1023 and 0 are neighbours (3 + 3), bin 512 is alone (3)
        assert s3[2, 0, 1023] == 6 and s3[2, 0, 0] == 6 and s3[2, 0, 512] == 3
        # sub-read 4: the alias holds 4, the single locus 2
        assert tab[3, 0, 800] == 4 and tab[3, 0, 900] == 2
    elif o == 1:
        assert thr.tolist() == [6, 6, 6, 6] and s3[2, 0, 1023] == 6 and s3[0, 0, 300] == 4          # vote_min above the fraction's 4
    else:
        assert thr.tolist() == [3, 4, 4, 4] and (frac * 7) % 256 != 0 and (frac * 8) % 256 != 0     # ceil(2.73), ceil(3.125); vote_min below
    assert stays.any() and not stays.all()
    qs = with_rc([q])
    assert 0 < len(ix.voted(qs[1], mo)) < ix.hits(qs[1])
    return Case("threshold%d" % o, [t], qs, io, mo, fate=[(0, int(k_), bool(s_)) for k_, s_ in zip(keys.tolist(), stays.tolist())])


# ---- counter width --------------------------------------------------------------------------------------------------------------
WIDTH_K, WIDTH_LEN = 15, 2048


@functools.lru_cache(maxsize=None)
def width_case():
    """a 1,024-base unit 256 times in tandem, then 8 kb of unique sequence.  Queries 0 and 2 (1 and 3: their reverse complements) start
    inside the array's last copy, run on into the unique sequence and are trimmed to exactly 65,535 and 65,536 hits; with
    vote_bin_shift = 0 and vote_len = 2,048 they are ONE sub-read whose hits all fold into ONE bin, so that bin holds 65,535 votes --
    the most a 16-bit counter holds -- and 65,536: a query on the wrong side of the split overflows.  15-mers: no chance hits.
    Nothing of these four is dropped; queries 4 and 5 begin with a copy of a small family whose other copies lose the vote."""
    rng = np.random.default_rng(20270117)
    unit = synth.random_seq(rng, 1024)
    nf = synth.random_seq(rng, 45)
    pad, tail = synth.random_seq(rng, 3000), synth.random_seq(rng, 8000)
    _scatter(rng, pad, nf, (500, 1200, 2100))
    g = np.concatenate([pad, np.tile(unit, 256), tail])
    t = _s(g)
    e = len(pad) + 256 * 1024
    io, mo = opts(vote_len=WIDTH_LEN, shift=0, k=WIDTH_K)
    ix = Index([t], io)
    x = 900
    while ix.hits(t[e - x:e]) > LIM16 - 20:           # (the part inside the array: 256 hits a minimizer)
        x -= 1
    qs = with_rc([tune(lambda L: t[e - x:e + L], ix.hits, n, 15, 7900) for n in (LIM16, LIM16 + 1)])
    qs += with_rc([_s(nf) + t[e - 900:e - 500]])
    hits = [ix.hits(q) for q in qs]
    assert hits[:4] == [LIM16, LIM16, LIM16 + 1, LIM16 + 1] and hits[4] < LIM16 and len(t) < 1_000_000
    vmax = []
    for q in qs:
        assert len(q) <= WIDTH_LEN
        _, tab, _ = VR.tables(ix.keys(q), len(q), mo)
        assert len(tab) == 1
        vmax.append(int(tab.max()))
    assert vmax[:4] == hits[:4]                                                    # every hit in one bin of one sub-read
    assert all(len(ix.voted(q, mo)) == h for q, h in zip(qs[:4], hits)) and all(0 < len(ix.voted(q, mo)) < ix.hits(q) for q in qs[4:])
    return Case("width", [t], qs, io, mo, hits=hits, vmax=vmax)


@functools.lru_cache(maxsize=None)
def wide_bin_case():
    """vote_bin_shift = 0 and a 1,024-base unit 800 times in tandem: every hit of the unit folds into one bin, which passes 65,535"""
    rng = np.random.default_rng(20270108)
    unit = synth.random_seq(rng, 1024)
    nf = synth.random_seq(rng, 45)
    pad = synth.random_seq(rng, 3000)
    _scatter(rng, pad, nf, (500, 1200, 2100))
    t = _s(np.concatenate([pad, np.tile(unit, 800), synth.random_seq(rng, 500)]))
    q = _s(np.concatenate([nf, unit[100:560]]))
    io, mo = opts(vote_len=512, shift=0)
    ix = Index([t], io)
    qs = with_rc([q])
    vmax = []
    for x in qs:
        assert len(x) <= 512
        _, tab, _ = VR.tables(ix.keys(x), len(x), mo)
        vmax.append(int(tab.max()))
        assert ix.hits(x) > LIM16 and 0 < len(ix.voted(x, mo)) < ix.hits(x)
    assert min(vmax) > LIM16 and len(t) < 1_000_000, vmax
    return Case("wide_bin", [t], qs, io, mo, vmax=vmax)


# ---- sort tiers -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tier_genome():
    """family F64 (1,024 bases, 64 copies), F8 (2,048 bases, 8 copies), a 256-base head H that holds a copy of a 45-base family (three
    more copies elsewhere: they lose the vote) and 3 kb of unique tail U; the copies lie 1,300 / 2,400 bases apart in random sequence"""
    rng = np.random.default_rng(20270109)
    f64, f8, nf = synth.random_seq(rng, 1024), synth.random_seq(rng, 2048), synth.random_seq(rng, 45)
    g = synth.random_seq(rng, 64 * 1300 + 8 * 2400 + 9000)
    _scatter(rng, g, f64, range(100, 64 * 1300, 1300))
    b = 64 * 1300
    _scatter(rng, g, f8, range(b + 100, b + 8 * 2400, 2400))
    u = b + 8 * 2400
    _scatter(rng, g, nf, (u + 100, u + 1000, u + 1500, u + 2000))
    head = g[u + 2000 - 100:u + 2000 - 100 + 256]
    tail = g[u + 4000:u + 8000]
    absent = synth.random_seq(rng, 300)
    return _s(g), _s(f64), _s(f8), _s(head), _s(tail), _s(absent)


def _tier_query(ix, measure, n):
    """head (if it fits) + F64[:256 a] + F8[:256 b] + tail[:L] with exactly n anchors: the blocks end on sub-read edges, the tail adds
    one anchor per minimizer"""
    _, f64, f8, head, tail, absent = _tier_genome()
    if n == 0:
        return absent
    pre = ""
    if measure(head + tail[:40]) <= n:
        pre = head
    for fam in (f64, f8):
        a = 0
        while 256 * (a + 1) <= len(fam) and measure(pre + fam[:256 * (a + 1)] + tail[:40]) <= n:
            a += 1
        pre += fam[:256 * a]
    return tune(lambda L: pre + tail[:L], measure, n, 12 if pre else 13, len(tail))


@functools.lru_cache(maxsize=None)
def tier_case(voted):
    """one query per count of TIER_COUNTS, in that order (no reverse complements: the counts are the point): the anchors after seeding
    (voted False: the same options with vote_len = 0) or after voting.  vote_min = 1, so that a lone minimizer of the tail's last
    sub-read stays and every count can be reached one minimizer at a time."""
    t = _tier_genome()[0]
    io, mo = opts(vmin=1)
    if not voted:
        mo = plain(mo)
    ix = Index([t], io)
    measure = (lambda q: len(ix.voted(q, mo))) if voted else ix.hits
    qs = [_tier_query(ix, measure, n) for n in TIER_COUNTS]
    counts = [measure(q) for q in qs]
    assert tuple(counts) == TIER_COUNTS, counts
    if voted:
        assert any(ix.hits(q) > c for q, c in zip(qs, counts))
    return Case("tiers_voted" if voted else "tiers_plain", [t], qs, io, mo, counts=counts)


def without_over(case):
    """the same case without the query above SEGSORT_CAP"""
    keep = [i for i, c in enumerate(case.facts["counts"]) if c <= SEGSORT_CAP]
    assert len(keep) == len(case.queries) - 1
    return Case(case.name + "_fit", case.targets, [case.queries[i] for i in keep], case.io, case.mo, counts=[case.facts["counts"][i] for i in keep])


def all_cases():
    """every case, by name (built on first use)"""
    c = {"stash": stash_case, "stash_chunks": stash_chunks_case, "trip": trip_case, "geometry": geometry_case, "subcap": subcap_case,
         "width": width_case, "wide_bin": wide_bin_case,
         "tiers_plain": lambda: tier_case(False), "tiers_voted": lambda: tier_case(True),
         "tiers_plain_fit": lambda: without_over(tier_case(False)), "tiers_voted_fit": lambda: without_over(tier_case(True))}
    for L in CHUNK_LENS:
        c["chunk%d" % L] = functools.partial(chunk_case, L)
    for o in range(len(THR_OPTS)):
        c["threshold%d" % o] = functools.partial(threshold_case, o)
    return c
