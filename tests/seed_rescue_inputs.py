"""Inputs of the TELR_MF_SEED_RESCUE tests (tests/test_seed_rescue_cpu.py, tests/test_gpu_seed_rescue.py), seeded and cached.

The rule fires where a query runs through a repeat that is MORE frequent than the occurrence cut-off, and an absent minimizer ends a
stretch like a rare one, so the queries must be accurate: the noisy reads of tests/chain_skip_inputs.py never meet it.

  two_family()   an 8-Mb random chromosome with family A (1,200 bp x 150 copies) and family B (3,000 bp x 40 copies) on a 20-kb
                 grid, and 40 near-exact queries across an A copy with 1-4 kb flanks.  B pulls the -f 2e-4 quantile BELOW A's copy
                 number (with A alone the cut-off lands on A itself and nothing is skipped).
  over_query()   one long query made of 70 pieces across A copies: with the rescue it holds more anchors than one workgroup
                 sorts in LDS (SEGSORT_CAP = 20,480).
  small_case()   a 103-kb genome with one 2-kb segment x 20 and one error-free query; cut-off clamped to 10 (-U 5,10).
  edge_cases()   small targets and named queries that meet every edge of the rule (see EDGE_NAMES), each with the rescued
                 minimizers the restatement (tests/seed_rescue_ref.py) expects."""
import functools

import numpy as np

from telr_amd import synth
from telr_amd.presets import preset
import seed_rescue_ref as R


def _s(a):
    return bytes(np.asarray(a, np.uint8)).decode()


@functools.lru_cache(maxsize=None)
def _two_family_genome():
    rng = np.random.default_rng(20261016)
    g = synth.random_seq_fast(rng, 8_000_000)
    fam_a, fam_b = synth.random_seq(rng, 1200), synth.random_seq(rng, 3000)
    slots = rng.permutation(np.arange(1, 399))[:190]
    a_pos = []
    for i, sl in enumerate(slots):
        p = int(sl) * 20000 + int(rng.integers(0, 10000))
        if i < 150:
            g[p:p + 1200] = fam_a
            a_pos.append(p)
        else:
            g[p:p + 3000] = fam_b
    return g, a_pos, rng


@functools.lru_cache(maxsize=None)
def two_family():
    """-> (targets, queries): one 8-Mb chromosome, 40 queries"""
    g, a_pos, _ = _two_family_genome()
    rng = np.random.default_rng(20261017)
    qs = []
    for i in range(40):
        p = a_pos[int(rng.integers(0, len(a_pos)))]
        lf, rf = int(rng.integers(1000, 4001)), int(rng.integers(1000, 4001))
        q = synth.mutate(rng, g[p - lf:p + 1200 + rf], 0.004, 0.0005, 0.0005)
        if i % 2:
            q = synth.revcomp_arr(q)
        qs.append(_s(q))
    return [_s(g)], qs


@functools.lru_cache(maxsize=None)
def over_query():
    """one query across 70 A copies with 300-base flanks, pieces joined end to end (error-free)"""
    g, a_pos, _ = _two_family_genome()
    return _s(np.concatenate([g[p - 300:p + 1500] for p in a_pos[:70]]))


def clamp_opts(pname):
    """the preset with the occurrence cut-off clamped to 5..10 (minimap2's -U 5,10)"""
    io, mo = preset(pname)
    mo.min_mid_occ = 5; mo.max_mid_occ = 10
    return io, mo


@functools.lru_cache(maxsize=None)
def small_case():
    """-> (targets, queries): a 103-kb genome, one 2-kb segment x 20, one error-free query across a copy"""
    rng = np.random.default_rng(20261018)
    g = synth.random_seq(rng, 103_000)
    seg = synth.random_seq(rng, 2000)
    for i in range(20):
        g[3000 + i * 5000:3000 + i * 5000 + 2000] = seg
    return [_s(g)], [_s(g[3000 + 7 * 5000 - 1500:3000 + 7 * 5000 + 2000 + 1200])]


# ---- the edges ---------------------------------------------------------------------------------------------------------------
EDGE_NAMES = ("opens_query", "closes_query", "span_250", "span_251", "span_750", "span_751", "k_exceeds_candidates", "occ_4094_and_4095",
              "equal_occ", "least_frequent_comes_later", "one_absent_between", "longer_than_256", "longer_than_1024", "no_minimizer")
EDGE_PRESET = "map-ont"


@functools.lru_cache(maxsize=None)
def _edge_targets():
    """T0: 60 kb unique.  T1: 20 copies of the 8-kb master H, 15 more of H[2000:3000], 10 more of H[2400:2600] (occ 20 / 35 / 45 along H).
    T2: 4,095 copies of the 820-base master W between unique spacers, ONE of them with a substitution placed so that exactly one
    minimizer of W is missing from that copy: that minimizer has 4,094 occurrences, the others inside W have 4,095."""
    from oracle import binding as ob
    rng = np.random.default_rng(20261019)
    t0 = synth.random_seq(rng, 60_000)
    H = synth.random_seq(rng, 8000)
    sp = lambda: synth.random_seq(rng, 100)
    t1 = [sp()]
    for _ in range(20):
        t1 += [H, sp()]
    for _ in range(15):
        t1 += [H[2000:3000], sp()]
    for _ in range(10):
        t1 += [H[2400:2600], sp()]
    W = synth.random_seq(rng, 820)
    io, _ = preset(EDGE_PRESET)
    hw = set((ob.sketch(_s(W), io.k, io.w)[0] >> np.uint64(8)).tolist())
    Wm = None
    for p in range(300, 520):
        m = W.copy(); m[p] = synth.BASES[(int(np.searchsorted(synth.BASES, W[p])) + 1) % 4]
        hm = set((ob.sketch(_s(m), io.k, io.w)[0] >> np.uint64(8)).tolist())
        if len(hw - hm) == 1:
            Wm = m
            break
    assert Wm is not None
    t2 = [sp()]
    for i in range(4095):
        t2 += [Wm if i == 2000 else W, sp()]
    return t0, H, W, [_s(t0), _s(np.concatenate(t1)), _s(np.concatenate(t2))]


@functools.lru_cache(maxsize=None)
def edge_cases():
    """-> (targets, io, mo, mid_occ, cases): cases = list of dicts name, query, rescued (indices the restatement expects), occ, pos"""
    from oracle import binding as ob
    t0, H, W, targets = _edge_targets()
    io, mo = clamp_opts(EDGE_PRESET)
    oix = ob.OracleIndex(targets, io)
    counts = R.IndexCounts(oix)
    mid = oix.mid_occ(mo)
    assert mid == 10, mid
    F1, F2 = t0[10_000:11_500], t0[30_000:31_500]

    def info(q):
        res, occ, pos = R.rescued_of_query(_s(q), io, counts, mid)
        st = [(s, e) + R.stretch_bounds(pos, len(q), s, e) for s, e in R.stretches(occ, mid)]
        return res, occ, pos, st

    cases = []

    def add(name, q, check):
        res, occ, pos, st = info(q)
        assert check(res, occ, pos, st, len(q)), name
        cases.append(dict(name=name, query=_s(q), rescued=res, occ=occ, pos=pos, stretches=st))

    add("opens_query", np.concatenate([H[500:1800], F2]),
        lambda res, occ, pos, st, n: st[0][0] == 0 and st[0][2] == 0 and any(i < st[0][1] for i in res))
    add("closes_query", np.concatenate([F1, H[500:1800]]),
        lambda res, occ, pos, st, n: st[-1][1] == len(occ) and st[-1][3] == n and any(i >= st[-1][0] for i in res))

    def with_span(d):
        # F1 + H[3100:b] + F2: the piece's end moves until the one stretch spans exactly d query bases between its neighbours
        for a in range(3100, 3160):
            for b in range(a + d - 60, a + d + 10):
                q = np.concatenate([F1, H[a:b], F2])
                _, _, _, st = info(q)
                if len(st) == 1 and st[0][3] - st[0][2] == d:
                    return q
        raise AssertionError("no piece of H gives a stretch spanning %d" % d)

    for d, k in ((250, 0), (251, 1), (750, 1), (751, 2)):
        add("span_%d" % d, with_span(d), lambda res, occ, pos, st, n, d=d, k=k: st[0][3] - st[0][2] == d and len(res) == k == R.k_float(d))
    # across W: every minimizer inside has 4,095 occurrences but one, which has 4,094, and only that one may be rescued although k = 2
    q = np.concatenate([F1, W, F2])
    add("k_exceeds_candidates", q, lambda res, occ, pos, st, n: len(res) == int((occ[st[0][0]:st[0][1]] < R.MAX_OCC).sum()) < R.k_float(st[0][3] - st[0][2]))
    add("occ_4094_and_4095", q, lambda res, occ, pos, st, n: len(res) > 0 and all(occ[i] == 4094 for i in res) and (occ[st[0][0]:st[0][1]] == 4095).any())
    # every minimizer of H[4000:6000] has 20 occurrences: the earliest ones win
    add("equal_occ", np.concatenate([F1, H[4000:6000], F2]),
        lambda res, occ, pos, st, n: len(st) == 1 and len(set(occ[st[0][0]:st[0][1]])) == 1 and res == list(range(st[0][0], st[0][0] + len(res))) and len(res) >= 2)

    # H[2100:3000] has 35 and 45 occurrences, H[3000:3900] has 20: the rescued ones are NOT the first of the stretch
    add("least_frequent_comes_later", np.concatenate([F1, H[2100:3900], F2]),
        lambda res, occ, pos, st, n: len(st) == 1 and len(res) >= 2 and all(occ[i] == 20 for i in res) and occ[st[0][0]] > 20 and res[0] > st[0][0] + 50)

    def one_absent():
        base = np.concatenate([F1, H[500:3500], F2])
        for p in range(1500 + 1400, 1500 + 1700):
            for alt in b"ACGT":
                if base[p] == alt:
                    continue
                q = base.copy(); q[p] = alt
                _, occ, _, st = info(q)
                if len(st) == 2 and st[1][0] - st[0][1] == 1 and occ[st[0][1]] == 0:
                    return q
        raise AssertionError("no substitution leaves exactly one absent minimizer between two stretches")

    add("one_absent_between", one_absent(), lambda res, occ, pos, st, n: len(st) == 2 and st[1][0] == st[0][1] + 1 and occ[st[0][1]] == 0 and len(res) > 0)
    # (H[0:2000] then the occ-35 / occ-45 core: the arg-min has to pass over 20s that come earlier)
    add("longer_than_256", np.concatenate([F1, H[0:3500], F2]),
        lambda res, occ, pos, st, n: len(st) == 1 and 256 < st[0][1] - st[0][0] <= 1024 and len(res) == R.k_float(st[0][3] - st[0][2]) and len(set(occ[st[0][0]:st[0][1]])) >= 3)
    add("longer_than_1024", np.concatenate([F1, H, F2]),
        lambda res, occ, pos, st, n: len(st) == 1 and st[0][1] - st[0][0] > 1024 and len(res) == R.k_float(st[0][3] - st[0][2]) >= 10)
    cases.append(dict(name="no_minimizer", query="ACGTACG", rescued=[], occ=np.zeros(0, np.int64), pos=np.zeros(0, np.int64), stretches=[]))
    assert tuple(c["name"] for c in cases) == EDGE_NAMES
    return targets, io, mo, mid, cases
