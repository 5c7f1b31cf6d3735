"""The first stage at its kernel edges: a plain reference of the minimizer sketch and of the index build, and the table of
hand-built target sets aimed at the branch points of the sketch kernels (k_sketch, k_sketch32<., 9 | 4 | 0>, k_sketch_hpc), of
the homopolymer pre-pass (k_hpc_flags / k_hpc_scatter / k_hpc_seq_offsets), of the radix sort (radix.hip.h) and of the entry,
count and probe-table kernels of index_build_impl.  No GPU and no oracle in here.

Reference: brute_minimizers / brute_minimizers_hpc enumerate every window (the set definition); ref_index lays the targets'
minimizers out in the engine's global coordinates and sorts them stably by hash with Python's sorted; ref_mid_occ restates the
occurrence quantile.  tests/test_sketch_reference.py holds the reference to hand-derived answers and the oracle to the reference on
every case; tests/test_gpu_sketch_edges.py and tests/sketch_child.py hold the engine to it.

A case is (id, k, w, hpc, targets).  What a case claims to reach (a palindrome, a tie, a tile filled to the last slot, an exact
minimizer count for the sort, ...) is in claims()[id], a list of (kind, argument) that missed_claims() evaluates on the reference's
own output, so that a case which no longer reaches its edge fails on the CPU.

usage: python tests/sketch_edges.py   (prints every case with its sizes and what it claims)
"""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

from telr_amd import synth
from telr_amd.fasta import revcomp

TPAD = 16384             # mirrors TELR_TPAD (telr_amd/csrc/kernels.hip.h): padding between targets in global coordinates
TILE = 1024              # SK_TILE: slots per sketch tile
CHUNK = 64               # bases per chunk of the homopolymer pre-pass; 128 chunks per block of k_hpc_scatter
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}

PLAIN_FORMS = [(15, 10), (13, 5), (15, 7), (15, 1), (15, 2), (15, 32), (15, 33), (14, 10), (12, 5), (16, 10), (19, 19), (19, 40),
               (28, 10), (4, 3), (24, 10), (15, 255)]
CONTENT_FORMS = [(15, 10), (13, 5), (14, 10), (16, 10), (15, 33)]
HPC_FORMS = [(19, 10), (14, 5)]


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & mask
    return key


def brute_minimizers(seq, k, w):
    """(w,k)-minimizers by the set definition (Li 2018, section 2.1.1), all windows enumerated."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    mask = (1 << 2 * k) - 1
    ns = len(seq) - k + 1
    xs = []
    for u in range(ns):
        kmer = seq[u:u + k]
        if any(c not in code for c in kmer):
            xs.append(None); continue
        fw = 0
        for c in kmer:
            fw = fw << 2 | code[c]
        rv = 0
        for c in reversed(kmer):
            rv = rv << 2 | (3 - code[c])
        if fw == rv:
            xs.append(None); continue
        z = 0 if fw < rv else 1
        xs.append((_hash64(rv if z else fw, mask) << 8 | k, (u + k - 1) << 1 | z))
    sel = set()
    win = min(w, ns)
    for j in range(0, ns - win + 1):
        vals = [xs[q][0] for q in range(j, j + win) if xs[q] is not None]
        if not vals:
            continue
        m = min(vals)
        for q in range(j, j + win):
            if xs[q] is not None and xs[q][0] == m:
                sel.add(q)
    return [(xs[q][0], xs[q][1]) for q in sorted(sel)]


def brute_minimizers_hpc(seq, k, w):
    """homopolymer-compressed variant: k-mers over runs, span in original bases, position = last base of the last run"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    runs = []
    i = 0
    while i < len(seq):
        j = i + 1
        while j < len(seq) and (seq[j] == seq[i] or (seq[j] not in code and seq[i] not in code)):
            j += 1
        runs.append((seq[i], i, j - 1)); i = j
    mask = (1 << 2 * k) - 1
    ns = len(runs) - k + 1
    xs = []
    for u in range(ns):
        rr = runs[u:u + k]
        span = rr[-1][2] - rr[0][1] + 1
        if any(c not in code for c, _, _ in rr) or span >= 256:
            xs.append(None); continue
        fw = 0
        for c, _, _ in rr:
            fw = fw << 2 | code[c]
        rv = 0
        for c, _, _ in reversed(rr):
            rv = rv << 2 | (3 - code[c])
        if fw == rv:
            xs.append(None); continue
        z = 0 if fw < rv else 1
        xs.append((_hash64(rv if z else fw, mask) << 8 | span, rr[-1][2] << 1 | z))
    sel = set()
    win = min(w, ns)
    for j in range(0, ns - win + 1):
        vals = [xs[q][0] for q in range(j, j + win) if xs[q] is not None]
        if not vals:
            continue
        m = min(vals)
        for q in range(j, j + win):
            if xs[q] is not None and xs[q][0] == m:
                sel.add(q)
    return [(xs[q][0], xs[q][1]) for q in sorted(sel)]


@functools.lru_cache(maxsize=None)
def brute(seq, k, w, hpc):
    """either form, computed once per (sequence, form) of a process: the tests share it and leave it unchanged"""
    return tuple((brute_minimizers_hpc if hpc else brute_minimizers)(seq, k, w))


def target_offsets(lens):
    """the engine's coordinate rule: goff[i + 1] = (goff[i] + len + TPAD + 63) & ~63"""
    g = [0]
    for n in lens:
        g.append((g[-1] + n + TPAD + 63) & ~63)
    return g


def ref_index(targets, k, w, hpc):
    """-> (ent_hash u64 [n_ent], ent_off u32 [n_ent + 1], pos u32 [n_mz], n_mz, n_ent): the per-target minimizers in target order,
    positions in global coordinates, sorted STABLY by hash = x >> 8 (so that pos ascends inside a hash)"""
    goff = target_offsets([len(t) for t in targets])
    mz = []
    for t, g in zip(targets, goff):
        for x, y in brute(t, k, w, hpc):
            mz.append((int(x), int(y) + (g << 1)))
    mz = sorted(mz, key=lambda m: m[0] >> 8)
    ent_hash, ent_off = [], []
    for i, (x, _) in enumerate(mz):
        if i == 0 or x >> 8 != mz[i - 1][0] >> 8:
            ent_hash.append(x >> 8); ent_off.append(i)
    ent_off.append(len(mz))
    return (np.array(ent_hash, np.uint64), np.array(ent_off, np.uint32), np.array([y for _, y in mz], np.uint32), len(mz), len(ent_hash))


def ref_mid_occ(counts, mo):
    """the occurrence cut-off: the (1 - f) quantile of the distinct minimizers' counts, + 1, clamped to [min_mid_occ, max_mid_occ]
    (the upper clamp only where it lies above the lower); min_mid_occ for an index without entries"""
    n = len(counts)
    if n == 0:
        occ = mo.min_mid_occ
    else:
        idx = int((1.0 - float(mo.mid_occ_frac)) * float(n))
        if idx >= n:
            idx = n - 1
        occ = int(sorted(int(c) for c in counts)[idx]) + 1
    if occ < mo.min_mid_occ:
        occ = mo.min_mid_occ
    if mo.max_mid_occ > mo.min_mid_occ and occ > mo.max_mid_occ:
        occ = mo.max_mid_occ
    return occ


# ---- what a case reaches, from plain restatements of their own ------------------------------------------------------------------
def hpc_runs(seq):
    """(base, first, last) of every run; consecutive ambiguous bases are one run"""
    runs, i = [], 0
    while i < len(seq):
        j = i + 1
        while j < len(seq) and (seq[j] == seq[i] or (seq[j] not in CODE and seq[i] not in CODE)):
            j += 1
        runs.append((seq[i], i, j - 1)); i = j
    return runs


def n_slots(seq, k, hpc):
    return (len(hpc_runs(seq)) if hpc else len(seq)) - k + 1


def slot_kmers(seq, k, hpc):
    """per slot: (the k bases or run bases, span)"""
    if not hpc:
        return [(seq[u:u + k], k) for u in range(len(seq) - k + 1)]
    r = hpc_runs(seq)
    return [("".join(c for c, _, _ in r[u:u + k]), r[u + k - 1][2] - r[u][1] + 1) for u in range(len(r) - k + 1)]


def n_palindromes(seq, k, hpc=0):
    return sum(1 for km, _ in slot_kmers(seq, k, hpc) if all(c in CODE for c in km) and km == revcomp(km))


def slot_values(seq, k, hpc=0):
    """hash of every slot's canonical k-mer, None for a slot without one (N, palindrome, span >= 256)"""
    mask, out = (1 << 2 * k) - 1, []
    for km, span in slot_kmers(seq, k, hpc):
        if any(c not in CODE for c in km) or km == revcomp(km) or span >= 256:
            out.append(None); continue
        fw = int("".join(str(CODE[c]) for c in km), 4); rv = int("".join(str(CODE[c]) for c in revcomp(km)), 4)
        out.append(_hash64(min(fw, rv), mask) << 8 | span)
    return out


def has_tie(seq, k, w, hpc=0):
    """some window whose minimum is held by more than one slot"""
    xs = slot_values(seq, k, hpc)
    win = min(w, len(xs))
    for j in range(0, len(xs) - win + 1):
        v = [x for x in xs[j:j + win] if x is not None]
        if v and v.count(min(v)) > 1:
            return True
    return False


def missed_claims(case):
    """every claim of the case that the reference's output does not bear out (empty: the case reaches its edges)"""
    cid, k, w, hpc, targets = case
    cnt = [len(brute(t, k, w, hpc)) for t in targets]
    ns = [n_slots(t, k, hpc) for t in targets]
    bad = []
    for kind, arg in claims()[cid]:
        if kind == "n_mz" and sum(cnt) != arg:
            bad.append("n_mz %d, not %d" % (sum(cnt), arg))
        elif kind == "n_mz_min" and sum(cnt) < arg:
            bad.append("n_mz %d < %d" % (sum(cnt), arg))
        elif kind == "n_mz_max" and not 0 < sum(cnt) <= arg:
            bad.append("n_mz %d not in 1 .. %d" % (sum(cnt), arg))
        elif kind == "slots" and ns != list(arg):
            bad.append("slots %s, not %s" % (ns, list(arg)))
        elif kind == "all_selected" and not (ns[arg] >= TILE and cnt[arg] == ns[arg]):
            bad.append("target %d: %d of %d slots selected" % (arg, cnt[arg], ns[arg]))
        elif kind == "none_selected" and not (ns[arg] > 0 and cnt[arg] == 0):
            bad.append("target %d: %d minimizers in %d slots" % (arg, cnt[arg], ns[arg]))
        elif kind == "empty" and not (sum(cnt) == 0 and max(ns) <= 0):
            bad.append("not empty")
        elif kind == "palindromes" and not n_palindromes(targets[arg[0]], k, hpc) >= arg[1]:
            bad.append("target %d: %d palindromes" % (arg[0], n_palindromes(targets[arg[0]], k, hpc)))
        elif kind == "tie" and not has_tie(targets[arg], k, w, hpc):
            bad.append("target %d: no tie" % arg)
        elif kind == "span":
            t, span, valid = arg
            sp = [x for _, x in slot_kmers(targets[t], k, hpc)]
            if sp.count(span) != k or max(sp) != span:
                bad.append("target %d: %d slots of span %d, widest %d" % (t, sp.count(span), span, max(sp)))
            picked = sum(1 for x, _ in brute(targets[t], k, w, hpc) if (x & 0xff) == (span & 0xff) and span > k)
            if valid != (picked > 0):
                bad.append("target %d: %d minimizers of span %d" % (t, picked, span))
        elif kind == "runs" and len(hpc_runs(targets[arg[0]])) != arg[1]:
            bad.append("target %d: %d runs, not %d" % (arg[0], len(hpc_runs(targets[arg[0]])), arg[1]))
        elif kind == "run_at":
            t, first, last = arg
            if not any(a == first and b == last for _, a, b in hpc_runs(targets[t])):
                bad.append("target %d: no run %d .. %d" % (t, first, last))
        elif kind == "last_run_long":
            r = hpc_runs(targets[arg])
            last_end = max((y >> 1 for _, y in brute(targets[arg], k, w, hpc)), default=-1)
            if not (r[-1][2] > r[-1][1] and last_end == len(targets[arg]) - 1):
                bad.append("target %d: the last k-mer is no minimizer ending in a multi-base run" % arg)
    return bad


# ---- building blocks -------------------------------------------------------------------------------------------------------
def rnd(rng, n):
    return bytes(synth.random_seq(rng, n)).decode()


def no_repeat(rng, n):
    """n bases, each drawn from the three that differ from the one before (no run longer than one base, no fixed period)"""
    if n <= 0:
        return ""
    step = 1 + rng.integers(0, 3, n)
    step[0] = rng.integers(0, 4)
    return "".join("ACGT"[c] for c in np.cumsum(step) % 4)


def runs_seq(rng, nruns):
    """a sequence of exactly nruns runs, of 1 .. 3 bases each"""
    return "".join(b * int(n) for b, n in zip(no_repeat(rng, nruns), rng.integers(1, 4, max(nruns, 0))))


def put(s, at, what):
    return s[:at] + what + s[at + len(what):]


def length_set(rng, k, w):
    """targets of these slot counts, in this order: the empty and too-short ones sit between tiled ones (tile_seq, targets without
    a tile, goff)"""
    ns = [-1, None, 1, w - 1, w, w + 1, TILE - 1, TILE, TILE + 1, TILE + w - 1, 2 * TILE, 2 * TILE + 1]
    want = [-k + 1 if n is None else n for n in ns]
    return [rnd(rng, 0 if n is None else n + k - 1) for n in ns], want


_CACHE = {}


def _table():
    if _CACHE:
        return _CACHE["cases"], _CACHE["claims"]
    cases, cl = [], {}

    def add(k, w, hpc, name, targets, claim):
        cid = "k%dw%d%s-%s" % (k, w, "h" if hpc else "", name)
        assert cid not in cl, cid
        cases.append((cid, k, w, hpc, list(targets))); cl[cid] = list(claim)

    # -- every form at the lengths where a tile, a window or a target begins and ends
    for f, (k, w) in enumerate(PLAIN_FORMS):
        rng = np.random.default_rng(1000 + f)
        tg, want = length_set(rng, k, w)
        add(k, w, 0, "lengths", tg, [("slots", want), ("n_mz_min", 50)])
    for f, (k, w) in enumerate(CONTENT_FORMS):
        _content_cases(add, np.random.default_rng(2000 + f), k, w)
    for f, (k, w) in enumerate(HPC_FORMS):
        _hpc_cases(add, np.random.default_rng(3000 + f), k, w)
    _sort_cases(add, np.random.default_rng(4000))
    _CACHE["cases"], _CACHE["claims"] = cases, cl
    return cases, cl


def _content_cases(add, rng, k, w):
    # an N as first base, as last base, and one N at each base 1023 .. 1024 + k - 1 (one target per position: every slot around
    # the tile seam is killed in turn)
    L = TILE + 2 * k + w + 20
    base = rnd(rng, L)
    tg = [put(base, 0, "N"), put(base, L - 1, "N")] + [put(base, p, "N") for p in range(TILE - 1, TILE + k)]
    add(k, w, 0, "n_at_seam", tg, [("n_mz_min", 40 * len(tg))])
    # homopolymers of 1,024 and 1,025 slots: every slot ties, every slot is selected, a tile's staging area is full
    if k % 2:
        tg = ["A" * (TILE + k - 1), "C" * (TILE + 1 + k - 1)]
        add(k, w, 0, "homopolymer", tg, [("all_selected", 0), ("all_selected", 1), ("n_mz", 2 * TILE + 1), ("tie", 0)])
    # tandem repeats of period 2, 3 and 4 laid across slot 1,024 (190 slots: slots 930 .. 1,119)
    tg = [rnd(rng, 930) + (unit * 80)[:190 + k - 1] + rnd(rng, 300) for unit in ("AG", "ACT", "AACG")]
    add(k, w, 0, "tandem", tg, [("tie", 0), ("tie", 1), ("tie", 2)])
    if k % 2 == 0:
        n = (TILE + 76 + k - 1) // 2
        h1, h2 = rnd(rng, k // 2), rnd(rng, k // 2)
        planted = put(put(rnd(rng, TILE + 200 + k), 1000, h1 + revcomp(h1)), 1040, h2 + revcomp(h2))
        tg = ["AT" * n, "ACGT" * (n // 2), planted]
        add(k, w, 0, "palindromes", tg, [("none_selected", 0), ("palindromes", (0, TILE + 1)), ("palindromes", (1, TILE // 2)),
                                         ("palindromes", (2, 2))])
    # every target shorter than k: the empty index
    add(k, w, 0, "empty_index", ["", rnd(rng, k - 1), "ACG", rnd(rng, 1)], [("empty", None)])


def _hpc_cases(add, rng, k, w):
    ns = [-1, 1, w, w + 1, TILE - 1, TILE, TILE + 1]
    tg = [runs_seq(rng, n + k - 1) for n in ns]
    add(k, w, 1, "run_counts", tg, [("slots", ns), ("n_mz_min", 300)] + [("runs", (i, n + k - 1)) for i, n in enumerate(ns)])
    # chunk seams (chunks of 64 bases from the target's start)
    a = put(no_repeat(rng, 400), 58, "G" + "A" * 11 + "C")                    # a run of 11 across the seam at 64: bases 59 .. 69
    b = put(no_repeat(rng, 400), 62, "GTTC")                                  # base 64 repeats base 63: no run starts at the chunk start
    b = put(b, 126, "GATTTC")                                                 # base 128 starts a run of 3 and differs from base 127
    c = put(no_repeat(rng, 400), 60, "G" + "N" * 7 + "C")                     # an N run across the seam: bases 61 .. 67
    c = put(c, 200, "GAAANNAAAC")                                             # Ns between two runs of the same base
    c = put(c, 300, "GNTTTG")                                                 # an N in front of a run
    for _ in range(400):                                                      # the last k-mer ends in a multi-base run, and is a minimizer
        d = no_repeat(rng, 300) + "GTTTT"
        if max((y >> 1 for _, y in brute(d, k, w, 1)), default=-1) == len(d) - 1:
            break
    add(k, w, 1, "chunk_seams", [a, b, c, d], [("run_at", (0, 59, 69)), ("run_at", (1, 63, 64)), ("run_at", (1, 128, 130)),
                                               ("run_at", (2, 61, 67)), ("run_at", (2, 201, 203)), ("run_at", (2, 204, 205)),
                                               ("run_at", (2, 206, 208)), ("run_at", (2, 301, 301)), ("run_at", (2, 302, 304)),
                                               ("run_at", (3, 301, 304)), ("last_run_long", 3), ("n_mz_min", 100)])
    add(k, w, 1, "chunk_lengths", [rnd(rng, n) for n in (63, 64, 65, 128, 8192)], [("n_mz_min", 500)])
    # 8,192 bases without two equal neighbours: 8,192 runs from the first 128 chunks, the LDS slots of a k_hpc_scatter block exactly
    head = no_repeat(rng, 8192)
    tail = rnd(rng, 300)
    if tail[0] == head[-1]:
        tail = "ACGT"[(CODE[tail[0]] + 1) % 4] + tail[1:]
    add(k, w, 1, "lds_full", [head + tail], [("n_mz_min", 1000)])
    # k runs spanning exactly 255 (the widest valid k-mer) and 256 bases: one long run among single-base runs
    tg = []
    for span in (255, 256):
        s = no_repeat(rng, 700)
        r = span - (k - 1)
        other = [x for x in "ACGT" if x not in (s[299], s[300 + r])][0]
        tg.append(put(s, 300, other * r))
    add(k, w, 1, "span_255_256", tg, [("span", (0, 255, True)), ("span", (1, 256, False)), ("run_at", (0, 300, 300 + 255 - k)),
                                      ("run_at", (1, 300, 300 + 256 - k))])


def _sort_cases(add, rng):
    k, w = 15, 10
    add(k, w, 0, "sort_nmz_1", [rnd(rng, k)], [("n_mz", 1)])
    # 2,047 / 2,048 / 2,049 minimizers (one radix tile less one, exactly, plus one): a random target's count topped up by a homopolymer
    r6 = rnd(rng, 6000)
    m = len(brute(r6, k, w, 0))
    for d in (-1, 0, 1):
        add(k, w, 0, "sort_nmz_%d" % (2048 + d), [r6, "T" * (2048 - m + d + k - 1)], [("n_mz", 2048 + d)])
    add(k, w, 0, "sort_nmz_gt4096", [rnd(rng, 30000)], [("n_mz_min", 4097)])
    add(k, w, 0, "sort_nmz_lt256", [rnd(rng, 600)], [("n_mz_max", 255)])
    # at least 65,536 minimizers (the 32-bit count sort): ~25 kb of random sequence and a homopolymer of 66,000 slots, the largest
    # input of the table (the brute form takes about a second for it, so its reference is the brute form like every other case's)
    add(k, w, 0, "sort_nmz_65536", [rnd(rng, 25000), "G" * (66000 + k - 1)], [("n_mz_min", 66000 + 4000)])
    # 4-mers: the whole key space in one radix pass, few entries with huge counts
    add(4, 3, 0, "keyspace_20kb", [rnd(rng, 20000)], [("n_mz_min", 5000)])


def cases():
    """-> [(id, k, w, hpc, targets)]"""
    return _table()[0]


def claims():
    """-> {id: [(kind, argument)]}, see missed_claims"""
    return _table()[1]


def forms():
    """every (k, w, hpc) of the table"""
    return [(k, w, 0) for k, w in PLAIN_FORMS] + [(k, w, 1) for k, w in HPC_FORMS]


def query_set(k, w, hpc):
    """the targets that are mapped against their own index (query side and probe table): the form's length / run-count set, and
    for the content forms its tandem stretches (190 slots each), its first three N targets and its planted
    palindromes; no homopolymers.  Plus three queries that share nothing with them."""
    by_id = {c[0]: c[4] for c in cases()}
    pre = "k%dw%d%s-" % (k, w, "h" if hpc else "")
    tg = list(by_id[pre + ("run_counts" if hpc else "lengths")])
    if hpc:
        tg += by_id[pre + "chunk_seams"] + by_id[pre + "span_255_256"]
    if (k, w) in CONTENT_FORMS and not hpc:
        tg += by_id[pre + "tandem"] + by_id[pre + "n_at_seam"][:3]
        if k % 2 == 0:
            tg += by_id[pre + "palindromes"][2:]
    # the foreign queries: random, drawn again until none of their minimizer hashes occurs in the set (short k-mers collide by
    # chance); every valid 4-mer occurs in any set, so for k = 4 they are queries without a minimizer: palindromes, Ns, too short
    if k == 4:
        return tg, ["AT" * 350, "N" * 1500, "ACG"]
    have = {x >> 8 for t in tg for x, _ in brute(t, k, w, hpc)}
    for attempt in range(100):
        rng = np.random.default_rng(5000 + 100 * k + w + 7919 * attempt)
        foreign = [rnd(rng, n) for n in (700, 1500, 2600)]
        if not have & {x >> 8 for q in foreign for x, _ in brute(q, k, w, hpc)}:
            return tg, foreign
    raise AssertionError("no foreign queries for k=%d w=%d" % (k, w))


def reference(case):
    """ref_index of a case"""
    cid, k, w, hpc, targets = case
    return ref_index(targets, k, w, hpc)


def mid_occ_options():
    """the map-ont options, and mid_occ_frac 0 and 1 with and without a lower clamp that hides the quantile"""
    from telr_amd.presets import preset
    out = [preset("map-ont")[1]]
    for frac in (0.0, 1.0):
        for lo in (10, 1):
            mo = preset("map-ont")[1]
            mo.mid_occ_frac = frac; mo.min_mid_occ = lo
            out.append(mo)
    return out


def check_index(engine, case, ref):
    """engine.index(targets) against ref_index, array for array; -> (n_mz, n_ent).  pos in order shows both the selection and the
    stability of the sort."""
    from telr_amd._abi import IdxOpt
    cid, k, w, hpc, targets = case
    ent_hash, ent_off, pos, n_mz, n_ent = ref
    ix = engine.index(targets, IdxOpt(k=k, w=w, is_hpc=hpc, bucket_bits=0))
    try:
        assert ix.stats() == (n_mz, n_ent), (cid, ix.stats(), (n_mz, n_ent))
        eh, eo, p = ix.debug_dump()
        np.testing.assert_array_equal(p, pos, err_msg=cid + ": pos")
        np.testing.assert_array_equal(eh, ent_hash, err_msg=cid + ": ent_hash")
        np.testing.assert_array_equal(eo, ent_off, err_msg=cid + ": ent_off")
        assert (np.diff(eh.astype(np.int64)) > 0).all(), cid + ": ent_hash not strictly ascending"
        assert int(eo[0]) == 0 and int(eo[-1]) == n_mz, (cid, int(eo[0]), int(eo[-1]))
        counts = np.diff(ent_off.astype(np.int64))
        for mo in mid_occ_options():
            assert ix.debug_mid_occ(mo) == ref_mid_occ(counts, mo), (cid, mo.mid_occ_frac, mo.min_mid_occ)
    finally:
        ix.free(); ix.targets.free()
    return n_mz, n_ent


if __name__ == "__main__":
    tot = {}
    for c in cases():
        cid, k, w, hpc, tg = c
        n = sum(len(brute(t, k, w, hpc)) for t in tg)
        tot.setdefault((k, w, hpc), [0, 0]); tot[(k, w, hpc)][0] += 1; tot[(k, w, hpc)][1] += n
        print("%-32s %2d targets %7d bases %6d minimizers  %s" % (cid, len(tg), sum(len(t) for t in tg), n, "; ".join(missed_claims(c)) or "ok"))
    for f, (nc, n) in tot.items():
        print("form k=%d w=%d hpc=%d: %d cases, %d minimizers" % (f + (nc, n)))
