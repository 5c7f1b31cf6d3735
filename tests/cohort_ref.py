"""The definition of telr_merge_sites (include/telr_hip.h) as plain Python: sorts and loops over tuples, sharing no code
with the engine.  Several samples' insertion calls -> clusters -> one site list; an own definition, not bcftools merge, SURVIVOR or Jasmine.
An entry is a (tid, pos, len, sample, group) tuple; `merge` returns dict(sites = [dict per site, SITE_FIELDS], members = [[input index,
...] per site, in key order], samples = [[sample, ...] per site, ascending]).  `generate` builds the seeded cohort of the tests (and,
scaled up, of tools/cohort_time.py); `coverage` counts what the generated case has to contain."""
import numpy as np

E_ARG, E_RANGE = -3, -4
MAX_ENTRIES = (1 << 31) - 16
SHADOWED, CROWDED = 1, 2
ENTRY_FIELDS = ("tid", "pos", "len", "sample", "group")
SITE_FIELDS = ("tid", "pos", "len", "group", "n_samples", "n_members", "n_sized", "len_min", "len_max", "pos_min", "pos_max", "rep", "flags", "winner")
DEFAULTS = dict(dist=50, min_samples=1, reserved0=0, reserved1=0)


def options(opt=None):
    o = dict(DEFAULTS)
    for k, v in (opt or {}).items():
        if k not in o:
            raise TypeError("no option %r" % k)
        o[k] = int(v)
    return o


def refusal(entries, n, n_targets, opt=None):
    """-> (code, text) when telr_merge_sites refuses (entries None: a null pointer; n: the count given, read before the array), else None"""
    o = options(opt)
    if n < 0:
        return E_ARG, "negative n"
    if n > 0 and entries is None:
        return E_ARG, "null entries"
    if o["dist"] < 0:
        return E_ARG, "negative dist"
    if o["min_samples"] < 1:
        return E_ARG, "min_samples below 1"
    if o["reserved0"] or o["reserved1"]:
        return E_ARG, "non-zero reserved field"
    if n >= MAX_ENTRIES:
        return E_RANGE, "too many entries"
    for i in range(n):
        tid, pos, ln, sample, group = entries[i]
        if tid < 0 or tid >= n_targets:
            return E_ARG, "entry %d: tid outside n_targets" % i
        for name, v in (("pos", pos), ("len", ln), ("sample", sample), ("group", group)):
            if v < 0:
                return E_ARG, "entry %d: negative %s" % (i, name)
    return None


def merge(entries, opt=None):
    o = options(opt)
    dist, min_samples = o["dist"], o["min_samples"]
    E = [tuple(int(x) for x in e) for e in entries]
    order = sorted(range(len(E)), key=lambda i: (E[i][0], E[i][4], E[i][1], E[i][3], E[i][2], i))
    clusters = []
    for i in order:
        tid, pos, _, _, group = E[i]
        if clusters:
            p = E[clusters[-1][-1]]
            if p[0] == tid and p[4] == group and pos - p[1] <= dist:
                clusters[-1].append(i)
                continue
        clusters.append([i])
    found = []
    for mem in clusters:
        m = len(mem)
        first, mid = E[mem[0]], mem[(m - 1) // 2]
        samples = sorted(set(E[i][3] for i in mem))
        sized = sorted((i for i in mem if E[i][2] > 0), key=lambda i: (E[i][2], E[i][3], i))
        s = dict(tid=first[0], group=first[4], pos=E[mid][1], pos_min=first[1], pos_max=E[mem[-1]][1], n_members=m, n_samples=len(samples), n_sized=len(sized),
                 len=0, len_min=0, len_max=0, rep=mid, flags=0, winner=-1)
        if sized:
            r = sized[(len(sized) - 1) // 2]
            s.update(len=E[r][2], rep=r, len_min=E[sized[0]][2], len_max=E[sized[-1]][2])
        if s["n_samples"] >= min_samples:
            found.append((s, mem, samples))
    found.sort(key=lambda x: (x[0]["tid"], x[0]["pos"], -x[0]["n_samples"], -x[0]["n_members"], x[0]["group"]))
    sites = [x[0] for x in found]
    for k, s in enumerate(sites):
        if k > 0 and (sites[k - 1]["tid"], sites[k - 1]["pos"]) == (s["tid"], s["pos"]):
            s["flags"] = SHADOWED
            s["winner"] = k - 1 if sites[k - 1]["winner"] < 0 else sites[k - 1]["winner"]
    open_ = [k for k, s in enumerate(sites) if not s["flags"] & SHADOWED]
    for r, k in enumerate(open_):
        s = sites[k]
        near = False
        if r > 0:
            b = sites[open_[r - 1]]
            near = b["tid"] == s["tid"] and s["pos"] - b["pos"] <= dist
        if r + 1 < len(open_):
            b = sites[open_[r + 1]]
            near = near or (b["tid"] == s["tid"] and b["pos"] - s["pos"] <= dist)
        if near:
            s["flags"] |= CROWDED
    return dict(sites=sites, members=[x[1] for x in found], samples=[x[2] for x in found])


def site_list(result):
    """the (tid, pos, len) triples of the sites that are not shadowed"""
    return [(s["tid"], s["pos"], s["len"]) for s in result["sites"] if not s["flags"] & SHADOWED]


def arrays(result):
    """-> {field: int32 array} of the sites, member_off / sample_off (int64), members / samples (int32)"""
    out = {f: np.array([s[f] for s in result["sites"]], np.int32) for f in SITE_FIELDS}
    for name in ("members", "samples"):
        off = np.zeros(len(result["sites"]) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in result[name]], dtype=np.int64)
        out[name[:-1] + "_off"] = off
        out[name] = np.array([v for x in result[name] for v in x], np.int32)
    return out


def generate(seed=20261021, target_lens=(400000, 300000, 900000), n_groups=4, n_samples=40, n_loci=480, plants=True, shuffle=True):
    """A seeded cohort -> list of entries.  n_loci loci, each with a target, a position, a group, a length and a carrier frequency: every
    sample that carries one gives an entry a few bases off, a fifth of them without a length.  plants (three targets, four groups): the
    structures the tests need whatever the seed --
      * 30 positions shared exactly by two or three groups (shadowed sites, decided at every level of the final key),
      * 30 pairs of groups 20 bases apart (crowded sites),
      * one chain of 600 entries three bases apart (one cluster above 512 members),
      * 600 single entries of one sample 1,000 bases apart, alone in their (target, group): consecutive clusters that min_samples = 2
        drops, so that at least one whole block of 256 lanes keeps nothing wherever the run starts,
      * 40 loci none of whose entries has a length."""
    rng = np.random.default_rng(seed)
    nt = len(target_lens)
    E = []
    for _ in range(n_loci):
        tid = int(rng.integers(0, nt))
        pos = int(rng.integers(1000, target_lens[tid] - 1000))
        group, ln, freq = int(rng.integers(0, n_groups)), int(rng.integers(100, 8000)), float(rng.beta(0.5, 1.5))
        for s in np.nonzero(rng.random(n_samples) < freq)[0]:
            E.append((tid, pos + int(rng.integers(-8, 9)), 0 if rng.random() < 0.2 else ln + int(rng.integers(-20, 21)), int(s), group))
    if plants:
        assert nt >= 3 and n_groups >= 4 and n_samples >= 8
        base = [target_lens[t] + 10000 for t in range(nt)]          # behind the loci: a planted structure meets nothing else
        for k in range(30):                                           # shared positions on target 0
            pos = base[0] + 1000 * k
            groups = (0, 1, 2) if k % 3 == 0 else (1, 3)
            for j, g in enumerate(groups):
                carriers = 3 if k % 5 == 0 else 3 + j               # k % 5 == 0: equal n_samples; then members (k % 10 == 0: equal too, the group decides)
                for s in range(carriers):
                    E.append((0, pos, 300 + s, int((s + k) % n_samples), g))
                if k % 5 == 0 and k % 10 != 0 and j == 1:
                    E.append((0, pos, 0, int(k % n_samples), g))      # one sample twice: more members, as many samples
        for k in range(30):                                           # pairs of groups 20 apart on target 1
            pos = base[1] + 1000 * k
            for s in range(2):
                E.append((1, pos, 500, s, 0))
                E.append((1, pos + 20, 700, s + 2, 2))
        for k in range(600):                                          # one chain on target 1, group 1
            E.append((1, base[1] + 100000 + 3 * k, 0 if k % 7 == 0 else 1000 + k % 50, k % n_samples, 1))
        for k in range(600):                                          # single entries, alone on (target 2, group 3)
            E.append((2, base[2] + 1000 * k, 250, 5, 3))
        for k in range(40):                                           # loci without a length on target 2, group 0
            for s in range(1 + k % 3):
                E.append((2, base[2] + 1000 * k + s, 0, 7 + s, 0))
        E = [e for e in E if not (e[0] == 2 and e[4] == 3 and e[3] != 5)]      # (target 2, group 3) holds the single entries only
    if shuffle:
        E = [E[i] for i in rng.permutation(len(E))]
    return E


def coverage(entries, opt=None):
    """what the generated case must contain, counted on this module's answer: shadowed and crowded sites, the largest cluster, the longest
    run of consecutive clusters (in key order) that min_samples = 2 drops, sites with and without a sized member"""
    o = options(opt)
    one = merge(entries, dict(o, min_samples=1))
    run = best = 0
    for s in sorted(one["sites"], key=lambda s: (s["tid"], s["group"], s["pos_min"])):          # the clusters in key order
        run = run + 1 if s["n_samples"] < 2 else 0
        best = max(best, run)
    return dict(entries=len(entries), sites=len(one["sites"]), shadowed=sum(1 for s in one["sites"] if s["flags"] & SHADOWED),
                crowded=sum(1 for s in one["sites"] if s["flags"] & CROWDED), largest=max(s["n_members"] for s in one["sites"]), dropped_run=best,
                sized=sum(1 for s in one["sites"] if s["n_sized"] > 0), unsized=sum(1 for s in one["sites"] if s["n_sized"] == 0))
