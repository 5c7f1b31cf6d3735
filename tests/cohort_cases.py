"""Hand-built entries for telr_merge_sites, one case per rule of its definition, each with the sites, member lists and sample lists worked
out by hand and a claim: the edge it is there for, asserted on its own data (tests/test_cohort_ref.py holds tests/cohort_ref.py to the hand
answers and checks the claims; tests/test_gpu_cohort.py holds the engine to cohort_ref on the same cases and on the generated one)."""
from cohort_ref import E_ARG, E_RANGE, MAX_ENTRIES, SITE_FIELDS, generate

N_TARGETS = 3
TOP = (1 << 31) - 1
SIZES = (255, 256, 257, 2047, 2048, 2049)          # around the 256-lane block and the 2,048-key radix tile


def S(tid, pos, ln, group, n_samples, n_members, n_sized, len_min, len_max, pos_min, pos_max, rep, flags=0, winner=-1):
    return dict(zip(SITE_FIELDS, (tid, pos, ln, group, n_samples, n_members, n_sized, len_min, len_max, pos_min, pos_max, rep, flags, winner)))


def case(name, entries, opt, sites, members, samples, claim):
    return dict(name=name, entries=entries, opt=opt, sites=sites, members=members, samples=samples, claim=claim)


def flags(c):
    return [s["flags"] for s in c["sites"]]


def hand_cases():
    """-> list of dict(name, entries [(tid, pos, len, sample, group)], opt, sites, members, samples, claim: case -> bool)"""
    C = []
    C.append(case("n_0", [], {}, [], [], [], lambda c: len(c["entries"]) == 0))
    C.append(case("n_1", [(0, 100, 60, 3, 0)], {}, [S(0, 100, 60, 0, 1, 1, 1, 60, 60, 100, 100, 0)], [[0]], [[3]], lambda c: len(c["entries"]) == 1))
    # 150 - 100 = dist: one cluster; 201 - 150 = dist + 1: a new one.  Two members, none sized: pos and rep are member 0's
    C.append(case("gap_dist_and_dist_plus_1", [(0, 100, 0, 0, 0), (0, 150, 0, 1, 0), (0, 201, 0, 2, 0)], {},
                  [S(0, 100, 0, 0, 2, 2, 0, 0, 0, 100, 150, 0), S(0, 201, 0, 0, 1, 1, 0, 0, 0, 201, 201, 2)], [[0, 1], [2]], [[0, 1], [2]],
                  lambda c: c["entries"][1][1] - c["entries"][0][1] == 50 and c["entries"][2][1] - c["entries"][1][1] == 51 and len(c["sites"]) == 2))
    # dist 0: equal positions merge, one base apart does not -- and is not crowded either
    C.append(case("dist_0", [(0, 100, 0, 0, 0), (0, 100, 0, 1, 0), (0, 101, 0, 2, 0)], dict(dist=0),
                  [S(0, 100, 0, 0, 2, 2, 0, 0, 0, 100, 100, 0), S(0, 101, 0, 0, 1, 1, 0, 0, 0, 101, 101, 2)], [[0, 1], [2]], [[0, 1], [2]],
                  lambda c: c["opt"]["dist"] == 0 and flags(c) == [0, 0]))
    # dist = 2^31 - 1: previous pos + dist (5 + 2^31 - 1) and pos + dist at the crowding test do not fit 32 bits.  5 and 2^31 - 1 are one
    # cluster; the site of group 1 at 2^31 - 2 and that one at 5 are 2^31 - 7 apart: both crowded
    C.append(case("wrap_at_2_31", [(0, 5, 0, 0, 0), (0, TOP, 0, 1, 0), (0, TOP - 1, 0, 0, 1)], dict(dist=TOP),
                  [S(0, 5, 0, 0, 2, 2, 0, 0, 0, 5, TOP, 0, 2), S(0, TOP - 1, 0, 1, 1, 1, 0, 0, 0, TOP - 1, TOP - 1, 2, 2)], [[0, 1], [2]], [[0, 1], [0]],
                  lambda c: c["entries"][0][1] + c["opt"]["dist"] >= 1 << 31 and c["sites"][0]["pos_max"] == TOP and flags(c) == [2, 2]))
    # one cluster = the whole input, given out of order: key order 1, 3, 2, 4, 0; five members -> member 2 (pos 120); three sized,
    # (100, s4, i0), (200, s2, i2), (300, s1, i3) -> the second
    C.append(case("one_cluster_whole_input", [(0, 140, 100, 4, 0), (0, 100, 0, 0, 0), (0, 120, 200, 2, 0), (0, 110, 300, 1, 0), (0, 130, 0, 3, 0)], {},
                  [S(0, 120, 200, 0, 5, 5, 3, 100, 300, 100, 140, 2)], [[1, 3, 2, 4, 0]], [[0, 1, 2, 3, 4]],
                  lambda c: len(c["sites"]) == 1 and c["sites"][0]["n_members"] == len(c["entries"]) == 5 and c["sites"][0]["n_sized"] == 3))
    C.append(case("all_singletons", [(0, 1000, 50, 0, 0), (0, 3000, 60, 1, 0), (0, 2000, 0, 2, 0), (1, 1000, 70, 0, 0)], {},
                  [S(0, 1000, 50, 0, 1, 1, 1, 50, 50, 1000, 1000, 0), S(0, 2000, 0, 0, 1, 1, 0, 0, 0, 2000, 2000, 2), S(0, 3000, 60, 0, 1, 1, 1, 60, 60, 3000, 3000, 1),
                   S(1, 1000, 70, 0, 1, 1, 1, 70, 70, 1000, 1000, 3)], [[0], [2], [1], [3]], [[0], [2], [1], [0]],
                  lambda c: len(c["sites"]) == len(c["entries"]) and all(s["n_members"] == 1 for s in c["sites"])))
    # sample 7 twice, with sample 2 between its entries in key order (positions come before samples there): two samples, three members
    C.append(case("one_sample_twice", [(0, 100, 60, 7, 0), (0, 105, 70, 2, 0), (0, 110, 80, 7, 0)], {},
                  [S(0, 105, 70, 0, 2, 3, 3, 60, 80, 100, 110, 1)], [[0, 1, 2]], [[2, 7]],
                  lambda c: c["sites"][0]["n_samples"] < c["sites"][0]["n_members"] and [e[3] for e in c["entries"]] == [7, 2, 7]))
    # no sized member, an even count: four members -> member 1
    C.append(case("no_sized_member", [(0, 100, 0, 0, 0), (0, 101, 0, 1, 0), (0, 102, 0, 2, 0), (0, 103, 0, 3, 0)], {},
                  [S(0, 101, 0, 0, 4, 4, 0, 0, 0, 100, 103, 1)], [[0, 1, 2, 3]], [[0, 1, 2, 3]],
                  lambda c: c["sites"][0]["n_sized"] == 0 and c["sites"][0]["len"] == 0 and c["sites"][0]["rep"] == 1))
    # even counts for both medians (four members, four sized: 10, 20, 30, 40 -> 20 = entry 2; positions -> 210), odd counts on target 1
    # (three: positions -> 51; lengths 5, 6, 7 -> 6 = entry 6)
    C.append(case("medians_even_and_odd", [(0, 200, 40, 0, 0), (0, 210, 30, 1, 0), (0, 220, 20, 2, 0), (0, 230, 10, 3, 0), (1, 50, 5, 0, 0), (1, 51, 7, 1, 0), (1, 52, 6, 2, 0)], {},
                  [S(0, 210, 20, 0, 4, 4, 4, 10, 40, 200, 230, 2), S(1, 51, 6, 0, 3, 3, 3, 5, 7, 50, 52, 6)], [[0, 1, 2, 3], [4, 5, 6]], [[0, 1, 2, 3], [0, 1, 2]],
                  lambda c: [s["n_sized"] for s in c["sites"]] == [4, 3] and [s["n_members"] for s in c["sites"]] == [4, 3]))
    # four sized members of one length: (100, s3, i1), (100, s3, i2), (100, s4, i3), (100, s5, i0) -> the second = entry 2.  By sample, then by
    # the INPUT index: in key order entry 2 (pos 101) comes before entry 1 (pos 102), and by the index alone entry 1 would be the second
    C.append(case("len_ties", [(0, 100, 100, 5, 0), (0, 102, 100, 3, 0), (0, 101, 100, 3, 0), (0, 103, 100, 4, 0)], {},
                  [S(0, 101, 100, 0, 3, 4, 4, 100, 100, 100, 103, 2)], [[0, 2, 1, 3]], [[3, 4, 5]],
                  lambda c: len(set(e[2] for e in c["entries"])) == 1 and c["sites"][0]["rep"] == 2 and c["members"][0].index(2) < c["members"][0].index(1)))
    # one (tid, pos) in two groups: two samples beat one
    C.append(case("shadow_two_groups", [(0, 500, 10, 0, 0), (0, 500, 20, 0, 1), (0, 500, 30, 1, 1)], {},
                  [S(0, 500, 20, 1, 2, 2, 2, 20, 30, 500, 500, 1), S(0, 500, 10, 0, 1, 1, 1, 10, 10, 500, 500, 0, 1, 0)], [[1, 2], [0]], [[0, 1], [0]],
                  lambda c: flags(c) == [0, 1] and c["sites"][0]["n_samples"] > c["sites"][1]["n_samples"] and c["sites"][0]["group"] > c["sites"][1]["group"]))
    # one (tid, pos) in four groups, the winner decided at each level: group 3 has three samples; of the others (two each) group 1 has
    # three members; groups 0 and 2 are equal in both and go by group.  Every loser's winner is site 0, not its predecessor
    C.append(case("shadow_each_level", [(0, 500, 0, 0, 0), (0, 500, 0, 1, 0), (0, 500, 0, 0, 1), (0, 500, 0, 1, 1), (0, 500, 0, 1, 1), (0, 500, 0, 0, 2), (0, 500, 0, 1, 2),
                                        (0, 500, 0, 0, 3), (0, 500, 0, 1, 3), (0, 500, 0, 2, 3)], {},
                  [S(0, 500, 0, 3, 3, 3, 0, 0, 0, 500, 500, 8), S(0, 500, 0, 1, 2, 3, 0, 0, 0, 500, 500, 3, 1, 0), S(0, 500, 0, 0, 2, 2, 0, 0, 0, 500, 500, 0, 1, 0),
                   S(0, 500, 0, 2, 2, 2, 0, 0, 0, 500, 500, 5, 1, 0)], [[7, 8, 9], [2, 3, 4], [0, 1], [5, 6]], [[0, 1, 2], [0, 1], [0, 1], [0, 1]],
                  lambda c: [s["group"] for s in c["sites"]] == [3, 1, 0, 2] and [s["winner"] for s in c["sites"]] == [-1, 0, 0, 0]))
    # a shadowed site between two sites.  Target 0: 1000, 1040 (+ its shadow), 1085: 1085 is 45 from the not-shadowed 1040 -> crowded, the
    # shadow itself never.  Target 1: 2000, 2040 (+ shadow), 2091: 51 away -> not crowded; 2040 is, by 2000
    C.append(case("shadowed_between", [(0, 1000, 0, 0, 0), (0, 1040, 0, 0, 1), (0, 1040, 0, 1, 1), (0, 1040, 0, 0, 2), (0, 1085, 0, 0, 0),
                                       (1, 2000, 0, 0, 0), (1, 2040, 0, 0, 1), (1, 2040, 0, 1, 1), (1, 2040, 0, 0, 2), (1, 2091, 0, 0, 0)], {},
                  [S(0, 1000, 0, 0, 1, 1, 0, 0, 0, 1000, 1000, 0, 2), S(0, 1040, 0, 1, 2, 2, 0, 0, 0, 1040, 1040, 1, 2), S(0, 1040, 0, 2, 1, 1, 0, 0, 0, 1040, 1040, 3, 1, 1),
                   S(0, 1085, 0, 0, 1, 1, 0, 0, 0, 1085, 1085, 4, 2), S(1, 2000, 0, 0, 1, 1, 0, 0, 0, 2000, 2000, 5, 2), S(1, 2040, 0, 1, 2, 2, 0, 0, 0, 2040, 2040, 6, 2),
                   S(1, 2040, 0, 2, 1, 1, 0, 0, 0, 2040, 2040, 8, 1, 5), S(1, 2091, 0, 0, 1, 1, 0, 0, 0, 2091, 2091, 9)],
                  [[0], [1, 2], [3], [4], [5], [6, 7], [8], [9]], [[0], [0, 1], [0], [0], [0], [0, 1], [0], [0]],
                  lambda c: flags(c) == [2, 2, 1, 2, 2, 2, 1, 0] and c["sites"][3]["pos"] - c["sites"][1]["pos"] == 45 and c["sites"][7]["pos"] - c["sites"][5]["pos"] == 51))
    # The filter comes before shadowing and crowding.  (A would-be WINNER that min_samples removes cannot leave a runner-up behind: the
    # winner of a (tid, pos) run has the most samples, so whatever drops it drops the rest of the run.  What the filter can remove is a
    # neighbour or a loser.)  At min_samples 1: 1000 and 1030 crowd each other and group 2 at 1030 is shadowed; at 2 only the site with two
    # samples is left: neither crowded nor a winner of anything
    ms = [(0, 1000, 0, 0, 0), (0, 1030, 0, 0, 1), (0, 1030, 0, 1, 1), (0, 1030, 0, 5, 2)]
    C.append(case("min_samples_1_of_the_pair", ms, dict(min_samples=1),
                  [S(0, 1000, 0, 0, 1, 1, 0, 0, 0, 1000, 1000, 0, 2), S(0, 1030, 0, 1, 2, 2, 0, 0, 0, 1030, 1030, 1, 2), S(0, 1030, 0, 2, 1, 1, 0, 0, 0, 1030, 1030, 3, 1, 1)],
                  [[0], [1, 2], [3]], [[0], [0, 1], [5]], lambda c: flags(c) == [2, 2, 1]))
    C.append(case("min_samples_2_before_shadow_and_crowd", ms, dict(min_samples=2), [S(0, 1030, 0, 1, 2, 2, 0, 0, 0, 1030, 1030, 1)], [[1, 2]], [[0, 1]],
                  lambda c: flags(c) == [0] and c["opt"]["min_samples"] == 2))
    # adjacent positions across a group change and a tid change do not merge (the two of target 0 crowd each other; target 1 stands alone)
    C.append(case("tid_and_group_change", [(0, 100, 0, 0, 0), (0, 101, 0, 1, 1), (1, 100, 0, 2, 0), (1, 101, 0, 3, 0)], {},
                  [S(0, 100, 0, 0, 1, 1, 0, 0, 0, 100, 100, 0, 2), S(0, 101, 0, 1, 1, 1, 0, 0, 0, 101, 101, 1, 2), S(1, 100, 0, 0, 2, 2, 0, 0, 0, 100, 101, 2)],
                  [[0], [1], [2, 3]], [[0], [1], [2, 3]], lambda c: len(c["sites"]) == 3 and flags(c) == [2, 2, 0]))
    for n in SIZES:
        C.append(singletons(n))
        C.append(one_cluster(n))
    return C


def singletons(n):
    """n entries 1,000 apart, in scattered input order: entry i has rank (7 i + 3) mod n; every third rank without a length"""
    inv = pow(7, -1, n)
    at = lambda r: ((r - 3) * inv) % n                              # the entry of rank r
    ln = lambda r: 0 if r % 3 == 0 else 100 + r
    entries = [(0, 1000 * ((7 * i + 3) % n), ln((7 * i + 3) % n), i % 40, 0) for i in range(n)]
    sites = [S(0, 1000 * r, ln(r), 0, 1, 1, 1 if ln(r) else 0, ln(r), ln(r), 1000 * r, 1000 * r, at(r)) for r in range(n)]
    return case("singletons_%d" % n, entries, {}, sites, [[at(r)] for r in range(n)], [[at(r) % 40] for r in range(n)],
                lambda c: len(c["sites"]) == len(c["entries"]) == n)


def one_cluster(n):
    """n entries two bases apart, one cluster: entry i has position rank (7 i + 3) mod n and the length 1 + (11 i + 1) mod n (all distinct)"""
    inv7, inv11 = pow(7, -1, n), pow(11, -1, n)
    at = lambda r: ((r - 3) * inv7) % n
    entries = [(1, 10 + 2 * ((7 * i + 3) % n), 1 + (11 * i + 1) % n, i % 40, 2) for i in range(n)]
    mid = (n - 1) // 2
    site = S(1, 10 + 2 * mid, 1 + mid, 2, 40, n, n, 1, n, 10, 10 + 2 * (n - 1), ((mid - 1) * inv11) % n)
    return case("one_cluster_%d" % n, entries, {}, [site], [[at(r) for r in range(n)]], [list(range(40))],
                lambda c: len(c["sites"]) == 1 and c["sites"][0]["n_members"] == n)


def refusals():
    """-> list of (name, entries or None (a null pointer), n or None (= len(entries)), n_targets, options, code)"""
    ok = [(0, 1000, 60, 0, 0)]
    R = [("n_negative", ok, -1, N_TARGETS, {}, E_ARG),
         ("entries_null", None, 1, N_TARGETS, {}, E_ARG),
         ("tid_high", [(N_TARGETS, 5, 0, 0, 0)], None, N_TARGETS, {}, E_ARG),
         ("tid_negative", [(-1, 5, 0, 0, 0)], None, N_TARGETS, {}, E_ARG),
         ("tid_with_no_targets", ok, None, 0, {}, E_ARG),
         ("pos_negative", ok + [(0, -1, 0, 0, 0)], None, N_TARGETS, {}, E_ARG),
         ("len_negative", ok + [(0, 5, -1, 0, 0)], None, N_TARGETS, {}, E_ARG),
         ("sample_negative", ok + [(0, 5, 0, -1, 0)], None, N_TARGETS, {}, E_ARG),
         ("group_negative", ok + [(0, 5, 0, 0, -1)], None, N_TARGETS, {}, E_ARG),
         ("dist_negative", ok, None, N_TARGETS, dict(dist=-1), E_ARG),
         ("min_samples_0", ok, None, N_TARGETS, dict(min_samples=0), E_ARG),
         ("reserved0", ok, None, N_TARGETS, dict(reserved0=1), E_ARG),
         ("reserved1", ok, None, N_TARGETS, dict(reserved1=1), E_ARG),
         ("too_many_entries", ok, MAX_ENTRIES, N_TARGETS, {}, E_RANGE)]          # refused by its count: the array is never read
    return R


# what the generated case has to contain (cohort_ref.coverage counts it on the checker's answer; test_cohort_ref.py asserts it)
NEEDS = dict(shadowed=20, crowded=20, largest=513, dropped_run=511, sized=1, unsized=1)


def generated():
    """the seeded case: 3 targets, 4 groups, 40 samples, about 6,000 entries (cohort_ref.generate says what is planted in it)"""
    return generate()
