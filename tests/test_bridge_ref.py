"""The definitions of telr_seqset_join and telr_bridge_contigs as plain Python (tests/bridge_ref.py, the checker of the device code)
against hand-derived answers -- every case of tests/bridge_cases.py asserts the edge it claims -- and against truth: a planted insertion
that no read spans, mapped by the CPU oracle, is rejected by the caller's defaults, called with min_sized = 0, left without a draft, and
bridged into the true haplotype slice letter for letter."""
import numpy as np
import pytest

import bridge_cases as cases
import bridge_ref as bref
import draft_ref as dref
import inscall_ref as iref
from telr_amd.presets import preset

BRIDGE = cases.bridge_cases()


# ---- join ---------------------------------------------------------------------------------------------------------------------------
def test_join_by_hand():
    seqs = ["ACGTNacgu", "GGGTTT"]
    # pieces: ACG | rc(GTN) = NAC | (empty) | u -> T ; second sequence: no pieces; third: rc(GGGTTT) twice
    got = bref.join(seqs, [0, 4, 4, 6], [0, 0, 1, 0, 1, 1], [0, 2, 3, 8, 0, 0], [3, 3, 0, 1, 6, 6], [0, 1, 0, 0, 1, 1])
    assert got == ["ACGNACT", "", "AAACCCAAACCC"]
    assert bref.join(seqs, [0], [], [], []) == []


def test_join_cases_cover_the_list():
    parent = cases.join_parent()
    off, idx, start, ln, rc, names = cases.join_cases(parent)
    assert len(names) == len(set(names)) == len(off) - 1 and off[-1] == len(idx)
    want = bref.join(parent, off, idx, start, ln, rc)
    by = dict(zip(names, want))
    assert parent[3][0] == "N" and parent[3][-1] == "N"
    for a in cases.JOIN_LENS:
        assert len(by["one_%d" % a]) == a
        for b in cases.JOIN_LENS:
            assert len(by["two_%d_%d" % (a, b)]) == a + b
    assert sorted((64 + r) % 32 for r in range(32)) == list(range(32))          # a second piece at every residue mod 32
    assert len(by["three_3_5_4"]) == 12 < 16 and len(by["three_1_1_1"]) == 3      # three pieces inside one output word
    assert by["N_seam_ff"][9:11] == "NN" and by["N_seam_rr"][9:11] == "NN"        # an N on both sides of the seam
    assert by["no_pieces"] == "" and by["empty_pieces"] == "" and by["three_0_0_0"] == ""
    assert by["repeat"][:50] == by["repeat"][50:100] == dref.revcomp(by["repeat"][100:])
    assert by["rc_11"] == dref.revcomp(parent[0][20:57]) + dref.revcomp(parent[1][30:71])
    assert sum(rc) > 40 and any(n == 0 for n in ln)


# ---- bridge -------------------------------------------------------------------------------------------------------------------------
def test_vote_by_hand():
    o = bref.options(k=11, window=20)
    U = "A" * 5 + "ACGTTGCAAGGCTTAGCCATG"          # cL = 26: the window is U[6:26]
    V = "TTTTT" + U[8:22] + "GGGGG"               # V[5:19] = U[8:22]: 11-mers at U offsets 8 .. 11 match at j = 5 .. 8 (d = 3)
    m = bref.matches(U, V, o)
    assert m == [(8, 5), (9, 6), (10, 7), (11, 8)]
    v = bref.vote(U, V, o)
    assert (v["votes"], v["i"], v["j"], v["diag"], v["best_bin"]) == (4, 9, 6, 3, -1)       # bins -1 and 0 tie at 4: the smaller; the second of four
    # the k-mer at U offset 5 straddles the window's first base: it is not in the window
    assert bref.matches(U, U[5:16], o) == [] and bref.matches(U, U[6:17], o) == [(6, 0)]
    # a k-mer that occurs twice in the window is not usable
    U2 = "ACGTACGTACGTACGTACGTAC"
    assert bref.matches(U2, U2[:11], bref.options(k=11, window=22)) == []
    assert bref.vote("ACGTACGTACGTA", "TTTTTTTTTTTTTT", bref.options())["votes"] == 0


@pytest.mark.parametrize("case", BRIDGE, ids=[c["name"] for c in BRIDGE])
def test_bridge_case(case):
    alns, cig, sigs, calls, reads = case["data"]
    out, seqs = bref.bridges(alns, cig, calls, sigs, reads, case["opt"], case["want"])
    case["expect"](out, seqs)
    for d, s in zip(out, seqs):
        assert (s is None) == (d["sig_l"] < 0)
        if s is not None:
            assert len(s) == d["len_l"] + d["len_r"] and d["qid_l"] != d["qid_r"] and 0 <= d["ins_off"] and d["ins_off"] + d["ins_len"] <= len(s)
        else:
            assert all(d[f] == 0 for f in bref.BRIDGE_FIELDS if f not in ("sig_l", "sig_r", "n_left", "n_right"))


def test_bridge_cases_cover_the_list():
    names = [c["name"] for c in BRIDGE]
    assert len(set(names)) == len(names) >= 35
    for need in ("cL_eq_k", "cL_eq_k_minus_1", "cL_eq_window_4096", "cL_eq_window_plus_1_4096", "window_duplicate", "N_in_U", "N_in_V", "bin_edge_m129_m128",
                 "bin_edge_m1_0", "bin_edge_127_128", "bins_tied", "even_band", "votes_eq_min_votes", "votes_below_min_votes", "fewer_than_pairs",
                 "cut_matters", "same_read_only", "pairs_tied", "strands_00", "strands_01", "strands_10", "strands_11", "want_mask", "no_bridge_reasons",
                 "max_len_one_over", "V_several_chunks", "V_second_bin_pass", "table_full"):
        assert need in names, need
    assert bref.DEFAULTS == dict(flank=2000, min_flank=500, reach=50, max_len=100000, k=13, window=4096, min_votes=8, pairs=4)


def test_an_error_free_pair_joins_without_a_seam():
    """the contig of a bridge is the two reads' common sequence: flank + element + flank, whatever the strands"""
    rng = np.random.default_rng(2)
    E = cases.rand_seq(rng, 900)
    for rl in (0, 1):
        for rr in (0, 1):
            b = cases.Build(10 + 2 * rl + rr)
            p = b.locus()
            ql = b.left(p, E[:600], rev=rl); qr = b.right(p, E[300:], rev=rr)
            b.call(p, [ql, qr])
            alns, cig, sigs, calls, reads = b.done()
            out, seqs = bref.bridges(alns, cig, calls, sigs, reads, cases.SMALL)
            fl_l = bref.strand_bases(alns[0], reads)[10:30]; fl_r = bref.strand_bases(alns[1], reads)[600:620]
            assert seqs[0] == fl_l + E + fl_r and out[0]["ins_off"] == 20 and out[0]["ins_len"] == 900 and out[0]["diag"] == 300


def test_noisy_pairs_are_consistent():
    """a few of the seeded 10 % pairs (the device test runs all 200): whatever the vote finds, the record describes its contig"""
    (alns, cig, sigs, calls, reads), opt = cases.noisy_pairs(n=12)
    out, seqs = bref.bridges(alns, cig, calls, sigs, reads, opt)
    assert len(out) == 12 and all(d["n_left"] == 1 and d["n_right"] == 1 for d in out)
    for d, s in zip(out, seqs):
        if s is not None:
            assert d["votes"] >= bref.DEFAULTS["min_votes"] and len(s) == d["len_l"] + d["len_r"]


# ---- an insertion that no read spans, against truth -----------------------------------------------------------------------------------
def test_spanless_insertion_is_bridged_into_the_true_haplotype():
    from oracle import binding as ob
    f = cases.spanless_fixture()
    io, mo = preset("map-ont")
    r = ob.OracleIndex([f["chrom"]], io).map(f["reads"], mo)
    alns, cig = r["alns"], r["cigars"]
    # no read spans: every record ends or starts at the insertion
    assert len(alns) == 14 and all(int(a["te"]) <= f["pos"] + 20 or int(a["ts"]) >= f["pos"] - 20 for a in alns)
    sigs, calls = iref.call_insertions(alns, cig)
    assert calls == [] and len(sigs) == 14 and all(s["kind"] == 2 for s in sigs)          # the defaults reject the cluster: no sized signature
    sigs, calls = iref.call_insertions(alns, cig, dict(min_sized=0))
    assert len(calls) == 1 and (calls[0]["rep"], calls[0]["len"], calls[0]["support"], calls[0]["n_sized"]) == (-1, 0, 14, 0)
    assert abs(calls[0]["pos"] - f["pos"]) <= 20
    d, dseq = dref.drafts(alns, cig, calls, sigs, f["reads"])
    assert d[0]["sig"] == -1 and d[0]["n_candidates"] == 0 and dseq == []                  # no draft: no sized signature to cut at
    out, seqs = bref.bridges(alns, cig, calls, sigs, f["reads"])
    b = out[0]
    assert b["sig_l"] >= 0 and (b["n_left"], b["n_right"], b["n_voted"]) == (7, 7, 16)
    sl, sr = sigs[b["sig_l"]], sigs[b["sig_r"]]
    truth = f["hap"][sl["pos"] - 2000:sr["pos"] + 2000 + len(f["fam"])]                     # flank 2000 either side of the two clips' positions
    assert seqs[0] == truth                                                                # error-free reads, an exact junction: letter for letter
    assert f["fam"] in seqs[0] and b["ins_len"] == len(f["fam"]) + (sr["pos"] - sl["pos"])
    assert seqs[0][b["ins_off"]:b["ins_off"] + b["ins_len"]] == f["hap"][sl["pos"]:sr["pos"] + len(f["fam"])]
    assert {f["names"][b["qid_l"]], f["names"][b["qid_r"]]} == {"L0", "R0"}                 # the two longest clips
