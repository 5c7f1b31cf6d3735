"""The multi-part index without a device: the plain-Python merge (tests/part_merge_ref.py) against answers derived by
hand, as the identity on a single oracle result, and split against unsplit with the CPU oracle; telr_part_plan through the library
against the definition, its exact-fit edges, the greedy property by brute force and its codes; tools/part_plan_check.cpp under ASan
and UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import part_merge_cases as pc
import part_merge_ref as ref
from telr_amd import _lib
from telr_amd._abi import MF_CIGAR, MF_MM2_MAPQ, MF_PER_TARGET, TELR_E_ARG, TELR_E_RANGE
from telr_amd.aligner import Engine
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition against hand-derived answers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.HAND, ids=[c["name"] for c in pc.HAND])
def test_merge_by_hand(c):
    alns, cig = ref.merge(c["parts"], c["tid_maps"], c["n_queries"], pc.options(**c["opt"]))
    assert pc.signature(c, alns) == c["expect"]
    # dense CIGAR offsets in output order, every record's words those of its source
    assert [int(x) for x in alns["cigar_off"]] == [int(x) for x in np.cumsum(alns["n_cigar"]) - alns["n_cigar"]] and len(cig) == int(alns["n_cigar"].sum())
    for r, (q, p, rank, *_) in zip(alns, pc.signature(c, alns)):
        a, w = c["parts"][p]
        src = a[a["qid"] == q][rank]
        assert np.array_equal(cig[r["cigar_off"]:r["cigar_off"] + r["n_cigar"]], w[src["cigar_off"]:src["cigar_off"] + src["n_cigar"]])
        assert r["tid"] == c["tid_maps"][p][src["tid"]] and (r["flags"] & ref.F_REV) == (src["flags"] & ref.F_REV)
        assert all(r[f] == src[f] for f in ("qlen", "qs", "qe", "tlen", "ts", "te", "mlen", "blen", "score", "dp_score", "cnt", "n_cigar", "n_ambi"))


def test_the_pri_ratio_edge_is_a_float32_edge():
    assert np.float32(1000) * np.float32(0.8) == np.float32(800) and float(np.float32(0.8)) > 0.8
    assert ref.masks(0, 1000, 500, 1500, 0.5) is False and ref.masks(0, 1000, 499, 1500, 0.5) is True       # overlap 500 of 1000: not above one half


def test_the_edge_cases_hold_what_they_claim():
    names = [c["name"] for c in pc.CASES]
    assert len(set(names)) == len(names)
    sizes, words, seams = set(), set(), 0
    for c in pc.EDGE:
        mo = pc.options(**c["opt"])
        alns, _ = ref.merge(c["parts"], c["tid_maps"], c["n_queries"], mo)
        pool = np.zeros(max(c["n_queries"], 1), np.int64)
        for a, _ in c["parts"]:
            pool += np.bincount(a["qid"], minlength=len(pool))
            words |= set(int(x) for x in a["n_cigar"])
        sizes |= set(int(x) for x in pool)
        # a parent in an earlier 64-tile of the order: a kept secondary whose parent lies 64 or more kept places before it
        first = {int(q): int(np.flatnonzero(alns["qid"] == q)[0]) for q in np.unique(alns["qid"])}
        seams += any((r["flags"] & ref.F_SECONDARY) and k - first[int(r["qid"])] - r["parent"] >= 64 for k, r in enumerate(alns))
    assert {0, 1, 2, 63, 64, 65, 130} <= sizes and {0, 1, 3, 4, 5, 63, 64, 65, 1000} <= words and seams >= 2
    assert any(len(a) == 0 for c in pc.EDGE for a, _ in c["parts"]) and any(c["n_queries"] == 0 for c in pc.EDGE) and any(not c["parts"] for c in pc.EDGE)
    assert {len(c["parts"]) for c in pc.EDGE} >= {1, 2, 3}


def test_refusals_of_the_definition():
    c = pc.HAND[0]
    mo = pc.options()
    mo.flags |= MF_PER_TARGET
    with pytest.raises(ValueError):
        ref.merge(c["parts"], c["tid_maps"], 1, mo)
    for field, value in (("qid", 1), ("tid", 2), ("n_cigar", 99), ("parent", 1), ("flags", 3), ("flags", 8)):
        a, w = c["parts"][0]
        a = a.copy(); a[field] = value
        with pytest.raises(ValueError):
            ref.merge([(a, w), c["parts"][1]], c["tid_maps"], 1, pc.options())


# ---- identity: one part -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled():
    d = os.path.join(ROOT, "tests", "data")
    return read_fasta(os.path.join(d, "ref_38kb.fasta"))[1], read_fasta(os.path.join(d, "reads.fasta"))[1]


@pytest.mark.parametrize("name", ["map-ont", "map-pb", "asm10", "ngmlr-ont", "ngmlr-pacbio"])
@pytest.mark.parametrize("mm2_mapq", [False, True])
def test_one_part_is_the_identity(bundled, name, mm2_mapq):
    from oracle import binding as ob
    ts, qs = bundled
    io, mo = preset(name)
    mo = mo.copy(); mo.flags |= MF_CIGAR | (MF_MM2_MAPQ if mm2_mapq else 0)
    res = ob.OracleIndex(ts, io).map(qs, mo)
    assert len(res["alns"]) > 0 or name == "asm10"          # (asm10 finds nothing in reads with 10 % errors: the empty result is its identity)
    alns, cig = ref.merge([(res["alns"], res["cigars"])], [np.arange(len(ts), dtype=np.int32)], len(qs), mo)
    assert ref.records_equal(alns, cig, res["alns"], res["cigars"])


# ---- split against unsplit with the oracle ----------------------------------------------------------------------------------------------
def oracle_parts(targets, reads, part_of, io, mo):
    from oracle import binding as ob
    parts, maps = [], []
    for p in range(max(part_of) + 1):
        m = np.array([t for t, x in enumerate(part_of) if x == p], np.int32)
        res = ob.OracleIndex([targets[t] for t in m], io).map(reads, mo)
        parts.append((res["alns"], res["cigars"])); maps.append(m)
    return parts, maps


@pytest.fixture(scope="module")
def oracle_runs():
    """(repeats, preset) -> (mo, unsplit result, {number of parts: merged result})"""
    from oracle import binding as ob
    out = {}
    for repeats in (False, True):
        targets, reads = pc.genome(repeats)
        for name in ("map-ont", "ngmlr-ont"):
            io, mo = preset(name)
            mo = mo.copy(); mo.flags |= MF_CIGAR
            whole = ob.OracleIndex(targets, io).map(reads, mo)
            merged = {}
            for n, part_of in pc.CUTS.items():
                parts, maps = oracle_parts(targets, reads, part_of, io, mo)
                merged[n] = ref.merge(parts, maps, len(reads), mo)
            out[(repeats, name)] = (mo, whole, merged)
    return out


@pytest.mark.parametrize("name", ["map-ont", "ngmlr-ont"])
@pytest.mark.parametrize("n_parts", [2, 4])
def test_split_equals_unsplit_on_the_unique_genome(oracle_runs, name, n_parts):
    _, whole, merged = oracle_runs[(False, name)]
    alns, cig = merged[n_parts]
    print("%s, %d parts: %d records unsplit, %d merged" % (name, n_parts, len(whole["alns"]), len(alns)))
    assert len(whole["alns"]) >= 80
    assert ref.records_equal(alns, cig, whole["alns"], whole["cigars"])


@pytest.mark.parametrize("name", ["map-ont", "ngmlr-ont"])
@pytest.mark.parametrize("n_parts", [2, 4])
def test_split_keeps_the_primaries_on_the_repeat_genome(oracle_runs, name, n_parts):
    _, whole, merged = oracle_runs[(True, name)]
    alns, _ = merged[n_parts]
    a = whole["alns"][(whole["alns"]["flags"] & ref.F_PRIMARY) != 0]
    b = alns[(alns["flags"] & ref.F_PRIMARY) != 0]
    print("%s, %d parts: %d records unsplit (%d secondary), %d merged (%d secondary)" % (
        name, n_parts, len(whole["alns"]), int(((whole["alns"]["flags"] & 2) != 0).sum()), len(alns), int(((alns["flags"] & 2) != 0).sum())))
    assert len(a) == len(b) > 0 and np.array_equal(a["qid"], b["qid"])
    for f in pc.PRIMARY_FIELDS:
        assert np.array_equal(a[f], b[f]), f


# ---- the planner through the library ----------------------------------------------------------------------------------------------------
LIMITS = [20000, 34816, 34817, 50000, 100000, 0]
SETS = [[1000] * 5, [0, 0, 0], [3000, 1, 15000, 2, 2, 9000, 64, 63, 65], [100], [], list(pc.LENGTHS)]


@pytest.mark.parametrize("limit", LIMITS)
def test_part_plan_equals_the_definition_and_is_greedy(limit):
    L = limit or ref.INDEX_LIMIT
    for lengths in SETS:
        try:
            want = ref.part_plan(lengths, limit)
        except OverflowError:
            with pytest.raises(_lib.TelrError) as e:
                Engine.part_plan(lengths, limit)
            assert e.value.code == TELR_E_RANGE and "target" in str(e.value)
            continue
        got = [int(x) for x in Engine.part_plan(lengths, limit)]
        assert got == want
        runs = [[t for t, p in enumerate(got) if p == k] for k in range(max(got) + 1)] if got else []
        for k, run in enumerate(runs):
            assert run == list(range(run[0], run[-1] + 1)) and (k == 0 or run[0] == runs[k - 1][-1] + 1)
            assert ref.index_accepts([lengths[t] for t in run], L)
            assert k + 1 == len(runs) or not ref.index_accepts([lengths[t] for t in run] + [lengths[run[-1] + 1]], L)


def test_part_plan_exact_fit_edges():
    # a target of 1,000 bases takes (1000 + 16384 + 63) & ~63 = 17,408: two of them REACH 34,816
    assert ref.extent_next(0, 1000) == 17408
    assert [int(x) for x in Engine.part_plan([1000] * 3, 34816)] == [0, 1, 2]
    assert [int(x) for x in Engine.part_plan([1000] * 3, 34817)] == [0, 0, 1]
    assert [int(x) for x in Engine.part_plan([1000], 17409)] == [0]
    for lengths, limit in (([1000], 17408), ([1000, 5000, 1000], 17409), ([(1 << 31) - 16384 - 63], 0)):
        with pytest.raises(_lib.TelrError) as e:
            Engine.part_plan(lengths, limit)
        assert e.value.code == TELR_E_RANGE
    assert [int(x) for x in Engine.part_plan([(1 << 31) - 16384 - 64], 0)] == [0]
    assert [int(x) for x in Engine.part_plan([1 << 30, 1 << 30, 1 << 30, 5], 0)] == [0, 1, 2, 2]
    assert [int(x) for x in Engine.part_plan([1 << 30, 1 << 30, 1 << 30, 5], 1 << 40)] == [0, 1, 2, 2]
    for n, part_of in pc.CUTS.items():
        assert [int(x) for x in Engine.part_plan(pc.LENGTHS, pc.max_part_bases(part_of))] == part_of


def test_part_plan_codes():
    L = _lib.lib()
    one = np.array([100], np.int32); neg = np.array([100, -1], np.int32); out = np.full(2, -7, np.int32); n = C.c_int32(-7)
    assert L.telr_part_plan(2, neg.ctypes.data, 0, out.ctypes.data, C.byref(n)) == TELR_E_ARG
    assert L.telr_part_plan(1, one.ctypes.data, -1, out.ctypes.data, C.byref(n)) == TELR_E_ARG
    assert L.telr_part_plan(-1, one.ctypes.data, 0, out.ctypes.data, C.byref(n)) == TELR_E_ARG
    assert L.telr_part_plan(1, None, 0, out.ctypes.data, C.byref(n)) == TELR_E_ARG
    assert L.telr_part_plan(1, one.ctypes.data, 0, None, C.byref(n)) == TELR_E_ARG
    assert L.telr_part_plan(1, one.ctypes.data, 0, out.ctypes.data, None) == TELR_E_ARG
    assert n.value == -7 and (out == -7).all()
    assert L.telr_part_plan(0, None, 0, None, C.byref(n)) == 0 and n.value == 0
    assert L.telr_part_plan(1, one.ctypes.data, 16000, out.ctypes.data, C.byref(n)) == TELR_E_RANGE and b"target 0" in L.telr_part_plan_error()
    with pytest.raises(_lib.TelrError) as e:
        Engine.part_plan([5, -1])
    assert e.value.code == TELR_E_ARG


def test_part_plan_check_under_sanitizers(tmp_path):
    """tools/part_plan_check.cpp = part_plan.h (the planner and the record checks of telr_merge_parts) as a program of its own, compiled
    with -fsanitize=address,undefined"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "part_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "part_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout
