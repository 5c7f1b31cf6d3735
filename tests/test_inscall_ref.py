"""The insertion caller's definition (tests/inscall_ref.py, the checker of telr_call_insertions) against hand-derived answers, one
case per rule, and against the known answer of the bundled reads: one non-reference insertion at chr2L:~33,017;
tools/record_checks_check.cpp (the record and call-list refusals the call stages share) under ASan and UBSan."""
import os
import shutil
import subprocess

import pytest

import inscall_cases as cases
import inscall_ref as ref
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = cases.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(case):
    _, recs, opt, want_sigs, want_calls = case
    alns, cig = cases.pack(recs)
    sigs, calls = ref.call_insertions(alns, cig, opt)
    assert sigs == want_sigs
    assert calls == want_calls


def test_defaults_are_the_documented_ones():
    assert ref.DEFAULTS == dict(min_len=50, min_mapq=20, min_clip=200, max_ref_gap=200, cluster_dist=50, min_support=10, min_sized=1)


def test_key_order_is_complete():
    # the same position, record and kind: ordered by len, then mate
    recs = [cases.rec(0, 3000, 0, 100, 1000, 1100, [(100, "M")]), cases.rec(0, 3000, 900, 1000, 1100, 1200, [(100, "M")], flags=4),
            cases.rec(0, 3000, 600, 700, 1150, 1250, [(100, "M")], flags=4)]
    sigs = ref.signatures(*cases.pack(recs), opt=cases.NO_CLIP)
    first = [(s["rec"], s["mate"], s["len"]) for s in sigs if s["rec"] == 0]
    assert first == [(0, 2, 450), (0, 1, 800)]          # len before mate


@pytest.fixture(scope="module")
def fixture_records(data_dir):
    from oracle import binding as ob
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    out = {}
    for name in ("map-pb", "ngmlr-pacbio", "map-ont"):
        io, mo = preset(name)
        out[name] = ob.OracleIndex(ts, io).map(qs, mo)
    return out


@pytest.mark.parametrize("name", ["map-pb", "ngmlr-pacbio", "map-ont"])
def test_bundled_reads_give_the_known_insertion(fixture_records, name):
    r = fixture_records[name]
    sigs, calls = ref.call_insertions(r["alns"], r["cigars"])
    assert len(calls) == 1
    c = calls[0]
    print(name, {k: c[k] for k in ref.CALL_FIELDS}, sorted(s["pos"] for s in sigs if s["qid"] in c["reads"] and abs(s["pos"] - c["pos"]) < 100))
    assert 33006 <= c["pos"] <= 33029
    assert c["support"] >= 12 and c["n_sized"] >= 5
    assert 4347 <= c["len"] <= 4678
    # the cluster at the end of the reference has six clipped reads and no sized one: still one call at min_support 6
    calls6 = ref.calls(sigs, dict(min_support=6, min_sized=1))
    assert len(calls6) == 1 and calls6[0]["pos"] == c["pos"]


def test_record_checks_check_under_sanitizers(tmp_path):
    """tools/record_checks_check.cpp = record_checks.h (what telr_call_insertions, telr_genotype_insertions and telr_draft_contigs refuse
    in a result's records and in a call list, with the full texts) as a program of its own, compiled with -fsanitize=address,undefined"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "record_checks_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "record_checks_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout
