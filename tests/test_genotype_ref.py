"""The genotyping step's definition (tests/genotype_ref.py, the checker of telr_genotype_insertions) against hand-derived answers,
one case per rule, and against the bundled reads: the one insertion has three reference reads and one ambiguous read next to its
12-13 supporters, whatever the preset."""
import pytest

import genotype_cases as cases
import genotype_ref as gref
import inscall_ref as iref
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

HAND = cases.hand_cases()


def trimmed(got):
    return [{k: g[k] for k in gref.GT_FIELDS + ("ref_reads", "ambig_reads")} for g in got]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(case):
    _, recs, calls, opt, want = case
    alns, cig = cases.pack(recs)
    assert trimmed(gref.genotype(alns, cig, calls, opt)) == want


def test_hand_cases_cover_both_sides_of_every_rule():
    names = [c[0] for c in HAND]
    assert len(set(names)) == len(names) >= 14
    gts = set(g["gt"] for c in HAND for g in c[4])
    assert gts == {0, 1, 2}
    assert any(g["ambig"] for c in HAND for g in c[4]) and any(g["ref"] for c in HAND for g in c[4])


def test_defaults_are_the_documented_ones():
    assert gref.DEFAULTS == dict(flank=50, min_mapq=20, max_window_indel=20, het_pct=30, hom_pct=80)


def test_window_indel_by_hand():
    # 900 + 80 M -> an I of 10 at 980 (inside [950, 1050]); 40 M -> a D of 200 over [1020, 1220): 30 of its bases inside
    alns, cig = cases.pack([cases.grec(0, 900, [(80, "M"), (10, "I"), (40, "M"), (200, "D"), (10, "M")])])
    assert gref.window_indel(alns[0], cig, 1000, 50) == 40
    assert gref.window_indel(alns[0], cig, 1000, 0) == 0          # window [1000, 1000]: the I is at 980, a D covers no base of an empty window
    assert gref.window_indel(alns[0], cig, 1120, 50) == 100       # wholly inside the D
    assert gref.gt_of(0, 0, 30, 80) == 2 and gref.gt_of(0, 1, 30, 80) == 0


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


@pytest.mark.parametrize("name,alt", [("map-pb", 13), ("map-ont", 12), ("ngmlr-pacbio", 13)])
def test_bundled_reads(fixture_records, name, alt):
    r = fixture_records[name]
    _, calls = iref.call_insertions(r["alns"], r["cigars"])
    assert len(calls) == 1 and 33022 <= calls[0]["pos"] <= 33024
    g = gref.genotype(r["alns"], r["cigars"], calls)[0]
    print(name, {k: g[k] for k in gref.GT_FIELDS}, g["ref_reads"], g["ambig_reads"], g["indels"])
    assert g["ref_reads"] == [1, 5, 12] and g["ambig_reads"] == [6]
    assert (g["ref"], g["ambig"], g["alt"], g["gt"]) == (3, 1, alt, 2)
    # far from the threshold of 20 on both sides, so the pin does not hang on a base
    assert all(4 <= min(g["indels"][q]) <= 7 for q in (1, 5, 12)) and 55 <= min(g["indels"][6]) <= 57
