"""The inputs of tests/vote_inputs.py on the CPU, no GPU: every builder's claims (asserted inside the builders: hits per sub-read and
chunk, list starts, sub-read counts, the designed vote tables, the exact anchor counts), and for every case and query

    the oracle's anchors with voting on  ==  tests/vote_ref.py applied to the oracle's anchors with vote_len = 0.

vote_ref is written from the header's text; where the two disagree the header decides.  The counts the builders took by brute force
over the oracle's sketch and index dump are checked against the oracle's own debug map here as well."""
import numpy as np
import pytest

import vote_inputs as I
import vote_ref as VR

CASES = I.all_cases()


@pytest.fixture(scope="module")
def maps():
    """-> name -> (case, the oracle's debug map without voting, with the case's options): computed once per case"""
    from oracle import binding as ob
    done = {}

    def get(name):
        if name not in done:
            c = CASES[name]()
            oix = ob.OracleIndex(list(c.targets), c.io)
            done[name] = (c, oix.map(list(c.queries), I.plain(c.mo), debug=True), oix.map(list(c.queries), c.mo, debug=True))
        return done[name]
    return get


def _per_query(o):
    off = o["anchor_off"]
    return [o["anchors"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_vote_ref(maps, name):
    c, unvoted, voted = maps(name)
    ix = I.Index(c.targets, c.io)
    removed = kept = 0
    for q, ku, kv in zip(c.queries, _per_query(unvoted), _per_query(voted)):
        np.testing.assert_array_equal(ku, ix.keys(q))                                 # the builders' brute force == the oracle's debug map
        want = VR.vote(ku, len(q), c.mo) if c.mo.vote_len > 0 else ku
        np.testing.assert_array_equal(kv, want)
        removed += len(ku) - len(kv); kept += len(kv)
    assert kept > 0 and (removed > 0 or c.mo.vote_len == 0)                           # not vacuous


def test_counts_from_the_oracle(maps):
    """the exact counts, from the oracle's anchor counts"""
    for name in ("stash", "width"):
        c, unvoted, _ = maps(name)
        assert np.diff(unvoted["anchor_off"]).tolist() == c.facts["hits"]
    assert maps("stash")[0].facts["hits"][:6] == [767, 767, 768, 768, 769, 769]
    assert maps("width")[0].facts["hits"][:4] == [65535, 65535, 65536, 65536] == maps("width")[0].facts["vmax"][:4]
    for name in ("tiers_plain", "tiers_voted"):
        c, _, voted = maps(name)
        assert tuple(np.diff(voted["anchor_off"]).tolist()) == I.TIER_COUNTS == tuple(c.facts["counts"])
    c, _, voted = maps("tiers_voted_fit")
    assert np.diff(voted["anchor_off"]).max() == I.SEGSORT_CAP


@pytest.mark.parametrize("o", range(len(I.THR_OPTS)))
def test_threshold_fates(maps, o):
    """every designed hit stays or goes in the oracle as the measured table says"""
    c, unvoted, voted = maps("threshold%d" % o)
    kv = set(_per_query(voted)[0].tolist())
    fate = c.facts["fate"]
    assert len(fate) == len(_per_query(unvoted)[0])
    for _, key, stays in fate:
        assert (key in kv) == stays, hex(key)
