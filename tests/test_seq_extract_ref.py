"""The checker of telr_seqset_extract (tests/seq_extract_ref.py) against answers written out by hand, and against the draft step's
checker: the piece a draft names is the draft's sequence."""
import pytest

import draft_ref as dref
import inscall_ref as iref
import seq_extract_ref as xref
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

#       0         1
#       01234567890123456789
READ = "NCGTACGNTTGCAAGGCTTN"          # 20 bases, N at 0, 7 and 19

# (start, len) -> (forward, reverse complement), each written out by hand
HAND = {(0, 20): ("NCGTACGNTTGCAAGGCTTN", "NAAGCCTTGCAANCGTACGN"),
        (7, 1): ("N", "N"),
        (6, 3): ("GNT", "ANC"),
        (19, 1): ("N", "N"),
        (5, 0): ("", "")}


def test_hand_written_pieces():
    assert len(READ) == 20 and [i for i, c in enumerate(READ) if c == "N"] == [0, 7, 19]
    keys = sorted(HAND)
    for rc in (0, 1):
        got = xref.extract([READ], [0] * len(keys), [k[0] for k in keys], [k[1] for k in keys], [rc] * len(keys))
        assert got == [HAND[k][rc].encode() for k in keys]
    # rc None is all forward; pieces repeat and come in any order; other letters read as the set holds them
    assert xref.extract([READ], [0, 0, 0], [6, 0, 6], [3, 20, 3]) == [b"GNT", READ.encode(), b"GNT"]
    assert xref.extract(["acgurykU", b"ACGT"], [0, 1], [0, 1], [8, 2], [0, 1]) == [b"ACGTNNNT", b"CG"]


@pytest.mark.parametrize("bad, text", [(dict(idx=[1]), "idx outside"), (dict(idx=[-1]), "idx outside"), (dict(start=[-1]), "negative start"),
                                       (dict(length=[-1]), "negative len"), (dict(start=[18], length=[3]), "beyond the sequence")])
def test_refusals(bad, text):
    a = dict(idx=[0], start=[0], length=[1])
    a.update(bad)
    with pytest.raises(ValueError, match=text):
        xref.extract([READ], a["idx"], a["start"], a["length"])


@pytest.mark.parametrize("name", ["map-pb", "map-ont", "ngmlr-pacbio"])
def test_a_drafts_piece_is_its_sequence(data_dir, name):
    from oracle import binding as ob
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset(name)
    r = ob.OracleIndex(ts, io).map(qs, mo)
    sigs, calls = iref.call_insertions(r["alns"], r["cigars"])
    drafts, seqs = dref.drafts(r["alns"], r["cigars"], calls, sigs, qs)
    have = [d for d in drafts if d["sig"] >= 0]
    assert len(have) == len(seqs) >= 1
    got = xref.extract(qs, [d["qid"] for d in have], [d["start"] for d in have], [d["len"] for d in have], [d["rc"] for d in have])
    assert [g.decode() for g in got] == list(seqs)
