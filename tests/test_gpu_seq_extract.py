"""telr_seqset_extract on the device == its definition in plain Python (tests/seq_extract_ref.py), byte for byte: every start and length
around the 16-base unit, the 16-base code word, the 32-base mask word and the 64-base padding of a sequence, forward and reverse
complement, with N on those seams; the orderings; the refusals; and agreement with the two kernels that cut pieces privately
(k_bam_ascii: BamInput.reads(); k_draft_extract: the contig set of draft_contigs)."""
import numpy as np
import pytest

import packed_np
import seq_extract_ref as xref
from telr_amd._abi import MF_KEEP_CIGARS, TELR_E_ARG
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 200, 0)                 # (seqset accepts an empty sequence: the last one)
N_AT = (0, 15, 16, 31, 32, 63, 64)
STARTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64)
LENS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, "end")


def make_seqs():
    rng = np.random.RandomState(7)
    seqs = []
    for n in LENGTHS:
        s = rng.choice(list("ACGT"), n).tolist()
        for p in N_AT + (n - 1,):
            if 0 <= p < n:
                s[p] = "N"
        seqs.append("".join(s))
    return seqs


def grid_pieces(seqs):
    """every start x every length that fits, forward and rc -> (idx, start, len, rc) lists"""
    out = []
    for i, s in enumerate(seqs):
        for st in STARTS:
            for ln in LENS:
                ln = len(s) - st if ln == "end" else ln
                if st <= len(s) and ln >= 0 and st + ln <= len(s):
                    out.append((i, st, ln, 0))
                    out.append((i, st, ln, 1))
    out = sorted(set(out))
    return [list(c) for c in zip(*out)]


@pytest.fixture(scope="module")
def small(engine):
    seqs = make_seqs()
    s = engine.seqset(seqs)
    idx, start, ln, rc = grid_pieces(seqs)
    yield dict(seqs=seqs, set=s, idx=idx, start=start, len=ln, rc=rc, want=xref.extract(seqs, idx, start, ln, rc))
    s.free()


def test_the_set_is_what_the_issue_names(small):
    seqs = small["seqs"]
    assert [len(s) for s in seqs] == list(LENGTHS)
    assert [i for i, c in enumerate(seqs[4]) if c == "N"] == [0, 15, 16, 31, 32, 63, 64, 199]
    assert seqs[0] == "N" and seqs[2][63] == "N" and seqs[3][64] == "N"
    got = set(zip(small["idx"], small["start"], small["len"], small["rc"]))
    assert len(got) > 400
    for st in STARTS:                              # the long sequence takes every start with every length, and "to the end"
        for ln in LENS:
            ln = 200 - st if ln == "end" else ln
            assert (4, st, ln, 0) in got and (4, st, ln, 1) in got
    assert (5, 0, 0, 0) in got and (5, 0, 0, 1) in got and (0, 1, 0, 1) in got and (3, 64, 1, 1) in got


def test_every_start_and_length_in_one_call(small):
    got = small["set"].extract(small["idx"], small["start"], small["len"], small["rc"])
    assert got == small["want"]
    assert any(b"N" in g for g in got) and sum(len(g) for g in got) > 10000


def test_descending_and_doubled(small):
    order = [k for k in reversed(range(len(small["idx"]))) for _ in (0, 1)]
    pick = lambda a: [a[k] for k in order]
    got = small["set"].extract(pick(small["idx"]), pick(small["start"]), pick(small["len"]), pick(small["rc"]))
    assert got == pick(small["want"])


def test_whole_sequences_one_piece_and_none(small):
    seqs, s = small["seqs"], small["set"]
    n = len(seqs)
    assert s.extract(range(n), [0] * n, [len(x) for x in seqs]) == [x.encode() for x in seqs]                      # rc None: all forward
    assert s.extract(range(n), [0] * n, [len(x) for x in seqs], [1] * n) == xref.extract(seqs, range(n), [0] * n, [len(x) for x in seqs], [1] * n)
    assert s.extract([4], [17], [65], [1]) == xref.extract(seqs, [4], [17], [65], [1])
    assert s.extract([4], [199], [1]) == [b"N"]
    assert s.extract([], [], []) == [] and s.extract([], [], [], []) == []
    assert s.extract([5, 0], [0, 1], [0, 0], [1, 0]) == [b"", b""]                                                  # only empty pieces


def test_1025_one_base_pieces(small):
    seqs = small["seqs"]
    idx = [4] * 1025
    start = [(7 * k) % 200 for k in range(1025)]
    rc = [k & 1 for k in range(1025)]
    got = small["set"].extract(idx, start, [1] * 1025, rc)
    assert got == xref.extract(seqs, idx, start, [1] * 1025, rc) and set(got) == {b"A", b"C", b"G", b"T", b"N"}


def test_same_bytes_on_every_run(small):
    runs = [b"|".join(small["set"].extract(small["idx"], small["start"], small["len"], small["rc"])) for _ in range(2)]
    assert runs[0] == runs[1] == b"|".join(small["want"])


def test_refusals_leave_the_output_untouched(engine, small):
    seqs, s, L = small["seqs"], small["set"], engine.L

    def call(n, idx, start, ln, rc, out_off, null=None):
        a = dict(idx=np.array(idx, np.int32), start=np.array(start, np.int32), len=np.array(ln, np.int32),
                 rc=None if rc is None else np.array(rc, np.uint8), off=np.array(out_off, np.int64))
        out = np.full(256, 0x5A, np.uint8)
        p = {k: (None if v is None or k == null else v.ctypes.data) for k, v in a.items()}
        code = L.telr_seqset_extract(engine.h, s.h, n, p["idx"], p["start"], p["len"], p["rc"], None if null == "out" else out.ctypes.data, p["off"])
        return code, out, L.telr_last_error(engine.h)

    def refused(text, *a, **kw):
        code, out, msg = call(*a, **kw)
        assert code == TELR_E_ARG, (code, msg)
        assert b"telr_seqset_extract" in msg and text in msg, msg
        assert (out == 0x5A).all()

    good = (2, [4, 1], [3, 0], [5, 2], [0, 1], [0, 5, 7])
    code, out, _ = call(*good)
    assert code == 0 and out[:7].tobytes() == b"".join(xref.extract(seqs, *good[1:5])) and (out[7:] == 0x5A).all()
    refused(b"negative n", -1, *good[1:])
    refused(b"piece 1: idx outside", 2, [4, 6], *good[2:])
    refused(b"piece 0: idx outside", 2, [-1, 1], *good[2:])
    refused(b"piece 1: negative start", 2, [4, 1], [3, -1], *good[3:])
    refused(b"piece 0: negative len", 2, [4, 1], [3, 0], [-5, 2], [0, 1], [0, -5, -3])
    refused(b"piece 0: start + len beyond", 2, [4, 1], [196, 0], *good[3:])
    refused(b"piece 1: start + len beyond", 2, [4, 5], [3, 0], [5, 1], [0, 1], [0, 5, 6])                            # the empty sequence holds no base
    refused(b"piece 1: out_off does not match", 2, *good[1:5], [0, 5, 8])
    refused(b"piece 0: out_off does not match", 2, *good[1:5], [1, 5, 7])
    refused(b"negative out_off", 2, *good[1:5], [-1, 4, 6])
    for null in ("idx", "start", "len", "off", "out"):
        refused(b"null", *good, null=null)
    assert L.telr_seqset_extract(engine.h, None, 1, None, None, None, None, None, None) == TELR_E_ARG                # a null set
    # n == 0 touches nothing, whatever the pointers; the Python layer raises TelrError with the code
    code, out, _ = call(0, [], [], [], None, [0], null="out")
    assert code == 0 and (out == 0x5A).all()
    with pytest.raises(TelrError) as e:
        s.extract([4], [190], [11])
    assert e.value.code == TELR_E_ARG and "beyond the sequence" in str(e.value)


def test_pieces_beyond_2_31_bases(engine):
    """the base offsets are 64-bit: a set of 33 x 2^26 bases made of device words (all A), a 200-base pattern with N planted in its last
    sequence, which starts at base 2^31 of the layout; pieces of the pattern forward and rc, and the last 20 bases of the set"""
    import torch
    from telr_amd.aligner import SeqSet
    n, each = 33, 1 << 26
    total = n * each
    assert (n - 1) * each == 1 << 31
    rng = np.random.RandomState(3)
    pat = "".join(rng.choice(list("ACGTN"), 200, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    _, w2, wn = packed_np.pack([pat])
    dev = "cuda:%d" % engine.device
    seq2 = torch.zeros(total // 16, dtype=torch.int32, device=dev)
    nmask = torch.zeros(total // 32, dtype=torch.int32, device=dev)
    at = (n - 1) * each + 64 * 5                      # where the pattern starts in the layout
    seq2[at // 16:at // 16 + len(w2)] = torch.from_numpy(w2.view(np.int32)).to(dev)
    nmask[at // 32:at // 32 + len(wn)] = torch.from_numpy(wn.view(np.int32)).to(dev)
    s = SeqSet.from_packed(engine, [each] * n, seq2, nmask)
    del seq2, nmask
    try:
        idx, start, ln, rc = [n - 1] * 4 + [n - 1, n - 1, 0], [320, 323, 320 + 17, 300, each - 20, each - 20, 5], [200, 150, 33, 250, 20, 20, 40], [0, 1, 1, 0, 0, 1, 1]
        head = "A" * 320 + pat + "A" * 56              # the first bases of the last sequence (the pattern's 64-base padding is A too)
        want = xref.extract([head], [0] * 4, start[:4], ln[:4], rc[:4]) + [b"A" * 20, b"T" * 20, b"T" * 40]
        assert s.extract(idx, start, ln, rc) == want and b"N" in want[0]
    finally:
        s.free()


# ---- agreement with the two kernels that cut pieces privately ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(engine, data_dir):
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-pb")
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    ix = engine.index(ts, io)
    qset = engine.seqset(qs)
    r = ix.map_raw(qset, mo)
    yield dict(ix=ix, r=r, tn=tn, qn=qn, qs=qs, qset=qset)
    ix.free_raw(r)


def test_whole_reads_of_a_loaded_bam_equal_its_text(engine, bundled, tmp_path):
    b = bundled
    path = str(tmp_path / "in.bam")
    b["ix"].write_bam_device(b["r"], b["qset"], b["qn"], b["tn"], path, cmdline="t", level=1)
    bi = engine.load_bam(path)
    try:
        buf, off, ln = bi.reads()
        n = bi.read_set.n
        assert n == len(b["qs"]) and sorted(bi.qnames) == sorted(b["qn"])
        got = bi.read_set.extract(range(n), [0] * n, ln)
        assert got == [buf[int(o):int(o) + int(l)].tobytes() for o, l in zip(off, ln)]
        assert sorted(got) == sorted(xref.held(s).encode() for s in b["qs"])
    finally:
        bi.free()


def test_draft_pieces_equal_the_contig_set(engine, bundled):
    b = bundled
    ic = b["ix"].call_insertions(b["r"])
    d, cset = b["ix"].draft_contigs(b["r"], ic, b["qset"])
    try:
        have = d[d["sig"] >= 0]
        assert len(have) == cset.n >= 1
        got = b["qset"].extract(have["qid"], have["start"], have["len"], have["rc"])
        w2, wn = cset.packed()
        decoded = packed_np.unpack(cset.len, w2.cpu().numpy(), wn.cpu().numpy())          # the contig set, decoded with numpy
        assert [g.decode() for g in got] == decoded
        assert got == cset.extract(range(cset.n), [0] * cset.n, cset.len)
        assert got == xref.extract(b["qs"], have["qid"], have["start"], have["len"], have["rc"])
        assert any(have["rc"]) and len(got[0]) > 5000
    finally:
        cset.free()
