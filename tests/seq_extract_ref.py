"""telr_seqset_extract in plain Python over host strings (the checker of tests/test_gpu_seq_extract.py; include/telr_hip.h has the
definition): piece k is bases [start[k], start[k] + len[k]) of sequence idx[k] as a sequence set holds them -- A C G T (either case, U
as T), anything else N -- reverse-complemented where rc[k] != 0, the complement of N being N.  Pieces may repeat, overlap and come in
any order; a length of 0 is an empty piece.  What the engine refuses raises ValueError with the engine's text."""

_HELD = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "a": "A", "c": "C", "g": "G", "t": "T", "u": "T"}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def held(seq):
    """a sequence as a set holds it"""
    s = seq.decode("latin-1") if isinstance(seq, (bytes, bytearray)) else seq
    return "".join(_HELD.get(c, "N") for c in s)


def extract(seqs, idx, start, length, rc=None):
    """-> list of bytes, one per piece"""
    n = len(idx)
    if len(start) != n or len(length) != n or (rc is not None and len(rc) != n):
        raise ValueError("one start, one length and one rc flag per index")
    out = []
    for k in range(n):
        i, s, l = int(idx[k]), int(start[k]), int(length[k])
        who = "piece %d: " % k
        if i < 0 or i >= len(seqs):
            raise ValueError(who + "idx outside the set")
        if s < 0:
            raise ValueError(who + "negative start")
        if l < 0:
            raise ValueError(who + "negative len")
        if s + l > len(seqs[i]):
            raise ValueError(who + "start + len beyond the sequence")
        piece = held(seqs[i])[s:s + l]
        if rc is not None and rc[k]:
            piece = "".join(_COMP[c] for c in reversed(piece))
        out.append(piece.encode())
    return out
