"""The reference TE annotation on the device == its definition in plain Python: SeqSet.pieces against
tests/seq_extract_ref.py (and telr_draft_contigs, which cuts its set with the same function now, against what it returned before),
telr_annotate_hits on every case of tests/refte_cases.py against tests/refte_ref.py, annotate_reference on the planted reference, and
the `telr` command with --ref_te."""
import ctypes as C
import os

import numpy as np
import pytest

import packed_np
import refte_cases as rc
import refte_ref as ref
import seq_extract_ref as sx
from telr_amd import telr, telr_te
from telr_amd._abi import ALN_DTYPE, MF_CIGAR, MF_KEEP_CIGARS, RefTeOpt, TE_FEAT_DTYPE, TELR_E_ARG, TILE_DTYPE
from telr_amd._lib import TelrError
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset

pytestmark = pytest.mark.gpu

FEAT_FIELDS = ("tid", "start", "end", "family", "strand", "score", "n_hits")


def feats_as_tuples(f):
    assert f.dtype == TE_FEAT_DTYPE
    return [tuple(int(x[k]) for k in FEAT_FIELDS) for x in f]


# ---- SeqSet.pieces ----------------------------------------------------------------------------------------------------------------------
def piece_parents():
    rng = np.random.RandomState(5)
    a = "".join(rng.choice(list("ACGT"), 5000))
    b = list("".join(rng.choice(list("ACGT"), 700)))
    for p in (0, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 164, 699):          # N where the pieces below start and end
        b[p] = "N"
    return [a, "".join(b), "ACGTN" * 13, "G"]


def piece_list(seqs):
    starts = (0, 15, 16, 17, 31, 32, 33, 63, 64, 65)
    lens = (0, 1, 15, 16, 17, 64, 65)
    P = [(0, s, l, r) for s in starts for l in lens for r in (0, 1)]
    P += [(1, s, l, r) for s in starts for l in lens for r in (0, 1)]                      # first / last base N: (s, l) = (0, 1), (15, 1), (15, 17): 15..31, ...
    P += [(1, 100, 65, 0), (1, 100, 65, 1), (1, 0, 700, 1), (1, 164, 536, 0)]              # N at the first and at the last base of a piece
    P += [(0, 7, 4321, 0), (0, 7, 4321, 1), (0, 0, 5000, 1), (0, 679, 4321, 0)]            # a few kb
    P += [(2, 3, 30, 1)] * 3 + [(2, 0, 65, 0), (2, 10, 40, 0), (2, 20, 45, 1), (3, 0, 1, 0), (3, 0, 1, 1), (3, 1, 0, 0), (3, 0, 0, 1)]      # repeated, overlapping, empty
    return P


def test_pieces_equal_the_definition(engine):
    seqs = piece_parents()
    parent = engine.seqset(seqs)
    P = piece_list(seqs)
    idx, start, length, rcf = (np.array([p[k] for p in P], np.int32) for k in range(4))
    want = sx.extract(seqs, idx, start, length, rcf)
    assert any(w[:1] == b"N" and w[-1:] == b"N" and len(w) > 1 for w in want) and any(len(w) == 0 for w in want)
    s = parent.pieces(idx, start, length, rc=rcf)
    try:
        assert s.n == len(P) and s.bases() == int(length.sum()) and not s.has_qual
        np.testing.assert_array_equal(s.len, length)
        got = s.extract(np.arange(len(P)), np.zeros(len(P), np.int32), length)
        assert got == want
        # the layout of any other set: the packed words are what the packer makes of the pieces, padding included
        w2, wn = s.packed()
        e_len, e2, en = packed_np.pack([w.decode() for w in want])
        np.testing.assert_array_equal(w2.cpu().numpy().view(np.uint32), e2)
        np.testing.assert_array_equal(wn.cpu().numpy().view(np.uint32), en)
        # rc None = all forward; a piece of a piece
        f = parent.pieces(idx, start, length)
        assert f.extract(np.arange(len(P)), np.zeros(len(P), np.int32), length) == sx.extract(seqs, idx, start, length)
        f.free()
        k = P.index((0, 7, 4321, 1))
        pp = s.pieces([k, k], [100, 0], [1000, 4321], rc=[1, 0])
        assert pp.extract([0, 1], [0, 0], [1000, 4321]) == sx.extract([want[k]], [0, 0], [100, 0], [1000, 4321], [1, 0])
        pp.free()
        # no pieces: an empty set
        e = parent.pieces([], [], [])
        assert e.n == 0 and e.bases() == 0
        e.free()
    finally:
        s.free(); parent.free()


def test_pieces_refused_arguments(engine):
    seqs = piece_parents()
    parent = engine.seqset(seqs)
    try:
        for idx, start, length, text in (([4], [0], [1], "idx outside the set"), ([-1], [0], [1], "idx outside the set"), ([0], [-1], [1], "negative start"),
                                         ([0], [0], [-1], "negative len"), ([0], [4990], [11], "start + len beyond the sequence"),
                                         ([3], [1], [1], "start + len beyond the sequence"), ([0, 1], [0, 690], [10, 11], "piece 1")):
            with pytest.raises(TelrError) as e:
                parent.pieces(idx, start, length)
            assert e.value.code == TELR_E_ARG and "telr_seqset_pieces" in str(e.value) and text in str(e.value)
            with pytest.raises(ValueError):
                sx.extract(seqs, idx, start, length)
        with pytest.raises(ValueError):
            parent.pieces([0], [0, 1], [1])
        L = engine.L
        h = C.c_void_p()
        one = np.zeros(1, np.int32)
        assert L.telr_seqset_pieces(engine.h, parent.h, -1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_seqset_pieces(engine.h, parent.h, 1, None, one.ctypes.data, one.ctypes.data, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_seqset_pieces(engine.h, None, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, C.byref(h)) == TELR_E_ARG
        assert L.telr_seqset_pieces(engine.h, parent.h, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, None) == TELR_E_ARG
    finally:
        parent.free()


def test_draft_contigs_returns_the_set_it_returned(engine, data_dir):
    """telr_draft_contigs cuts its set with the function telr_seqset_pieces uses: on the bundled reads the draft is the one
    tests/test_draft_ref.py pins (BUNDLED) and its set the sequence the plain-Python definition gives over the oracle's records"""
    import draft_ref as dref
    import inscall_ref as iref
    import test_draft_ref as cpu
    from oracle import binding as ob
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    qn, qs = read_fasta(data_dir + "/reads.fasta")
    io, mo = preset("map-pb")
    want = ob.OracleIndex(ts, io).map(qs, mo)
    sigs, calls = iref.call_insertions(want["alns"], want["cigars"])
    wd, wseq = dref.drafts(want["alns"], want["cigars"], calls, sigs, qs)
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    ix = engine.index(ts, io)
    qset = engine.seqset(qs)
    r = ix.map_raw(qset, mo)
    try:
        d, s = ix.draft_contigs(r, ix.call_insertions(r), qset)
        assert len(d) == 1 and {k: int(d[0][k]) for k in cpu.BUNDLED["map-pb"] if k != "n_candidates"} == {k: v for k, v in cpu.BUNDLED["map-pb"].items() if k != "n_candidates"}
        w2, wn = s.packed()
        e_len, e2, en = packed_np.pack(wseq)
        np.testing.assert_array_equal(s.len, e_len)
        np.testing.assert_array_equal(w2.cpu().numpy().view(np.uint32), e2)
        np.testing.assert_array_equal(wn.cpu().numpy().view(np.uint32), en)
        # ... and equals the same piece cut by SeqSet.pieces
        p = qset.pieces([d[0]["qid"]], [d[0]["start"]], [d[0]["len"]], rc=[d[0]["rc"]])
        for x, y in zip(p.packed(), s.packed()):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        p.free(); s.free()
    finally:
        ix.free_raw(r); qset.free(); ix.free()


# ---- telr_annotate_hits -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_ix(engine):
    """result_from_arrays hangs off an index; the step itself needs none"""
    io, _ = preset("map-ont")
    return engine.index(["ACGT" * 64], io)


def annotate(engine, lib_ix, c, opt=None):
    r = lib_ix.result_from_arrays(c["alns"], np.zeros(0, np.uint32))
    try:
        return engine.annotate_hits(r, c["tiles"], c["target_len"], c["n_families"], RefTeOpt.default(**(c["opt"] if opt is None else opt)))
    finally:
        lib_ix.free_raw(r)


@pytest.mark.parametrize("c", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_annotate_hits_equals_the_definition(engine, lib_ix, c):
    want = ref.features(ref.hits(c["alns"], [tuple(int(x) for x in t) for t in c["tiles"]], c["opt"]), c["opt"])
    got = annotate(engine, lib_ix, c)
    assert feats_as_tuples(got) == want
    assert annotate(engine, lib_ix, c).tobytes() == got.tobytes()          # the same bytes on every run


def test_annotate_hits_defaults_and_refused_arguments(engine, lib_ix):
    o = RefTeOpt()
    engine.L.telr_refte_opt_default(C.byref(o))
    assert (o.min_len, o.min_mapq, o.join_gap, o.reserved) == (100, 0, 0, 0) == tuple(getattr(RefTeOpt.default(), k) for k, _ in RefTeOpt._fields_)
    assert {k: getattr(o, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    with pytest.raises(TypeError):
        RefTeOpt.default(nope=1)
    base = next(c for c in rc.CASES if c["name"] == "tile offsets")
    # opt NULL = the defaults
    r = lib_ix.result_from_arrays(base["alns"], np.zeros(0, np.uint32))
    try:
        h = C.c_void_p()
        tiles, tl = np.ascontiguousarray(base["tiles"]), base["target_len"]
        args = (len(tiles), tiles.ctypes.data, len(tl), tl.ctypes.data, 1)
        assert engine.L.telr_annotate_hits(engine.h, r, *args, None, C.byref(h)) == 0
        assert engine.L.telr_te_feats_count(h) == 2
        engine.L.telr_te_feats_free(h)
        assert engine.L.telr_annotate_hits(engine.h, None, *args, None, C.byref(h)) == TELR_E_ARG
        assert engine.L.telr_annotate_hits(engine.h, r, *args, None, None) == TELR_E_ARG
        assert engine.L.telr_te_feats_count(None) == 0 and not engine.L.telr_te_feats_data(None)
    finally:
        lib_ix.free_raw(r)

    def changed(**kw):
        c = dict(base, alns=base["alns"].copy(), tiles=base["tiles"].copy(), target_len=base["target_len"].copy())
        for k, v in kw.items():
            if k in ("alns", "tiles"):
                i, f, x = v
                c[k][i][f] = x
            else:
                c[k] = v
        return c
    for c, opt, text in ((base, dict(min_len=-1), "negative option"), (base, dict(min_mapq=-1), "negative option"), (base, dict(join_gap=-1), "negative option"),
                         (base, dict(reserved=-1), "negative option"), (changed(alns=(0, "qid", 4)), None, "qid outside the tiles"),
                         (changed(alns=(1, "qid", -1)), None, "qid outside the tiles"), (changed(alns=(2, "tid", 1)), None, "tid outside n_families"),
                         (changed(alns=(2, "tid", -1)), None, "tid outside n_families"), (changed(tiles=(3, "len", 3857)), None, "outside its target"),
                         (changed(tiles=(0, "tid", 1)), None, "outside its target"), (changed(tiles=(1, "start", -1)), None, "outside its target"),
                         (changed(alns=(0, "qe", 3857)), None, "qe beyond its tile"), (changed(alns=(1, "qs", 2553)), None, "coordinates"),
                         (changed(alns=(1, "qs", -1)), None, "coordinates"), (changed(target_len=np.array([-1], np.int32)), None, "negative length")):
        with pytest.raises(TelrError) as e:
            annotate(engine, lib_ix, c, opt)
        assert e.value.code == TELR_E_ARG and "telr_annotate_hits" in str(e.value) and text in str(e.value), str(e.value)
    # an ineligible record is checked like any other, and a refused call leaves the next one alone
    sec = changed(alns=(0, "flags", 2))
    sec["alns"][0]["qe"] = 3857
    with pytest.raises(TelrError):
        annotate(engine, lib_ix, sec)
    assert feats_as_tuples(annotate(engine, lib_ix, base)) == base["expect"]


# ---- annotate_reference on the planted reference ----------------------------------------------------------------------------------------
def test_annotate_reference_on_the_planted_reference(engine):
    P = rc.planted()
    tset = engine.seqset([P["ref"]])
    try:
        rows = telr_te.annotate_reference(engine, tset, ["chrP"], P["lib_names"], P["lib_seqs"], tile=rc.PLANT_TILE, stride=rc.PLANT_STRIDE)
        assert rows == [["chrP", str(s), str(e), P["lib_names"][f], ".", "-" if st else "+"] for s, e, f, st in P["plants"]]
        rows1 = telr_te.annotate_reference(engine, tset, ["chrP"], P["lib_names"], P["lib_seqs"], tile=rc.PLANT_TILE, stride=rc.PLANT_STRIDE,
                                           opt=RefTeOpt.default(join_gap=1))
        assert rows1 == [["chrP", str(s), str(e), P["lib_names"][f], ".", "-" if st else "+"] for s, e, f, st in rc.planted_joined(P["plants"])]
        # the definition applied to the engine's own records
        tiles = engine.tile_plan(tset.len, rc.PLANT_TILE, rc.PLANT_STRIDE)
        assert [tuple(int(x) for x in t) for t in tiles] == ref.tile_plan([len(P["ref"])], rc.PLANT_TILE, rc.PLANT_STRIDE)
        io, mo = preset("map-ont")
        mo = mo.copy(); mo.bw_long = 0; mo.secondary = 0; mo.flags |= MF_CIGAR
        lib = engine.index(P["lib_seqs"], io)
        q = tset.pieces(tiles["tid"], tiles["start"], tiles["len"])
        r = lib.map_raw(q, mo)
        try:
            alns = lib.result_arrays(r).alns
            for opt in (dict(), dict(join_gap=1), dict(min_len=3000), dict(min_mapq=61)):
                want = ref.features(ref.hits(alns, [tuple(int(x) for x in t) for t in tiles], opt), opt)
                assert feats_as_tuples(engine.annotate_hits(r, tiles, tset.len, 3, RefTeOpt.default(**opt))) == want
            assert len(alns) >= len(P["plants"])
        finally:
            lib.free_raw(r); q.free(); lib.free()
    finally:
        tset.free()


# ---- the command ------------------------------------------------------------------------------------------------------------------------
MM2 = ("--aligner", "minimap2", "-x", "pacbio", "--polish", "poa")


def argv_for(data_dir, out, *extra):
    return ["-i", data_dir + "/reads.fasta", "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out)] + list(extra)


def without_sequences(final):
    return [{k: v for k, v in f.items() if k not in ("te_sequence",)} for f in final]


def test_telr_with_ref_te(engine, data_dir, tmp_path, capsys):
    out = tmp_path / "engine"
    res = telr.run(telr.get_args(argv_for(data_dir, out, *MM2, "-k", "--ref_te", "engine")), engine=engine)
    bed = out / "intermediate_files" / "ref_38kb.fasta.te.bed"
    assert res["files"]["ref_te"] == str(bed) and bed.exists()
    rows = telr_te.read_te_bed(str(bed))
    assert res["counts"]["ref_te_features"] == len(rows) and "ref_te" in res["seconds"] and res["seconds"]["ref_te"] >= 0
    assert list(res["seconds"]).index("ref_te") == list(res["seconds"]).index("index10") + 1
    # ... equals annotate_reference called directly
    tn, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    ln, ls = read_fasta(data_dir + "/library.fasta")
    tset = engine.seqset(ts)
    direct = telr_te.annotate_reference(engine, tset, tn, ln, ls)
    tset.free()
    assert rows == direct and open(str(bed)).read() == "".join("\t".join(r) + "\n" for r in direct)
    for r in rows:
        assert len(r) == 6 and r[0] in tn and 0 <= int(r[1]) < int(r[2]) <= len(ts[tn.index(r[0])]) and r[3] in ln and r[4] == "." and r[5] in "+-"
    print("reference TE features:", rows)
    print("final rows with --ref_te engine:", without_sequences(res["final"]), res["counts"])          # recorded in DESIGN.md 5.15; nothing is asserted about the jockey row
    # the outputs parse
    body = [l.split("\t") for l in open(res["files"]["vcf"]).read().splitlines() if not l.startswith("#")]
    assert len(body) == res["counts"]["loci_written"] == len(open(res["files"]["bed"]).read().splitlines()) == len(res["final"])
    for row in body:
        assert len(row) == 10 and int(row[1]) > 0
    head = [l for l in open(res["files"]["vcf"]).read().splitlines() if l.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.1" and head[-1].startswith("#CHROM")
    # --ref_te FILE with that BED: the same final rows
    res2 = telr.run(telr.get_args(argv_for(data_dir, tmp_path / "file", *MM2, "--ref_te", str(bed))), engine=engine)
    assert res2["final"] == res["final"] and res2["counts"]["ref_te_features"] == len(rows) and "ref_te" in res2["seconds"]
    assert res2["files"]["ref_te"] == str(bed)
    # the default is `none`: no stage, no count, no file
    a = telr.get_args(argv_for(data_dir, tmp_path / "none", *MM2))
    assert a.ref_te == "none"
    # an unreadable FILE: the message of the other inputs, status 1
    with pytest.raises(SystemExit) as e:
        telr.get_args(argv_for(data_dir, tmp_path / "bad", *MM2, "--ref_te", str(tmp_path / "no_such.bed")))
    assert e.value.code == 1 and "Can not open input file" in capsys.readouterr().err
    # a FILE that opens but is no BED6: a message and status 1 as well
    (tmp_path / "short.bed").write_text("chr2L\t5\t9\n")
    with pytest.raises(SystemExit) as e:
        telr.get_args(argv_for(data_dir, tmp_path / "bad", *MM2, "--ref_te", str(tmp_path / "short.bed")))
    assert e.value.code == 1 and "valid BED6" in capsys.readouterr().out
