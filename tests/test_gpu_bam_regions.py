"""telr_bam_load_regions on the device == the definition (tests/bam_region_ref.py), array for array: names, lengths, packed words, mask,
qualities, records, CIGAR words, the counters and region_info, on the generated file of about 500 records whose BGZF seams lie inside
records (tests/test_bam_region_ref.py holds every case to the edge it claims); the refusals with their codes; the other two loads
untouched by a region load on the same engine; and the `telr` command with --region."""
import os
import shutil
import struct

import numpy as np
import pytest

import bam_in_ref as R
import bam_reference as BR
import bam_region_ref as G
from test_gpu_bam_in import loaded_equals
from telr_amd import aligner, telr
from telr_amd._lib import TelrError

pytestmark = pytest.mark.gpu

CASES = G.cases()
BY_NAME = {c["name"]: c for c in CASES}
_REF = {}


def definition(case):
    if case["name"] not in _REF:
        F = G.layout(case["layout"])
        _REF[case["name"]] = G.load(F["data"], F["bai"], case["regions"], case["keep_qual"])
    return _REF[case["name"]]


def snapshot(engine, bi, members=True):
    """everything a load leaves, as bytes"""
    m = bi.map_result()
    c = dict(bi.counters)
    if not members:
        c.pop("members")
    out = [bi.tnames, [int(x) for x in bi.tlens], bi.qnames, c, m.alns.tobytes(), m.cigars.tobytes(), bi.read_set.len.tobytes(), bi.read_set.has_qual]
    if bi.read_set.n:
        w2, wn = bi.read_set.packed()
        out += [w2.cpu().numpy().tobytes(), wn.cpu().numpy().tobytes()]
    if bi.read_set.has_qual:
        tot = int(((bi.read_set.len.astype(np.int64) + 63) // 64 * 64).sum())
        q = np.zeros(tot, np.uint8)
        assert engine.L.telr_debug_seqset_qual(bi.read_set.h, q.ctypes.data, tot) == tot
        out.append(q.tobytes())
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """layout name -> path of its BAM, the .bai next to it"""
    d = tmp_path_factory.mktemp("bam_regions")
    out = {}
    for name in sorted({c["layout"] for c in CASES}):
        F = G.layout(name)
        out[name] = str(d / (name + ".bam"))
        open(out[name], "wb").write(F["data"])
        open(out[name] + ".bai", "wb").write(F["bai"])
    return out


def load(engine, files, case, **kw):
    args = dict(keep_qual=case["keep_qual"], chunk_bytes=case["chunk_bytes"], regions=case["regions"])
    args.update(kw)
    return engine.load_bam(files[case["layout"]], **args)


# ---- 1. the case table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case(engine, files, case):
    L = definition(case)
    bi = load(engine, files, case)
    info, chunks = bi.region_info, bi.chunk_info
    print(case["name"], info, chunks, bi.counters)
    loaded_equals(engine, bi, L)
    bi.free()
    assert info == L.region_info
    if info["members"] == 0:
        assert chunks["chunks"] == 0
    elif case["chunk_bytes"] == 1:                  # every member is a chunk, and records straddle members: the carry goes on
        assert chunks["chunks"] == info["members"] and chunks["largest_carry"] > 0
    elif case["chunk_bytes"] >= 1 << 40:
        assert chunks["chunks"] == 1 and chunks["largest_carry"] == 0
    if case["name"].startswith("qualities"):
        assert chunks["chunks"] > 1


def test_every_target_is_the_whole_file_load(engine, files):
    """regions over every target, no unmapped record in the file: telr_bam_load's result (members apart: the EOF marker is no interval's);
    with unmapped records added to the file they vanish and nothing else changes"""
    whole = engine.load_bam(files["mid"], keep_qual=True)
    want = snapshot(engine, whole, members=False)
    assert whole.region_info == dict.fromkeys(G.REGION_INFO, 0)
    whole.free()
    for name in ("every_target", "every_target_unmapped_added"):
        bi = load(engine, files, BY_NAME[name])
        assert snapshot(engine, bi, members=False) == want, name
        bi.free()


def test_same_bytes_on_two_runs(engine, files):
    for name in ("many_intervals_one_chunk", "every_member_a_chunk"):
        snaps = []
        for _ in range(2):
            bi = load(engine, files, BY_NAME[name])
            snaps.append(snapshot(engine, bi) + [bi.region_info])
            bi.free()
        assert snaps[0] == snaps[1]


def test_growing_and_shrinking_lists_on_one_engine(engine, files):
    """small, large, small again on one engine == each on an engine of its own: nothing of a load's buffers leaks into the next"""
    order = ["end_behind_pos", "short_intervals_next_to_a_long_one", "every_member_a_chunk", "orphan", "many_intervals_one_chunk", "zero_regions", "w16_left"]
    got = []
    for name in order:
        bi = load(engine, files, BY_NAME[name])
        got.append(snapshot(engine, bi) + [bi.region_info])
        bi.free()
    for name, have in zip(order, got):
        fresh = aligner.Engine(0)
        bi = load(fresh, files, BY_NAME[name])
        assert snapshot(fresh, bi) + [bi.region_info] == have, name
        bi.free(); fresh.close()


def test_explicit_index_path(engine, files, tmp_path):
    case = BY_NAME["w16_left"]
    p = tmp_path / "elsewhere.idx"
    p.write_bytes(G.layout("mid")["bai"])
    bam = tmp_path / "alone.bam"
    bam.write_bytes(G.layout("mid")["data"])
    bi = engine.load_bam(str(bam), regions=case["regions"], bai=str(p))
    loaded_equals(engine, bi, definition(case))
    bi.free()


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def moved_chunk_bai():
    """the `per_record` index with w30's chunk start moved 9 bytes into the record"""
    F = G.layout("per_record")
    k = F["names"].index("w30")
    members = G.member_table(F["data"])
    old, new = G.voffset(members, F["starts"][k]), G.voffset(members, F["starts"][k] + 9)
    assert F["bai"].count(struct.pack("<Q", old)) >= 1
    return F["bai"].replace(struct.pack("<Q", old), struct.pack("<Q", new)), [(0, 30 * 16384, 31 * 16384)]


def beyond_bai():
    """... with the END of w30's chunk behind the file (a start there would make the chunk an empty one, which is dropped)"""
    F = G.layout("per_record")
    k = F["names"].index("w30")
    members = G.member_table(F["data"])
    old = G.voffset(members, F["starts"][k + 1])
    return F["bai"].replace(struct.pack("<Q", old), struct.pack("<Q", (len(F["data"]) + 5) << 16)), [(0, 30 * 16384, 31 * 16384)]


def test_refusals(engine, files, tmp_path):
    good = BY_NAME["w16_left"]
    bam = tmp_path / "x.bam"
    bam.write_bytes(G.layout("per_record")["data"])
    region = [(0, 30 * 16384, 31 * 16384)]

    def refused(code, text, regions=region, bai=None, **kw):
        if bai is not None:
            open(str(bam) + ".bai", "wb").write(bai)
        engine.release_scratch()
        free0 = engine.mem_info()[0]
        with pytest.raises(TelrError) as e:
            engine.load_bam(str(bam), regions=regions, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)
        engine.release_scratch()                                  # nothing is left allocated beyond the context's scratch
        assert engine.mem_info()[0] == free0, (text, free0, engine.mem_info()[0])
        bi = load(engine, files, good)                            # the engine is as good as before
        loaded_equals(engine, bi, definition(good))
        bi.free()
    refused(R.E_IO, "cannot open the index")                     # no .bai next to the file
    refused(R.E_ARG, "references", bai=G.write_bai(R.bgzf(R.bam_header(["a", "b"], [10, 10]))))          # another file's
    full = G.layout("per_record")["bai"]
    refused(R.E_ARG, "past the index's end", bai=full[:len(full) // 2])
    refused(R.E_ARG, "no BAI magic", bai=b"BAJ\1" + full[4:])
    b, reg = moved_chunk_bai()
    refused(R.E_ARG, "the index does not match the file at virtual offset", regions=reg, bai=b)
    refused(R.E_ARG, "the index does not match the file at virtual offset", regions=reg, bai=b, chunk_bytes=1)
    b, reg = beyond_bai()
    refused(R.E_ARG, "at or beyond the BAM's size", regions=reg, bai=b)
    open(str(bam) + ".bai", "wb").write(full)
    for bad in ([(3, 0, 1)], [(-1, 0, 1)], [(0, -1, 1)], [(0, 5, 5)], [(0, G.TLENS[0], G.TLENS[0] + 5)], [(0, 0, 1, 7)]):
        refused(R.E_ARG, "region 0", regions=bad)
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(bam), regions=region, chunk_bytes=-2)
    assert e.value.code == R.E_ARG
    bi = engine.load_bam(str(bam), regions=region)               # and with the right index the file loads
    assert bi.region_info["selected"] == 1
    bi.free()


def test_a_fault_in_a_walked_record_is_named_by_its_virtual_offset(engine, tmp_path):
    """a record the bins over-select but no region overlaps is still checked: an op code above 8 in w40, asked for ins_only, which shares
    its 16-kb bin.  Stored members (level 0), so that the good file's index fits the bad file byte for byte"""
    F = G.layout("big")
    k = F["names"].index("w40")
    raw = bytearray(F["raw"])
    at = F["starts"][k] + 36 + raw[F["starts"][k] + 12]
    assert raw[at] & 15 == 0
    raw[at] |= 9
    data = R.bgzf(bytes(raw), level=0)
    p = tmp_path / "op9.bam"
    p.write_bytes(data)
    open(str(p) + ".bai", "wb").write(G.write_bai(R.bgzf(F["raw"], level=0)))
    want = G.voffset(G.member_table(data), F["starts"][k])
    t, pos, _ = G._pos("ins_only")
    with pytest.raises(TelrError) as e:
        engine.load_bam(str(p), regions=[(t, pos, pos + 1)])
    assert e.value.code == R.E_ARG and "record at virtual offset %d: CIGAR op code above 8" % want in str(e.value), str(e.value)


IN_W30, IN_W100 = [(0, 30 * 16384, 31 * 16384)], [(0, 100 * 16384, 101 * 16384)]
BOTH_CHUNKINGS = (1, 1 << 40)          # every member a chunk; one chunk


def region_members(F, regions):
    """the members that a load of `regions` inflates for its intervals: their numbers in the file"""
    merged = G.merge_regions(regions, G.TLENS)
    return [m for a, b in G.interval_members(F["data"], G.plan(F["bai"], len(G.TLENS), merged)) for m in range(a, b)]


@pytest.fixture(scope="module")
def crc_damaged(tmp_path_factory):
    """the `per_record` file with one bit flipped in the CRC-32 field of the first member of w30's interval: the file's length, every
    member's frame and the index stay valid.  -> (path, the member's number in the file, its file offset)"""
    F = G.layout("per_record")
    k = region_members(F, IN_W30)[0]
    off, n, _, _ = R.hop(F["data"])[k]
    data = bytearray(F["data"])
    data[off + n] ^= 0x10
    assert G.member_table(bytes(data)) == G.member_table(F["data"]) and k >= G.header_members(F["data"], F["raw"])
    p = tmp_path_factory.mktemp("bam_regions_crc") / "crc.bam"
    p.write_bytes(bytes(data))
    open(str(p) + ".bai", "wb").write(F["bai"])
    return str(p), k, G.member_table(F["data"])[k][0]


@pytest.mark.parametrize("chunk_bytes", BOTH_CHUNKINGS)
def test_a_failed_member_of_a_region_load_is_named_by_its_file_offset(engine, files, crc_damaged, chunk_bytes):
    path, k, coff = crc_damaged
    good = BY_NAME["w16_left"]
    engine.release_scratch()
    free0 = engine.mem_info()[0]
    with pytest.raises(TelrError) as e:
        engine.load_bam(path, regions=IN_W30, chunk_bytes=chunk_bytes)
    assert e.value.code == R.E_ARG and "block at file offset %d: CRC-32 mismatch" % coff in str(e.value), str(e.value)
    engine.release_scratch()                                      # nothing is left allocated beyond the context's scratch
    assert engine.mem_info()[0] == free0, (free0, engine.mem_info()[0])
    bi = load(engine, files, good)                                # the engine is as good as before
    loaded_equals(engine, bi, definition(good))
    bi.free()


@pytest.mark.parametrize("chunk_bytes", BOTH_CHUNKINGS)
def test_a_damaged_member_that_no_interval_names_is_never_inflated(engine, crc_damaged, chunk_bytes):
    """the same file, a region elsewhere: the load is the definition's of the undamaged file"""
    path, k, _ = crc_damaged
    F = G.layout("per_record")
    assert k not in range(G.header_members(F["data"], F["raw"])) and k not in region_members(F, IN_W100)
    L = G.load(F["data"], F["bai"], IN_W100)
    assert L.region_info["selected"] == 1
    bi = engine.load_bam(path, regions=IN_W100, chunk_bytes=chunk_bytes)
    loaded_equals(engine, bi, L)
    info = bi.region_info
    bi.free()
    assert info == L.region_info


@pytest.mark.parametrize("chunk_bytes", BOTH_CHUNKINGS)
def test_the_whole_file_load_names_the_same_member_by_its_number(engine, crc_damaged, chunk_bytes):
    """both namings come out of the one wait"""
    path, k, _ = crc_damaged
    with pytest.raises(TelrError) as e:
        engine.load_bam(path, chunk_bytes=chunk_bytes)
    assert e.value.code == R.E_ARG and "block %d: CRC-32 mismatch" % k in str(e.value), str(e.value)


# ---- 3. the other two loads ----------------------------------------------------------------------------------------------------------
def test_whole_file_and_chunked_loads_are_untouched(engine, files):
    def both():
        out = []
        for kw in (dict(), dict(chunk_bytes=1), dict(chunk_bytes=30000)):
            bi = engine.load_bam(files["unmapped"], keep_qual=True, **kw)
            out.append(snapshot(engine, bi) + [bi.region_info])
            bi.free()
        return out
    before = both()
    bi = load(engine, files, BY_NAME["every_member_a_chunk"])
    bi.free()
    assert both() == before
    assert before[0] == before[1] == before[2] and before[0][-1] == dict.fromkeys(G.REGION_INFO, 0)
    loaded = R.load(G.layout("unmapped")["data"], True)
    bi = engine.load_bam(files["unmapped"], keep_qual=True)
    loaded_equals(engine, bi, loaded)
    bi.free()


# ---- 4. the command ------------------------------------------------------------------------------------------------------------------
MM2 = ("--aligner", "minimap2", "-x", "pacbio", "--polish", "poa")
SITES = [(0, 20000, 0), (0, 33022, 4562), (0, 33100, 0), (0, 37990, 0)]          # the four sites of DESIGN.md 5.19


def argv_for(data_dir, reads, out, *extra):
    return ["-i", reads, "-r", data_dir + "/ref_38kb.fasta", "-l", data_dir + "/library.fasta", "-o", str(out)] + list(extra)


@pytest.fixture(scope="module")
def reads_run(engine, data_dir, tmp_path_factory):
    """the reads route with -k, as tests/test_gpu_telr_cli.py runs it: it keeps the sorted BAM and its .bai"""
    out = tmp_path_factory.mktemp("telr_regions")
    return telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", out, *MM2, "-k")), engine=engine)


def vcf_body(path):
    return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("#")]


def test_command_region_gives_the_known_row(engine, data_dir, tmp_path, reads_run):
    bam = reads_run["files"]["bam"]
    res = telr.run(telr.get_args(argv_for(data_dir, bam, tmp_path, *MM2, "--region", "chr2L:32,000-34,000")), engine=engine)
    print(res["counts"])
    assert len(res["final"]) == 1
    f = res["final"][0]
    assert (f["type"], f["chrom"], f["family"], f["strand"]) == ("non-reference", "chr2L", "jockey", "-")
    assert 33006 <= f["start"] <= f["end"] <= 33029
    assert 13 / 18 - 0.1 <= f["allele_frequency"] <= 13 / 16 + 0.1
    body = vcf_body(res["files"]["vcf"])
    assert len(body) == 1 and body[0][0] == "chr2L" and int(body[0][1]) == f["start"] + 1 and body[0][-2] == "GT:DR:DV"
    assert "FAMILY=jockey" in body[0][7] and "STRANDS=-" in body[0][7]
    c = res["counts"]
    assert c["regions"] == 1 and c["intervals"] >= 1 and 0 < c["selected"] <= c["walked"] and c["records"] <= c["selected"] and c["calls"] == 1
    # two options, three texts, given out of order: the same regions
    again = telr.run(telr.get_args(argv_for(data_dir, bam, tmp_path / "b", *MM2, "--region", "chr2L:33,500-34,000,chr2L:32000-32999", "--region", "chr2L:33000-33499")),
                     engine=engine)
    assert vcf_body(again["files"]["vcf"]) == body and again["counts"]["regions"] == 1


def test_command_region_sites(engine, data_dir, tmp_path, reads_run):
    bam = reads_run["files"]["bam"]
    tsv = tmp_path / "sites.tsv"
    tsv.write_text("".join("chr2L\t%d\t%d\n" % (p, l) for _, p, l in SITES))
    plain = telr.run(telr.get_args(argv_for(data_dir, bam, tmp_path / "plain", *MM2, "--sites", str(tsv))), engine=engine)
    reg = telr.run(telr.get_args(argv_for(data_dir, bam, tmp_path / "reg", *MM2, "--sites", str(tsv), "--region", "sites")), engine=engine)
    print(reg["counts"], plain["counts"])
    assert open(reg["files"]["sites_tsv"]).read() == open(plain["files"]["sites_tsv"]).read()
    assert reg["counts"]["regions"] == 3 and "regions" not in plain["counts"]          # 33,022 and 33,100 lie within two margins: one region
    assert telr.site_region_margin(telr.get_args(argv_for(data_dir, bam, tmp_path / "m", "--sites", str(tsv), "--site_reach", "7"))) == 7 + 200 + 1
    with pytest.raises(SystemExit):
        telr.get_args(argv_for(data_dir, bam, tmp_path / "x", "--region", "sites"))


def test_command_region_on_the_reads_route_changes_nothing(engine, data_dir, tmp_path, reads_run, capsys):
    res = telr.run(telr.get_args(argv_for(data_dir, data_dir + "/reads.fasta", tmp_path, *MM2, "-k", "--region", "chr2L:1-100")), engine=engine)
    assert capsys.readouterr().err.count(telr.REGION_INERT) == 1
    assert vcf_body(res["files"]["vcf"]) == vcf_body(reads_run["files"]["vcf"]) and res["counts"] == reads_run["counts"]
    for k in ("bed", "json", "bam"):
        assert open(res["files"][k], "rb").read() == open(reads_run["files"][k], "rb").read()


def test_command_without_an_index_ends_with_status_1(engine, data_dir, tmp_path, reads_run, capsys, monkeypatch):
    bam = tmp_path / "alone.bam"
    shutil.copy(reads_run["files"]["bam"], bam)
    monkeypatch.setattr(telr, "make_engine", lambda device: engine)
    monkeypatch.setattr(engine, "close", lambda: None, raising=False)
    assert telr.main(argv_for(data_dir, str(bam), tmp_path / "o", *MM2, "--region", "chr2L")) == 1
    err = capsys.readouterr().err
    assert "cannot open the index" in err and str(bam) + ".bai" in err
    assert not os.path.exists(str(tmp_path / "o" / "alone.telr.vcf"))
    with pytest.raises(ValueError, match="'chr9:1-5'"):
        telr.run(telr.get_args(argv_for(data_dir, reads_run["files"]["bam"], tmp_path / "p", *MM2, "--region", "chr9:1-5")), engine=engine)


def test_the_engines_bai_and_the_references_agree(reads_run):
    """the .bai that the device writer put next to the kept BAM against the reference's writer on the same bytes: the same bins, the same
    linear index, and chunks that differ only where a writer may merge (bam_reference.compare_bai's rule)"""
    data = open(reads_run["files"]["bam"], "rb").read()
    theirs = open(reads_run["files"]["bam"] + ".bai", "rb").read()
    raw, _, _ = R.inflate_file(data)
    _, tlens, recs = R.parse_stream(raw)
    head, offs, end = G.record_offsets(raw)
    rows = []
    for r, o, e in zip(recs, offs, offs[1:] + [end]):
        span = G.ref_span(r) or 1
        rows.append(dict(tid=r["refid"], pos=r["pos"], end=r["pos"] + span, off=o, size=e - o, bin=BR.reg2bin(r["pos"], r["pos"] + span) if r["refid"] >= 0 else 4680))
    ref_index = BR.bai_reference(BR.Stream(raw, head, offs, rows), tlens)
    blocks = G.member_table(data)
    BR.compare_bai(theirs, blocks, ref_index)
    BR.compare_bai(G.write_bai(data), blocks, ref_index)
    a, b = BR.parse_bai(theirs), BR.parse_bai(G.write_bai(data))
    assert [sorted(X["bins"]) for X in a["refs"]] == [sorted(X["bins"]) for X in b["refs"]]
    assert [X["linear"] for X in a["refs"]] == [X["linear"] for X in b["refs"]]
    for region in ([(0, 32000, 34000)], [(0, 0, 38000)], [(0, 20000, 20001)]):          # and the same records are reached through either
        wa, wb = (G.walked(data, raw, G.plan(x, len(tlens), region)) for x in (theirs, G.write_bai(data)))
        keep = [k for k, r in enumerate(recs) if G.is_selected(r, region)]
        assert set(keep) <= set(wa) and set(keep) <= set(wb)
