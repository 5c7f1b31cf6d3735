"""Stage-1 alignment, mirroring the reference's `src/telr/TELR_alignment.py`.

`alignment(bam, read, reference, out, sample_name, thread, method, presets)` keeps the reference's
signature and argument meaning (:9): `method` is "nglmr" (sic, the reference's spelling) or "minimap2",
`presets` is "ont" or "pacbio".  Instead of `ngmlr ... > tmp.sam` / `minimap2 --cs --MD -Y -L -ax ... >
sam` (:28-82) followed by `samtools sort` + `samtools index` (:103-114), the reads are mapped by the HIP
engine and the coordinate-sorted, indexed BAM is built on the device from what is resident there (reads,
reference, CIGARs: telr_write_bam_dev) -- the host parses the two input files (telr_fasta_load), packs and
uploads them, and moves the finished file image into `bam`, whose pages are being allocated while the reads
are still mapped (telr_bam_prepare).
"""
import atexit
import logging
import os
import sys
import threading
import time

from .aligner import Engine
from .fasta import read_fasta, load, load_reads
from .presets import preset
from ._abi import MF_KEEP_CIGARS


def format_time(seconds):          # TELR_utility.py:34-41
    h, rem = divmod(seconds, 3600)
    m, s = divmod(rem, 60)
    return "%d:%02d:%02d" % (int(h), int(m), round(s))


_release_threads = []


def wait_release():
    """join the background releases of earlier alignment() calls (before Engine.close(), or at exit)"""
    while _release_threads:
        _release_threads.pop().join()


atexit.register(wait_release)


def split_region_specs(text):
    """`SPEC[,SPEC...]` -> [SPEC]: a comma separates two specs unless it groups digits -- the piece behind it is three digits, alone or
    followed by `-` and digits, and the spec before it holds a colon (`chr2L:32,000-34,000` is one spec; a target whose whole name is
    three digits goes into an option of its own)"""
    import re
    out = []
    for piece in text.split(","):
        if out and ":" in out[-1] and re.fullmatch(r"\d{3}(-\d+)?", piece):
            out[-1] += "," + piece
        elif piece:
            out.append(piece)
    return out


def parse_regions(specs, tnames, tlens):
    """samtools-style region texts -> [(tid, beg, end)], 0-based and half-open.  `chr` is the whole target, `chr:beg-end` is 1-based and
    inclusive, `chr:beg` runs to the target's end; digit-group commas are allowed in the numbers.  A text that is a target's name as it
    stands, colon and all, is that target.  ValueError with the text of the spec: an unknown name, a bad number, beg below 1 or
    behind the target's end, end below beg.  An end behind the target's end is clipped to it."""
    names = [n.decode() if isinstance(n, bytes) else str(n) for n in tnames]
    tid_of = {}
    for i, n in enumerate(names):
        tid_of.setdefault(n, i)
    out = []
    for spec in specs:
        spec = str(spec)

        def bad(why):
            return ValueError("region %r: %s" % (spec, why))
        if spec in tid_of:
            tid = tid_of[spec]
            out.append((tid, 0, int(tlens[tid])))
            continue
        name, colon, span = spec.rpartition(":")
        if not colon or name not in tid_of:
            raise bad("no target of that name")
        tid = tid_of[name]
        tlen = int(tlens[tid])
        lo, dash, hi = span.partition("-")

        def number(t):
            t = t.replace(",", "")
            if not t.isdigit() or not t.isascii():
                raise bad("%r is no position" % t)
            return int(t)
        beg = number(lo)
        end = number(hi) if dash else tlen
        if beg < 1 or beg > tlen or end < beg:
            raise bad("positions %d to %d are no stretch of a target of %d bases" % (beg, end, tlen))
        out.append((tid, beg - 1, min(end, tlen)))
    return out


def bam_input(bam, out, sample_name, engine=None, index=None, keep_qual=False, chunk_bytes=None, regions=None, bai=None):
    """The `.bam` branch of parse_input (TELR_input.py:300-305, 329-361): the alignment is skipped and the reads come out of the BAM.
    The file is loaded on the device (Engine.load_bam); <out>/<sample_name>.telr.fasta is written as bam2fasta writes it (first
    record of a name wins) and the BamInput is returned: its read_set and result are what alignment() + a re-read of the BAM would
    have left on the device.  index: an Index whose targets the file's references must equal (names, lengths, order; ValueError).
    A coordinate-sorted file needs no sort_index_bam; another order is accepted as it is.  chunk_bytes: as Engine.load_bam takes it
    (None: the whole file at once; 0 or n: in chunks, a file of any size).  regions: a list of (tid, beg, end) (parse_regions): only
    what overlaps them is loaded, through the index `bai` (None: bam + ".bai"); None: the whole file."""
    eng = engine or (index.eng if index is not None else Engine(0))
    if regions is None:
        bi = eng.load_bam(bam, keep_qual=keep_qual, chunk_bytes=chunk_bytes)
    else:
        bi = eng.load_bam(bam, keep_qual=keep_qual, chunk_bytes=chunk_bytes, regions=regions, bai=bai)
    if index is not None:
        names = getattr(index, "tnames", None)
        if names is not None:
            bi.check_targets(names, index.targets.len)
        elif [int(x) for x in bi.tlens] != [int(x) for x in index.targets.len]:
            raise ValueError("the BAM's references are not the index's targets (lengths and order must agree)")
    bi.write_fasta(os.path.join(out, sample_name + ".telr.fasta"))
    logging.info("BAM input: %d reads, %d of %d mapped records kept" % (bi.counters["reads"], bi.counters["kept"], bi.counters["mapped"]))
    return bi


def alignment(bam, read, reference, out, sample_name, thread, method, presets, engine=None, chain_skip=False, seed_rescue=False, mm2_mapq=False,
              keep_qual=False):
    """keep_qual: carry the base qualities of a FASTQ `read` file into QUAL of the BAM, as ngmlr and `minimap2 -a` do (1 byte of
    device memory per read base, a level-1 BAM of about 1.55 times the size for ONT-shaped qualities: 0.81 -> 1.26 bytes per read base); a FASTA has none and gives the same file either way.  Default: QUAL 0xff.
    chain_skip (minimap2 branch only): minimap2's own chaining scan (presets.preset(..., chain_skip=True)), not the fixed look-back.
    seed_rescue, mm2_mapq (minimap2 branch only): minimap2's high-occurrence seed rescue and its own MAPQ (presets.preset)"""
    logging.info("Start alignment...")
    start_time = time.time()
    if presets not in ("ont", "pacbio"):
        print("Read presets not recognized, please provide ont or pacbio, exiting...")
        sys.exit(1)
    if method == "nglmr":
        name = "ngmlr-ont" if presets == "ont" else "ngmlr-pacbio"
        rg = (sample_name, sample_name, "ont" if presets == "ont" else "pb")     # --rg-id/--rg-sm/--rg-lb (:32-49)
        cmd = "ngmlr -r %s -q %s -x %s -t %s" % (reference, read, presets, thread)
    elif method == "minimap2":
        name = "map-ont" if presets == "ont" else "map-pb"
        rg = None
        cmd = "minimap2 --cs --MD -Y -L -ax %s%s%s %s %s" % (name, " --max-chain-skip 25" if chain_skip else "", " -e 500" if seed_rescue else "", reference, read)
    else:
        print("Alignment method not recognized, please provide ont or pacbio, exiting...")
        sys.exit(1)
    if chain_skip and method != "minimap2":
        raise ValueError("chain_skip is an option of the minimap2 branch")
    if (seed_rescue or mm2_mapq) and method != "minimap2":
        raise ValueError("seed_rescue and mm2_mapq are options of the minimap2 branch")
    eng = engine or Engine(0)
    io, mo = preset(name, chain_skip=chain_skip, seed_rescue=seed_rescue, mm2_mapq=mm2_mapq)
    tm = {}                                       # seconds per phase of the last call: alignment.last_timings
    t0 = time.time()
    tf = load(reference)                          # None for gzip: the Python reader
    ri = load_reads(read, eng, keep_qual) if str(read).endswith(".gz") else None          # gzip / BGZF reads: parsed and packed on the device (None: refused)
    qf = load(read) if ri is None else None
    if tf is not None:
        tn, ts = tf.names_c, tf.triple
    else:
        tn, ts = read_fasta(reference)
    qq = None
    if ri is not None:
        qn, qs, n_bases = ri.names_c, None, ri.n_bases
    elif qf is not None:
        qn, qs, n_bases = qf.names_c, qf.triple, int(qf.triple[2].sum())
        if keep_qual:
            qq = qf.qual
    else:
        qn, qs, qq = read_fasta(read, with_qual=True)
        n_bases = sum(len(x) for x in qs)
        if not keep_qual:
            qq = None
    with_cs = method == "minimap2"
    tm["parse_files"] = time.time() - t0; t0 = time.time()
    ix = eng.index(ts, io)
    tm["pack_reference_build_index"] = time.time() - t0; t0 = time.time()
    qset = ri.read_set if ri is not None else eng.seqset(qs, qual=qq)
    has_qual = qq is not None or (ri is not None and qset.has_qual)
    tm["pack_upload_reads"] = time.time() - t0; t0 = time.time()
    # about 0.85 bytes of BAM per read base with --cs --MD, 0.6 without cs, at level 1; qualities add their entropy (0.45 measured for ONT-shaped ones, at most 0.82: 6.55 bits)
    ix.bam_prepare(bam, int(((0.95 if with_cs else 0.7) + (0.85 if has_qual else 0)) * n_bases) + (64 << 20))
    mo.flags |= MF_KEEP_CIGARS                   # the CIGAR array stays on the device as well: the BAM writer reads it there
    r = None
    try:
        r = ix.map_raw(qset, mo)
        tm["map"] = time.time() - t0; t0 = time.time()
        ix.write_bam_device(r, qset, qn, tn, bam, md=True, cs=with_cs, softclip=True, rg=rg, cmdline=cmd, index=True, level=1)
        tm["sorted_bam"] = time.time() - t0; t0 = time.time()
    except BaseException:
        # nothing half-made at the output path: the pre-sized file of bam_prepare goes with its sink (the writer itself
        # unlinks what it could not finish), so that the existence test below -- the reference's -- means what it says
        ix.bam_discard()
        for leftover in (bam, bam + ".bai"):
            if os.path.exists(leftover):
                os.unlink(leftover)
        raise
    finally:
        if r is not None:
            ix.free_raw(r)
        # giving the rest back -- hipFree of the packed reads and of the index (0.12 s for a 30x set), the parsed files or their
        # mappings -- is not something the caller has to wait for with its BAM finished: sequence sets and indexes are plain device
        # memory without context state.  The thread is joined at interpreter exit and by wait_release() (a caller that closes
        # the engine right away).

        def _drop(files, reads, index):
            reads.free()
            index.free()
            for f in files:
                if f is not None:
                    f.close()
        th = threading.Thread(target=_drop, args=((tf, qf, ri), qset, ix), daemon=False)
        _release_threads.append(th)
        th.start()
    tm["release"] = time.time() - t0
    # (the engine keeps its grow-only mapping scratch, 150-200 GB for a 30x read set: a caller that goes on to the per-locus
    # stages with the same engine gives it back with Engine.release_scratch() -- 0.2 s -- when it knows stage 1 will not run again)
    alignment.last_timings = tm
    if os.path.isfile(bam) is False:
        sys.stderr.write("Sorted and indexed BAM file does not exist, exiting...\n")
        sys.exit(1)
    logging.info("First alignment finished in " + format_time(time.time() - start_time))
