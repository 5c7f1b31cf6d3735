"""The `telr` command: reads, or a BAM of mapped reads, to `<sample>.telr.vcf` in one run on the device.

    python -m telr_amd.telr -i reads.fasta -r reference.fasta -l library.fasta -o out

The arguments are those of the reference's `get_args` (src/telr/TELR_input.py:10-256) with its defaults and its messages, restated
here; the flow is that of its `main` (src/telr/telr.py:22-189) with this project's stages in the place of the tools it shells out to:

    reference, library         fasta.read_fasta
    stage-1 index              Engine.index with the aligner's preset (`--aligner nglmr`: ngmlr-ont / ngmlr-pacbio, `minimap2`: map-ont / map-pb)
    reads route                fasta.load -> Engine.seqset -> Index.map_raw (TELR_MF_CIGAR | TELR_MF_KEEP_CIGARS) -> the sorted BAM + .bai
                               with the device writer into <out>/intermediate_files/<sample>_sort.bam
    gzip / BGZF reads          a reads file ending `.gz`: fasta.load_reads -> Engine.load_reads: the container is decided
                               by content, the text is inflated (BGZF: on the device; gzip: one zlib thread), parsed and packed on the device
                               in chunks (`--reads_chunk_mb N`; 0, the default: the engine's own size) and never becomes host text.  A file
                               whose grammar the device parser refuses goes to fasta.read_fasta as before.  Same outputs either way.
    BAM route (`-i x.bam`)     Engine.load_bam, BamInput.check_targets against the reference.  `--bam_chunk_mb N`: in chunks of N MiB of
                               inflated bytes (a file of any size); 0 (the default): the whole file at once when it and
                               its inflated stream fit into half the free device memory, else in chunks of the engine's own size --
                               one hop of the member headers decides and is handed on.  The outputs do not depend on the choice.
    `--region SPEC[,SPEC...]`  on the BAM route, any number of times: only the records that overlap the regions are loaded, and
                               only the BGZF members that <bam>.bai names for them are uploaded and inflated (Engine.load_bam(regions=...)).
                               SPEC as samtools takes it -- `chr`, `chr:beg-end` (1-based, inclusive), `chr:beg` -- resolved against the
                               reference's names, which check_targets ties to the BAM's header.  Discovery, drafts and loci (or `--sites`)
                               then run on what was loaded.  `--region sites` with `--sites FILE`: one region [pos - m, pos + m) per listed
                               site, m = site_reach + the caller's max_ref_gap + 1 (site_region_margin).  As after `samtools view` of the
                               regions, a read whose primary record lies outside them is no read of the run and its records inside are
                               orphans; nothing repairs that.  A missing or unfit .bai ends the run with the engine's text and status 1:
                               nothing falls back to the whole file.  On the reads route the option is reported once as having no effect.
    calls                      telr_sv.call_insertions(..., reads=<the resident set>, genotype=True)      (not Sniffles)
    drafts                     telr_assembly.draft_loci(..., reads=<the resident set>)                     (not wtdbg2 / flye)
    `--bridge`                 insertions that no single read spans: the caller runs with min_sized = 0, so a cluster of
                               clips alone is a call; a call without a draft gets a bridge of two reads joined at one shared k-mer
                               (Index.bridge_contigs + SeqSet.join; not an assembler); its row's sv_length and ins_seq become the
                               bridge's ins_len and ALT.  Without the option nothing changes.
    `--sites FILE`             a mode of its own: genotype the insertion sites of FILE -- another sample's `telr.vcf`, a cohort's
                               merged list, a truth set; a VCF as this command writes it or a TSV chrom, pos0[, len[, id]] -- on THIS sample.
                               Reference, stage-1 index and the reads or BAM route as above, then telr_sv.genotype_sites (Index.call_at_sites
                               + Index.genotype_insertions; not Sniffles' forced genotyping), then <sample>.telr.sites.tsv with one line
                               per site, `0/0` and `./.` included, and for a VCF input <sample>.telr.sites.vcf.  `--site_reach N` (50): a
                               signature supports the nearest site within N bases; `--site_len_pct N` (0: off): a sized signature whose
                               length differs from the site's by more than N percent is dropped.  No discovery, draft, asm10 index or
                               loci stage runs; `--polish`, `--bridge` and `--ref_te` are reported once as having no effect.
    asm10 index                Engine.index over the same resident reference
    a reference above 2^31     `--index_part_bases N`: the reference is cut into parts of at most N bases of padded extent, each
                               with an index of its own (Engine.index_parts); the reads are mapped against every part and the records merged
                               on the device.  With 0 (the default) the run is what it was, and goes this way only when the reference does
                               not fit one index (about 2.1 Gbp).  The BAM route maps nothing and is unaffected.
    reference TE copies        `--ref_te engine`: telr_te.annotate_reference on the resident reference (not RepeatMasker),
                               kept as <out>/intermediate_files/<reference>.te.bed; `--ref_te FILE`: a BED6 of the caller's; default none
    loci                       locus_pipeline.run_loci(..., read_set, contig_set, polish, ref_te_rows, ...)
    outputs                    locus_pipeline.write_outputs(..., sv_info=telr_sv.sv_info(rows))

On neither route are the reads decoded to host text: the ALT sequences and the contigs are cut out of the resident packed set by
`SeqSet.extract`, and the host copy of a reads file is given back once the set is on the device.  `<sample>.telr.fasta`, which the
reference's bam2fasta leaves behind on the BAM route, is therefore not written; nothing in the run reads it.

Different from the reference on purpose: every value it prints a message for ends the run with status 1 (the reference goes on after
four of its messages: -p below 1, a negative --af_flank_offset or --af_te_offset, --af_te_interval below 1); a reads file of any
extension other than `.bam` is read as reads (a `.gz` on the device, see above; one it refuses, and every plain file, by the readers).  Not built: the ALT pre-screen, merge_rows on the
caller's rows, the RepeatMasker route for families, the N-rank path, gzip on the BAM route, a bridge of more than two reads (an
element longer than two reads' clips together stays without a contig); for `--sites`: no draft or liftover for the listed sites, no
N-rank path (several samples' VCFs are merged into the list by `python -m telr_amd.telr_cohort merge`).  On a multi-part reference: the occurrence
cut-off of the seeding is per part, as with minimap2 -I (secondaries the unsplit index would not report), all parts are resident together,
and `--ref_te engine` maps the tiles to the library, not to the reference, so it runs as it is.
"""
import argparse
import os
import shutil
import sys
import time

INERT = "--assembler, --polisher, --different_contig_name and --minimap2_family have no effect here: this project has one drafting " \
        "step (a supporting read's piece, polished on the device) and annotates families by alignment only"


REGION_INERT = "--region has no effect on the reads route: it selects the records of a BAM of mapped reads through its .bai; reads are mapped as a whole"


SITES_INERT = ("--polish", "--bridge", "--ref_te")          # options of the stages that a --sites run does not have


def _say(msg):
    sys.stderr.write(msg + "\n")


def _exit(msg):
    print(msg)
    sys.exit(1)


def get_args(argv=None):
    """-> argparse.Namespace with every default filled in; an unreadable input or an invalid value prints the reference's message and
    exits with status 1"""
    p = argparse.ArgumentParser(prog="telr", description="Program for detecting non-reference TEs in long read data")
    opt = p._action_groups.pop()
    req = p.add_argument_group("required arguments")
    req.add_argument("-i", "--reads", type=str, required=True, help="reads in fasta/fastq format or read alignments in bam format")
    req.add_argument("-r", "--reference", type=str, required=True, help="reference genome in fasta format")
    req.add_argument("-l", "--library", type=str, required=True, help="TE consensus sequences in fasta format")
    opt.add_argument("--aligner", type=str, help="method for read alignment, 'nglmr' or 'minimap2' (default = 'nglmr')")
    opt.add_argument("--assembler", type=str, help="'wtdbg2' or 'flye' (default = 'wtdbg2'); parsed, no effect here")
    opt.add_argument("--polisher", type=str, help="'wtdbg2' or 'flye' (default = 'wtdbg2'); parsed, no effect here")
    opt.add_argument("-x", "--presets", type=str, help="parameter presets for the sequencing technology, 'pacbio' or 'ont' (default = 'pacbio')")
    opt.add_argument("-p", "--polish_iterations", type=int, help="iterations of contig polishing (default = 1)")
    opt.add_argument("-o", "--out", type=str, help="directory to output data (default = '.')")
    opt.add_argument("-t", "--thread", type=int, help="max cpu threads to use (default = '1')")
    opt.add_argument("-g", "--gap", type=int, help="max gap size for flanking sequence alignment (default = '20')")
    opt.add_argument("-v", "--overlap", type=int, help="max overlap size for flanking sequence alignment (default = '20')")
    opt.add_argument("--flank_len", type=int, help="flanking sequence length (default = '500')")
    opt.add_argument("--af_flank_interval", type=int, help="5' and 3' flanking sequence interval size used for allele frequency estimation (default = '100')")
    opt.add_argument("--af_flank_offset", type=int, help="5' and 3' flanking sequence offset size used for allele frequency estimation (default = '200')")
    opt.add_argument("--af_te_interval", type=int, help="5' and 3' te sequence interval size used for allele frequency estimation (default: '50')")
    opt.add_argument("--af_te_offset", type=int, help="5' and 3' te sequence offset size used for allele frequency estimation (default: '50')")
    opt.add_argument("--different_contig_name", action="store_true", help="parsed, no effect here")
    opt.add_argument("--minimap2_family", action="store_true", help="parsed, no effect here (families are annotated by alignment)")
    opt.add_argument("-k", "--keep_files", action="store_true", help="keep the intermediate files (default: remove them)")
    own = p.add_argument_group("options of this project")
    own.add_argument("--polish", type=str, help="polishing of the drafts on the device: 'none', 'pileup' or 'poa' (default = 'poa')")
    own.add_argument("--device", type=int, default=0, help="the GPU to run on (default = 0)")
    own.add_argument("--keep_qual", action="store_true", help="carry the base qualities of a FASTQ or a BAM into the read set and the BAM")
    own.add_argument("--chain_skip", action="store_true", help="minimap2's own chaining scan (minimap2 aligner only)")
    own.add_argument("--seed_rescue", action="store_true", help="minimap2's high-occurrence seed rescue (minimap2 aligner only)")
    own.add_argument("--mm2_mapq", action="store_true", help="minimap2's own MAPQ (minimap2 aligner only)")
    own.add_argument("--ref_te", type=str, default="none", help="the reference's own TE copies for the liftover: 'none', 'engine' (annotated on the device; not "
                     "RepeatMasker) or a BED6 file with the columns RepeatMasker's GFF gives (default = 'none')")
    own.add_argument("--index_part_bases", type=int, default=0, help="cut the reference into index parts of at most N bases (padded extent) and merge the "
                     "per-part records on the device; 0: one index, parts only when the reference does not fit one (default = 0)")
    own.add_argument("--bam_chunk_mb", type=int, default=0, help="load a BAM of reads in chunks of at most N MiB of inflated bytes; 0: the whole file at once "
                     "when it fits into half the free device memory next to its inflated stream, else chunks of the engine's own size (default = 0)")
    own.add_argument("--reads_chunk_mb", type=int, default=0, help="parse a gzip or BGZF reads file on the device in chunks of at most N MiB of text; "
                     "0: chunks of the engine's own size (default = 0)")
    own.add_argument("--bridge", action="store_true", help="also call insertions that no single read spans (clusters of clipped reads alone) and draft them "
                     "as a bridge of two reads joined at one shared k-mer (not an assembler)")
    own.add_argument("--sites", type=str, help="genotype the insertion sites of FILE on this sample instead of discovering calls: a VCF as this command writes it, "
                     "or a TSV with the columns chrom, pos0[, len[, id]]; writes <sample>.telr.sites.tsv (and .sites.vcf for a VCF) with one line per site, "
                     "0/0 and ./. included (not Sniffles' forced genotyping)")
    own.add_argument("--site_reach", type=int, default=50, help="with --sites: a signature supports the nearest site within N bases (default = 50)")
    own.add_argument("--site_len_pct", type=int, default=0, help="with --sites: drop a sized signature whose length differs from the site's by more than N percent; "
                     "0: no length test (default = 0)")
    own.add_argument("--region", action="append", metavar="SPEC[,SPEC...]", help="on the BAM route: load only the records that overlap these regions, through "
                     "<bam>.bai (samtools-style: chr, chr:beg-end 1-based and inclusive, chr:beg to the target's end); may be given more than once.  'sites' "
                     "together with --sites: one region around every listed site.  A read whose primary record lies outside the regions is not loaded")
    own.add_argument("--sample", type=str, help="sample name (default: the reads file's name without its extension)")
    p._action_groups.append(opt)
    a = p.parse_args(argv)

    for path in (a.reads, a.reference, a.library) + (() if a.ref_te in ("none", "engine") else (a.ref_te,)) + (() if a.sites is None else (a.sites,)):
        try:
            open(path, "r").close()
        except Exception as e:
            print(e)
            _say("Can not open input file: " + path)
            sys.exit(1)
    if a.ref_te not in ("none", "engine"):
        from . import telr_te
        try:
            telr_te.read_te_bed(a.ref_te)
        except (OSError, ValueError) as e:
            print(e)
            _exit("Please provide a valid BED6 file of the reference's TE copies (--ref_te), exiting...")

    def choice(name, default, allowed, what):
        v = getattr(a, name)
        if v is None:
            setattr(a, name, default)
        elif v not in allowed:
            _exit("Please provide a valid %s (%s), exiting..." % (what, "/".join(allowed)))
    choice("aligner", "nglmr", ("nglmr", "minimap2"), "alignment method")
    choice("assembler", "wtdbg2", ("wtdbg2", "flye"), "assembly method")
    choice("polisher", "wtdbg2", ("wtdbg2", "flye"), "polish method")
    choice("presets", "pacbio", ("pacbio", "ont"), "preset option")
    choice("polish", "poa", ("none", "pileup", "poa"), "polishing step")

    def number(name, default, ok, msg):
        v = getattr(a, name)
        if v is None:
            setattr(a, name, default)
        elif not ok(v):
            _exit(msg)
    number("polish_iterations", 1, lambda v: v >= 1, "Please provide a valid number of iterations for polishing, exiting...")
    number("thread", 1, lambda v: True, "")
    number("flank_len", 500, lambda v: True, "")
    number("af_flank_interval", 100, lambda v: v > 0,
           "Please provide a valid flanking sequence interval size (positive integer) for allele frequency estimation, exiting...")
    number("af_flank_offset", 200, lambda v: v >= 0,
           "Please provide a valid flanking sequence offset size (positive integer) for allele frequency estimation, exiting...")
    number("af_te_interval", 50, lambda v: v > 0, "Please provide a valid TE interval size (positive integer) for allele frequency estimation, exiting...")
    number("af_te_offset", 50, lambda v: v >= 0, "Please provide a valid TE offset size (positive integer) for allele frequency estimation, exiting...")
    number("gap", 20, lambda v: True, "")
    number("overlap", 20, lambda v: True, "")
    if a.device < 0:
        _exit("Please provide a valid device number, exiting...")
    if a.index_part_bases < 0:
        _exit("Please provide a valid number of bases per index part (0 or a positive integer), exiting...")
    if a.bam_chunk_mb < 0:
        _exit("Please provide a valid BAM chunk size in MiB (0 or a positive integer), exiting...")
    if a.reads_chunk_mb < 0:
        _exit("Please provide a valid reads chunk size in MiB (0 or a positive integer), exiting...")
    if a.site_reach < 0:
        _exit("Please provide a valid site reach (0 or a positive integer), exiting...")
    if not 0 <= a.site_len_pct <= 100:
        _exit("Please provide a valid site length tolerance in percent (0 to 100), exiting...")
    if a.region and a.sites is None and any(s == "sites" for text in a.region for s in text.split(",")):
        _exit("--region sites needs the site list of --sites, exiting...")
    if (a.chain_skip or a.seed_rescue or a.mm2_mapq) and a.aligner != "minimap2":
        _exit("--chain_skip, --seed_rescue and --mm2_mapq are options of the minimap2 aligner, exiting...")
    a.out = os.path.abspath("." if a.out is None else a.out)
    os.makedirs(a.out, exist_ok=True)
    if a.sample is None:
        a.sample = os.path.splitext(os.path.basename(a.reads))[0]
    given = lambda names: [o for o in names if any(x == o or x.startswith(o + "=") for x in (sys.argv[1:] if argv is None else argv))]
    a.inert_given = given(("--assembler", "--polisher", "--different_contig_name", "--minimap2_family"))
    a.sites_inert_given = given(SITES_INERT) if a.sites is not None else []
    return a


def is_bam(path):
    """the branch of parse_input (TELR_input.py:299-305): by extension"""
    return os.path.splitext(path)[1] == ".bam"


def aligner_preset(args):
    """-> (preset name, read group or None, the command line the BAM's @PG names)"""
    if args.aligner == "nglmr":
        return ("ngmlr-ont" if args.presets == "ont" else "ngmlr-pacbio", (args.sample, args.sample, "ont" if args.presets == "ont" else "pb"),
                "ngmlr -r %s -q %s -x %s -t %s" % (args.reference, args.reads, args.presets, args.thread))
    name = "map-ont" if args.presets == "ont" else "map-pb"
    return name, None, "minimap2 --cs --MD -Y -L -ax %s%s%s %s %s" % (name, " --max-chain-skip 25" if args.chain_skip else "",
                                                                       " -e 500" if args.seed_rescue else "", args.reference, args.reads)


# ---- the stages: module-level so that a caller (or a test) can put its own in their place ------------------------------------------
def make_engine(device):
    from .aligner import Engine
    return Engine(device)


def index_stage(eng, targets, io, part_bases, like=None):
    """the index of a stage over the reference -> (index, number of parts).  part_bases 0: Engine.index as ever, unless the planner says
    that the reference needs more than one part; part_bases > 0: always Engine.index_parts.  like: the stage-1 index, whose resident
    targets (and parts) the asm10 index is built over"""
    from .aligner import Engine, PartIndex
    if like is not None:
        if isinstance(like, PartIndex):
            ix = eng.index_parts(None, io, max_part_bases=like.max_part_bases, like=like)
            return ix, ix.n_parts
        return eng.index(like.targets, io), 1
    if part_bases == 0:
        part_of = Engine.part_plan([len(s) for s in targets])
        if len(part_of) == 0 or int(part_of[-1]) == 0:
            return eng.index(targets, io), 1
    ix = eng.index_parts(targets, io, max_part_bases=part_bases)
    return ix, ix.n_parts


def load_reads(eng, ix, args, tnames, bam_path):
    """the reads route: reader -> resident set -> telr_map -> sorted BAM + .bai -> (read names, read set, raw result, free function)"""
    from . import fasta
    from ._abi import MF_CIGAR, MF_KEEP_CIGARS
    from .presets import preset
    name, rg, cmd = aligner_preset(args)
    _, mo = preset(name, chain_skip=args.chain_skip, seed_rescue=args.seed_rescue, mm2_mapq=args.mm2_mapq)
    mo.flags |= MF_CIGAR | MF_KEEP_CIGARS
    ri = fasta.load_reads(args.reads, eng, args.keep_qual, getattr(args, "reads_chunk_mb", 0) << 20) if str(args.reads).endswith(".gz") else None
    qf = fasta.load(args.reads) if ri is None else None
    if ri is not None:                              # gzip or BGZF: parsed and packed on the device, never host text
        qnames, qset = ri.qnames, ri.read_set
        ri.free()
    elif qf is not None:
        qnames = list(qf.names)
        qset = eng.seqset(qf.triple, qual=qf.qual if args.keep_qual else None)
        qf.close()                                  # the host copy is not needed again: every later piece comes from the set
    else:
        qnames, qs, qq = fasta.read_fasta(args.reads, with_qual=True)
        qset = eng.seqset(qs, qual=qq if args.keep_qual else None)
        del qs, qq
    r = ix.map_raw(qset, mo)
    try:
        ix.write_bam_device(r, qset, qnames, tnames, bam_path, md=True, cs=args.aligner == "minimap2", softclip=True, rg=rg, cmdline=cmd, index=True, level=1)
    except BaseException:
        ix.free_raw(r)
        raise
    return qnames, qset, r, lambda: (ix.free_raw(r), qset.free())


def load_bam(eng, ix, args, tnames, tlens):
    """the BAM route: the file inflated and parsed on the device, its references checked against the reference's -> the same four"""
    from .aligner import BAM_CHUNK_FIT
    bi = eng.load_bam(args.reads, keep_qual=args.keep_qual, chunk_bytes=args.bam_chunk_mb << 20 if args.bam_chunk_mb > 0 else BAM_CHUNK_FIT)
    try:
        bi.check_targets(tnames, tlens)
    except BaseException:
        bi.free()
        raise
    return bi.qnames, bi.read_set, bi.result, lambda: (bi.free(), bi.read_set.free())


def site_region_margin(args):
    """`--region sites`: the margin m of the region [pos - m, pos + m) around a listed site (DESIGN.md 5.20 derives it): a signature is
    kept at a site within site_reach of it and lies inside its record's span, ends included; the mate of a split signature starts
    within the caller's max_ref_gap of that; a record that the genotyper counts spans the site itself.  So m = site_reach + max_ref_gap
    + 1 is the smallest m for which every such record overlaps the region"""
    from ._abi import InsOpt
    return args.site_reach + InsOpt.default().max_ref_gap + 1


def bam_regions(args, tnames, tlens, listed):
    """the `--region` texts -> [(tid, beg, end)]; `sites`: one region per listed site"""
    from .telr_alignment import parse_regions, split_region_specs
    specs = [s for text in args.region for s in split_region_specs(text)]
    out = parse_regions([s for s in specs if s != "sites"], tnames, tlens)
    if "sites" in specs:
        m = site_region_margin(args)
        out += [(tid, max(0, pos - m), min(pos + m, int(tlens[tid]))) for tid, pos, _ in listed["sites"]]
    return out


def load_bam_regions(eng, ix, args, tnames, tlens, regions):
    """the BAM route with `--region`: only what overlaps the regions is loaded, through the file's .bai -> the four of load_bam and
    BamInput.region_info"""
    from .aligner import BAM_CHUNK_FIT
    bi = eng.load_bam(args.reads, keep_qual=args.keep_qual, chunk_bytes=args.bam_chunk_mb << 20 if args.bam_chunk_mb > 0 else BAM_CHUNK_FIT, regions=regions)
    try:
        bi.check_targets(tnames, tlens)
    except BaseException:
        bi.free()
        raise
    return bi.qnames, bi.read_set, bi.result, lambda: (bi.free(), bi.read_set.free()), bi.region_info


def call_stage(ix, r, tnames, qnames, read_set, sample, bridge=False):
    """bridge: the caller's min_sized = 0 -- a cluster of clips alone is a call (rep = -1, len = 0, ins_seq "N")"""
    from . import telr_sv
    from ._abi import InsOpt
    opt = InsOpt.default(min_sized=0) if bridge else None
    rows = telr_sv.call_insertions(ix, r, tnames, qnames, read_set, opt=opt, sample=sample, genotype=True)
    return rows, ix.call_insertions(r, opt)


def sites_stage(ix, r, tnames, qnames, listed, args):
    """--sites: the listed sites genotyped on this sample's result -> the dicts of telr_sv.genotype_sites, one per site"""
    from . import telr_sv
    from ._abi import SiteOpt
    return telr_sv.genotype_sites(ix, r, tnames, qnames, listed["sites"], site_opt=SiteOpt.default(reach=args.site_reach, len_pct=args.site_len_pct))


def draft_stage(ix, r, ic, rows, read_set, chrom_ids, bridge=False):
    from . import telr_assembly
    if not bridge:
        return telr_assembly.draft_loci(ix, r, ic, rows, read_set, read_set, chrom_ids)
    return telr_assembly.draft_loci(ix, r, ic, rows, read_set, read_set, chrom_ids, bridge=True)


def ref_te_stage(eng, ix, tnames, lib_names, lib_seqs, args, bed_path):
    """--ref_te: the reference's TE copies as BED6 rows for the liftover -- annotated on the device and written to bed_path ('engine'), or read
    from the caller's file"""
    from . import telr_te
    if args.ref_te == "engine":
        rows = telr_te.annotate_reference(eng, ix.targets, tnames, lib_names, lib_seqs)
        telr_te.write_te_bed(rows, bed_path)
        return rows
    return telr_te.read_te_bed(args.ref_te)


def loci_stage(eng, ix10, tnames, ref_seq, loci, lib_names, lib_seqs, read_set, cset, args, ref_te_rows=None):
    from . import locus_pipeline
    return locus_pipeline.run_loci(eng, ix10, tnames, ref_seq, loci, lib_names, lib_seqs, presets=args.presets, read_set=read_set, contig_set=cset,
                                   ref_te_rows=ref_te_rows,
                                   polish=None if args.polish == "none" else args.polish, polish_iterations=args.polish_iterations,
                                   flank_len=args.flank_len, gap=args.gap, overlap=args.overlap,
                                   af_params=(args.af_flank_interval, args.af_flank_offset, args.af_te_interval, args.af_te_offset))


EMPTY_RESULT = {"annotation": [], "liftover": [], "summary": {}, "af": {}}


def run(args, engine=None):
    """One run of the pipeline with the Namespace of `get_args` -> dict(final = the rows of `<sample>.telr.json`, files = {name: path},
    counts = {reads, records, calls, calls_without_draft, loci_annotated, loci_lifted, loci_written; with --bridge also calls_bridged; with
    --region on the BAM route also the six of BamInput.region_info: regions, intervals, members, header_members, walked, selected},
    seconds = {stage: wall time}).  With args.sites: final = [], sites = the dicts of telr_sv.genotype_sites, files gains sites_tsv (and
    sites_vcf), counts gains sites and sites_supported, and the stages are inputs, index, reads, sites, outputs.
    engine: an aligner.Engine to run on (default: a new one on args.device, closed at the end).  Engine errors are raised as TelrError;
    nothing falls back to another path."""
    from . import fasta, locus_pipeline, telr_sv
    from .presets import preset
    counts = dict(reads=0, records=0, calls=0, calls_without_draft=0, loci_annotated=0, loci_lifted=0, loci_written=0)
    seconds = {}
    sample = args.sample
    inter = os.path.join(args.out, "intermediate_files")
    os.makedirs(inter, exist_ok=True)
    files = {k: os.path.join(args.out, sample + ".telr." + k) for k in ("vcf", "bed", "json", "expanded.json", "te.fasta", "contig.fasta")}
    files["locus_table"] = os.path.join(inter, sample + ".vcf_filtered.tsv")
    clock = [time.time()]

    def done(stage, text):
        now = time.time()
        seconds[stage] = now - clock[0]
        clock[0] = now
        _say("[telr] %-10s %s (%.2f s)" % (stage, text, seconds[stage]))

    if getattr(args, "inert_given", None):
        _say("[telr] " + INERT)
    sites_path = getattr(args, "sites", None)
    if sites_path is not None and getattr(args, "sites_inert_given", None):
        _say("[telr] %s %s no effect with --sites: the run genotypes the listed sites and has no discovery, draft or loci stage"
             % (", ".join(args.sites_inert_given), "has" if len(args.sites_inert_given) == 1 else "have"))
    own_engine = engine is None
    eng = make_engine(args.device) if own_engine else engine
    release = None
    ix = ix10 = cset = None
    try:
        # 1. reference and library; the reference goes by a link in the intermediate directory, as parse_input places it (its .fai lands there)
        tnames, tseqs = fasta.read_fasta(args.reference)
        lib_names, lib_seqs = fasta.read_fasta(args.library)
        ref_copy = os.path.join(inter, os.path.basename(args.reference))
        if os.path.islink(ref_copy):
            os.remove(ref_copy)
        if not os.path.exists(ref_copy):
            os.symlink(os.path.abspath(args.reference), ref_copy)
        by_name = dict(zip(tnames, tseqs))
        chrom_ids = {n: i for i, n in enumerate(tnames)}
        listed = None
        if sites_path is not None:                  # refused before anything is mapped
            listed = telr_sv.read_sites(sites_path, chrom_ids, {n: len(q) for n, q in zip(tnames, tseqs)}, report=lambda m: _say("[telr] " + m))
        done("inputs", "%d reference sequences, %d library sequences" % (len(tnames), len(lib_names)) + ("" if listed is None else ", %d sites" % len(listed["sites"])))
        # 2. the stage-1 index
        io, _ = preset(aligner_preset(args)[0])
        ix, n_parts = index_stage(eng, tseqs, io, args.index_part_bases)
        done("index", "stage-1 index (%s), %d part%s" % (aligner_preset(args)[0], n_parts, "" if n_parts == 1 else "s"))
        # 3. the reads: mapped here, or taken from the BAM
        region = getattr(args, "region", None)
        if is_bam(args.reads) and region:
            tlens = [len(s) for s in tseqs]
            qnames, read_set, r, release, info = load_bam_regions(eng, ix, args, tnames, tlens, bam_regions(args, tnames, tlens, listed))
            counts.update(info)
            route = "BAM input, %d regions: %d of its BGZF members inflated, %d of %d records walked selected" % (
                info["regions"], info["members"] + info["header_members"], info["selected"], info["walked"])
        elif is_bam(args.reads):
            qnames, read_set, r, release = load_bam(eng, ix, args, tnames, [len(s) for s in tseqs])
            route = "BAM input"
        else:
            if region:
                _say("[telr] " + REGION_INERT)
            files["bam"] = os.path.join(inter, sample + "_sort.bam")
            qnames, read_set, r, release = load_reads(eng, ix, args, tnames, files["bam"])
            route = "mapped, sorted BAM written"
        counts["reads"] = len(qnames)
        counts["records"] = int(eng.L.telr_result_count(r))
        done("reads", "%d reads, %d records (%s)" % (counts["reads"], counts["records"], route))
        if listed is not None:
            # --sites: the listed sites genotyped, then the outputs; no discovery, draft, asm10 index or loci stage
            site_rows = sites_stage(ix, r, tnames, qnames, listed, args)
            counts["sites"] = len(site_rows)
            counts["sites_supported"] = sum(1 for x in site_rows if x["support"] > 0)
            done("sites", "%d sites genotyped, %d with a supporting read" % (counts["sites"], counts["sites_supported"]))
            files["sites_tsv"] = os.path.join(args.out, sample + ".telr.sites.tsv")
            telr_sv.write_sites_tsv(site_rows, listed["ids"], files["sites_tsv"])
            if listed["vcf"]:
                files["sites_vcf"] = os.path.join(args.out, sample + ".telr.sites.vcf")
                telr_sv.write_sites_vcf(site_rows, listed, sample, files["sites_vcf"])
            done("outputs", "%d sites written to %s" % (len(site_rows), files["sites_tsv"]))
            return dict(final=[], files=files, counts=counts, seconds=seconds, sites=site_rows)
        # 4. the calls, genotyped
        bridge = bool(getattr(args, "bridge", False))
        rows, ic = call_stage(ix, r, tnames, qnames, read_set, sample, bridge) if bridge else call_stage(ix, r, tnames, qnames, read_set, sample)
        counts["calls"] = len(rows)
        done("calls", "%d insertion calls" % len(rows))
        if not rows:
            # "no loci" is a normal end (src/telr/telr.py:176): header-only VCF, empty BED
            final, _ = locus_pipeline.write_outputs(EMPTY_RESULT, [], args.out, sample, ref_copy, sv_info={})
            telr_sv.write_locus_table([], files["locus_table"])
            done("outputs", "TELR found no non-reference TE insertions")
            return dict(final=final, files=files, counts=counts, seconds=seconds)
        # 5. a draft per call
        if bridge:
            loci, cset, skipped = draft_stage(ix, r, ic, rows, read_set, chrom_ids, True)
            # a bridged call's row: the length and the ALT are the bridge's (the caller had no sized signature to take them from)
            by_locus = {l["name"]: l for l in loci if l.get("bridged")}
            for row in rows:
                l = by_locus.get(telr_sv.locus_name(row))
                if l is not None:
                    row[3], row[7] = str(l["ins_len"]), l["alt"] or "N"
            counts["calls_bridged"] = len(by_locus)
            counts["calls_without_draft"] = len(skipped)
            done("drafts", "%d drafts, %d of them bridges of two reads, %d calls without one" % (len(loci), len(by_locus), len(skipped)))
        else:
            loci, cset, skipped = draft_stage(ix, r, ic, rows, read_set, chrom_ids)
            counts["calls_without_draft"] = len(skipped)
            done("drafts", "%d drafts, %d calls without one" % (len(loci), len(skipped)))
        if hasattr(eng, "release_scratch"):
            eng.release_scratch()                   # stage 1 will not run again: its mapping scratch goes back to the device
        # 6. the asm10 index over the same resident reference
        io10, _ = preset("asm10")
        ix10, n_parts10 = index_stage(eng, None, io10, args.index_part_bases, like=ix)
        done("index10", "asm10 index of the reference, %d part%s" % (n_parts10, "" if n_parts10 == 1 else "s"))
        ref_te_rows = None
        if args.ref_te != "none" and loci:          # (only the liftover of a locus reads them)
            files["ref_te"] = os.path.join(inter, os.path.basename(args.reference) + ".te.bed") if args.ref_te == "engine" else args.ref_te
            ref_te_rows = ref_te_stage(eng, ix, tnames, lib_names, lib_seqs, args, files["ref_te"])
            counts["ref_te_features"] = len(ref_te_rows)
            done("ref_te", "%d reference TE features (%s)" % (len(ref_te_rows), "annotated on the device" if args.ref_te == "engine" else "from " + args.ref_te))
        # 7. annotation, liftover, allele frequency
        res = loci_stage(eng, ix10, tnames, lambda ch: by_name[ch], loci, lib_names, lib_seqs, read_set, cset, args, ref_te_rows) if loci else dict(EMPTY_RESULT)
        counts["loci_annotated"] = len(set(a[0] for a in res["annotation"]))
        counts["loci_lifted"] = sum(1 for x in res["liftover"] if x["report"]["type"] == "non-reference")
        done("loci", "%d loci annotated, %d lifted over" % (counts["loci_annotated"], counts["loci_lifted"]))
        # 8. the outputs
        loci_out = [dict(l, contig=res["contigs"][l["name"]]) for l in loci] if "contigs" in res else loci
        final, _ = locus_pipeline.write_outputs(res, loci_out, args.out, sample, ref_copy, sv_info=telr_sv.sv_info(rows))
        telr_sv.write_locus_table(rows, files["locus_table"])          # every call's row (write_outputs leaves those of the drafted ones)
        counts["loci_written"] = len(final)
        done("outputs", "%d insertions written to %s" % (len(final), files["vcf"]))
        return dict(final=final, files=files, counts=counts, seconds=seconds)
    finally:
        if cset is not None:
            cset.free()
        for x in (ix10, ix):
            if x is not None:
                x.free()
        if release is not None:
            release()
        if own_engine and hasattr(eng, "close"):
            eng.close()
        if not args.keep_files:
            shutil.rmtree(inter, ignore_errors=True)


def main(argv=None):
    args = get_args(argv)
    t0 = time.time()
    try:
        out = run(args)
    except SystemExit:
        raise
    except Exception as e:                          # TelrError carries the engine's text; nothing is retried another way
        _say("telr: %s: %s" % (type(e).__name__, e))
        return 1
    if "sites" in out["counts"]:
        _say("[telr] finished in %.2f s: %d sites genotyped" % (time.time() - t0, out["counts"]["sites"]))
        return 0
    _say("[telr] finished in %.2f s: %d insertions" % (time.time() - t0, out["counts"]["loci_written"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
