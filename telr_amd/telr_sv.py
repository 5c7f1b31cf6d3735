"""Candidate-locus table (`<sample>.vcf_filtered.tsv`) handling: schema, merge of nearby calls, helpers.

Mirror of the table-side half of the reference's SV module: `merge_vcf` src/telr/TELR_sv.py:84-140, `string2int`
:143-150, `average` :153-156, `swap_coordinate` :183-190, `rm_vcf_redundancy` :193-228, `filter_vcf` :231-324,
`write_ins_seqs` :328-334, `id_merge` :337-341, `get_unique_list` :343-348, `af_sum` :351-355, and `create_loci_set`
src/telr/TELR_utility.py:44-50.  Calling Sniffles / bcftools (`detect_sv`, the query in `parse_vcf`) is outside the
alignment path and not provided; its opt-in counterpart is `call_insertions`: the engine's own insertion caller
(`telr_call_insertions`, a definition of its own, not Sniffles') run on the stage-1 result, returning rows of this table.  `filter_vcf` keeps the reference's table arithmetic and takes the TE intervals of the
ALT sequences from a `screen`: `gff_screen` reads a RepeatMasker `.out.gff` (the reference's source, :256-295),
`engine_screen` (opt-in: it changes which loci pass) maps the TE library onto the ALT sequences
with the HIP engine instead.  `genotype_sites` answers the other question of a cohort study: for a site list that came from
somewhere else (`read_sites`: a VCF of this project or a TSV), what does THIS sample show there -- supporters, reference reads and a
genotype per site, `0/0` and `./.` included (`telr_call_at_sites`; not Sniffles' forced genotyping).  The list itself
can come from the cohort's own calls: `read_cohort` -> `merge_site_lists` (`telr_merge_sites`; not bcftools merge, SURVIVOR
or Jasmine) -> `write_cohort_tsv` / `write_cohort_vcf`, and `join_sites_vcfs` puts the per-sample results into one multi-sample VCF.

The 14 columns are addressed by index by every later stage; COLUMNS names them.

Kept on purpose:
  * the representative call of a merged group is chosen with `max()` over the SV lengths *as text*
    (lexicographic: "999" beats "1000"), TELR_sv.py:103-104;
  * merged start/end are Python-`round`ed means (ties to even), coverage is a float sum, AF a float sum capped to the
    integer 1, alt_count the number of distinct supporting reads (:100-115).
One deliberate difference: distinct read names keep first-appearance order instead of `set` iteration order, which in
the reference depends on PYTHONHASHSEED; the set of names, and therefore alt_count, is identical.
"""
COLUMNS = ("chrom", "start", "end", "sv_length", "coverage", "sniffles_af", "sv_id", "ins_seq", "reads", "filter",
           "genotype", "ref_count", "alt_count", "ins_te_prop")


_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
# what a row made by call_insertions(genotype=None) holds where Sniffles would supply a value the caller does not compute: an AF that parses as a
# float (merge_rows and dedup_rows add the column up), the VCF missing genotype, a ref_count that is text (summed as text, printed as is)
NO_AF, NO_GENOTYPE, NO_REF_COUNT, NO_TE_PROP = "nan", "./.", "NA", "NA"
GENOTYPES = ("0/0", "0/1", "1/1")          # telr_ins_gt.gt 0, 1, 2


def call_insertions(index, result, tnames, qnames, reads, opt=None, sample="telr", te_prop_column=True, genotype=None):
    """Candidate-locus rows (COLUMNS order; te_prop_column=False leaves the 14th out, for a table that goes through `filter_vcf`,
    which appends it) from a stage-1 result, with the engine's
    own insertion caller (`telr_call_insertions`) in the place of `detect_sv` + `parse_vcf` (TELR_sv.py:13-81,
    159-181).  Opt-in and NOT Sniffles: another definition of a call, whose agreement with Sniffles is not pinned.
    index: the aligner.Index the reads were mapped against; result: the raw handle of `index.map_raw`; tnames / qnames: target
    and read names by id; reads: the read sequences (a list of str / bytes, or the (buffer, offsets, lengths) triple given to
    `seqset`), or the resident `aligner.SeqSet` the result was mapped from: the ALT pieces (the representative signature's qid,
    seg_start, seg_len and its record's strand) are then cut on the device in ONE `SeqSet.extract` call and only they come to the host.
    For reads made only of upper-case A C G T N the rows are equal between the two forms; any other letter comes back as the set
    holds it (lower case as upper case, U as T, anything else N), where host strings give the letter itself.
    opt: an `_abi.InsOpt` (None = defaults).
    start = the call's position, end = start + 1, sv_length = the median length of the sized signatures, coverage = alt_count =
    the distinct supporting reads, ins_seq = the representative signature's segment of its read, on the reference strand.
    Rows are sorted by (target id, position), as `merge_rows` and `telr_assembly.window_reads` take them.
    genotype: None leaves sniffles_af, genotype and ref_count at their placeholders ("nan", "./.", "NA"); True or an `_abi.GenoOpt`
    runs the engine's genotyping step on the calls (`telr_genotype_insertions`, DESIGN.md 5.11 -- an own definition again, NOT
    Sniffles' genotyper) and fills them: sniffles_af = "%.6f" % (alt / (alt + ref)), genotype = 0/0, 0/1 or 1/1, ref_count = the
    distinct reads that cross the call with the reference allele."""
    import numpy as np
    from .aligner import _np_from
    from ._abi import ALN_DTYPE, F_REV
    from .fasta import segment
    ic = index.call_insertions(result, opt)
    L = index.eng.L
    flags = _np_from(L.telr_result_alns(result), L.telr_result_count(result), ALN_DTYPE)["flags"] if len(ic.calls) else None
    gt = None if genotype is None or genotype is False else index.genotype_insertions(result, ic, None if genotype is True else genotype).gt

    cut = None
    if hasattr(reads, "extract"):              # a resident set: every ALT piece in one engine call
        reps = [ic.sigs[c["rep"]] for c in ic.calls if c["rep"] >= 0]
        cut = iter(reads.extract([int(s["qid"]) for s in reps], [int(s["seg_start"]) for s in reps], [int(s["seg_len"]) for s in reps],
                                 [1 if int(flags[s["rec"]]) & F_REV else 0 for s in reps]))
    rows = []
    for k, c in enumerate(ic.calls):
        seq = b"N"
        if c["rep"] >= 0 and cut is not None:
            seq = next(cut) or b"N"
        elif c["rep"] >= 0:
            s = ic.sigs[c["rep"]]
            seq = segment(reads, int(s["qid"]), int(s["seg_start"]), int(s["seg_len"])) or b"N"
            if int(flags[s["rec"]]) & F_REV:
                seq = seq.translate(_RC)[::-1]
        names = ",".join(qnames[q] for q in ic.reads_of(k).tolist())
        af, genotype_text, ref_count = NO_AF, NO_GENOTYPE, NO_REF_COUNT
        if gt is not None:
            alt, ref = int(gt[k]["alt"]), int(gt[k]["ref"])
            af = "%.6f" % (alt / (alt + ref)) if alt + ref else NO_AF
            genotype_text, ref_count = GENOTYPES[int(gt[k]["gt"])], str(ref)
        rows.append([tnames[c["tid"]], str(int(c["pos"])), str(int(c["pos"]) + 1), str(int(c["len"])), str(int(c["support"])), af,
                     "%s.INS.%d" % (sample, k), seq.decode(), names, "PASS", genotype_text, ref_count, str(int(c["support"]))] +
                    ([NO_TE_PROP] if te_prop_column else []))
    return rows


SITE_FIELDS = ("chrom", "pos", "site_len", "len", "support", "n_sized", "ref", "ambig", "gt_text", "af_text", "reads")


def site_texts(alt, ref, gt):
    """(gt_text, af_text) of a site: ./. and nan when no read speaks for either allele (the genotyper's gt is 2 there, since 0 >= 0),
    else the genotyper's 0/0, 0/1 or 1/1 and "%.6f" % (alt / (alt + ref))"""
    if alt + ref == 0:
        return NO_GENOTYPE, NO_AF
    return GENOTYPES[int(gt)], "%.6f" % (alt / (alt + ref))


def genotype_sites(index, result, tnames, qnames, sites, opt=None, site_opt=None, geno_opt=None):
    """Genotype insertion sites that came from somewhere else -- another sample's calls, a cohort's list, a truth set -- on this sample's
    stage-1 result: `Index.call_at_sites` (telr_call_at_sites) gathers the supporters of every site, the existing
    `Index.genotype_insertions` counts the reference and ambiguous reads.  An own definition, NOT Sniffles' forced genotyping
    (--genotype-vcf); its agreement with Sniffles is not pinned.
    sites: an (n, 3) int32 array or a list of (tid, pos, len) triples, strictly ascending by (tid, pos), len = the expected insertion
    length or 0 (`read_sites` gives them); opt / site_opt / geno_opt: an `_abi.InsOpt` / `SiteOpt` / `GenoOpt` (None = defaults).
    -> one dict per site, in site order (SITE_FIELDS): chrom, pos, site_len, len (the lower median length of the kept sized signatures,
    0 without one), support and n_sized (distinct reads), ref and ambig (distinct reads), gt_text (./. when support + ref == 0, else
    0/0, 0/1, 1/1), af_text ("%.6f" % (support / (support + ref)) or nan), reads (the supporters' names, ascending by read id)."""
    import numpy as np
    s = np.asarray(sites, dtype=np.int32).reshape(-1, 3)
    ic = index.call_at_sites(result, s, opt, site_opt)
    gt = index.genotype_insertions(result, ic, geno_opt).gt
    out = []
    for k, c in enumerate(ic.calls):
        alt, ref = int(c["support"]), int(gt[k]["ref"])
        gt_text, af_text = site_texts(alt, ref, gt[k]["gt"])
        out.append(dict(chrom=tnames[int(c["tid"])], pos=int(c["pos"]), site_len=int(s[k][2]), len=int(c["len"]), support=alt, n_sized=int(c["n_sized"]),
                        ref=ref, ambig=int(gt[k]["ambig"]), gt_text=gt_text, af_text=af_text, reads=[qnames[q] for q in ic.reads_of(k).tolist()]))
    return out


def read_sites(path, chrom_ids, chrom_lens=None, report=None, all_lines=False):
    """A site list for `genotype_sites` from a VCF as `telr_output.write_vcf` writes it (a first line `##fileformat=VCF...`), or from a plain
    TSV with the columns chrom, pos0[, len[, id]] (lines starting with # and blank lines are skipped).
    From a VCF: CHROM, the site position POS - 1, ID, and len(ALT) as the expected length when ALT is made of letters, else 0.
    chrom_ids: {chromosome name: target id}; chrom_lens: {name: length} (None: the end is not checked).
    -> dict(sites = [(tid, pos, len), ...] sorted by (tid, pos), ids = their ids ("" without one), vcf = is it a VCF, header = the VCF's
    header lines, lines = the VCF's data lines split into columns, in site order (all_lines: a TSV's too), duplicates = the lines dropped).
    A duplicate (chrom, pos) keeps the first line; all of them are reported in one message (report: a callable taking the text; default
    stderr).  An unknown chromosome, a position that is negative or past the chromosome's end, a negative length or a line that does not
    parse raise ValueError with the line's number."""
    import sys
    with open(path, "r") as fh:
        text = fh.read().splitlines()
    vcf = bool(text) and text[0].startswith("##fileformat=VCF")
    header, found = [], []
    for no, line in enumerate(text, 1):
        if not line.strip():
            continue
        if line.startswith("#"):
            if vcf:
                header.append(line)
            continue
        f = line.split("\t")
        where = "%s line %d: " % (path, no)
        try:
            if vcf:
                if len(f) < 8:
                    raise ValueError("a VCF line has at least 8 columns")
                chrom, pos, ln, sid = f[0], int(f[1]) - 1, len(f[4]) if f[4].isalpha() else 0, f[2]
            else:
                if len(f) < 2:
                    raise ValueError("a site line has the columns chrom, pos0[, len[, id]]")
                chrom, pos, ln, sid = f[0], int(f[1]), int(f[2]) if len(f) > 2 and f[2] != "" else 0, f[3] if len(f) > 3 else ""
        except ValueError as e:
            raise ValueError(where + str(e))
        if chrom not in chrom_ids:
            raise ValueError(where + "chromosome %r is not in the reference" % chrom)
        if pos < 0 or (chrom_lens is not None and pos > chrom_lens[chrom]):
            raise ValueError(where + "position %d is negative or past the end of %s" % (pos, chrom))
        if ln < 0:
            raise ValueError(where + "negative length")
        found.append(((chrom_ids[chrom], pos), ln, sid, f))
    found.sort(key=lambda x: x[0])          # stable: the first line of a position stays first
    kept = [x for k, x in enumerate(found) if k == 0 or x[0] != found[k - 1][0]]
    dup = len(found) - len(kept)
    if dup:
        (report or (lambda m: sys.stderr.write(m + "\n")))("%s: %d line%s repeat%s the (chrom, pos) of an earlier line; the first line of a position is kept"
                                                          % (path, dup, "" if dup == 1 else "s", "s" if dup == 1 else ""))
    return dict(sites=[(k[0], k[1], ln) for k, ln, _, _ in kept], ids=[sid for _, _, sid, _ in kept], vcf=vcf, header=header,
                lines=[f for _, _, _, f in kept] if vcf or all_lines else [], duplicates=dup)


# ---- a cohort: several samples' calls -> one site list ----------------------------------------------------------
NO_FAMILY = "."
COHORT_FIELDS = ("chrom", "pos", "len", "id", "family", "n_samples", "n_members", "n_sized", "len_min", "len_max", "pos_min", "pos_max", "crowded", "samples")


def _sample_name(path):
    import os
    base = os.path.basename(path)
    return base[:-len(".telr.vcf")] if base.endswith(".telr.vcf") else os.path.splitext(base)[0]


def _family_of(fields, vcf):
    if not vcf:
        return fields[4] if len(fields) > 4 and fields[4] != "" else NO_FAMILY
    for kv in fields[7].split(";"):
        if kv.startswith("FAMILY="):
            return kv[len("FAMILY="):] or NO_FAMILY
    return NO_FAMILY


def read_cohort(paths, chrom_ids, chrom_lens=None, by_family=True, report=None):
    """The per-sample call files of a cohort -> the entries `merge_site_lists` takes.  Every file is read by `read_sites`, with its rules (a
    VCF of this project or a TSV; a repeated (chrom, pos) within one file keeps its first line); the family of a call is FAMILY= in INFO of a
    VCF line, the optional fifth column of a TSV line, `.` without one.  The sample of file k is number k; its name is the file's base
    name without `.telr.vcf` (else without its extension), and two files of one name are refused (ValueError).  by_family: the family
    names, sorted, are numbered as the groups (calls of different families never merge -- by NAME: one family under two spellings is
    two groups); else every call is in group 0.
    -> dict(entries = a COHORT_ENTRY_DTYPE array in file order, samples = the sample names, families = the group's name by number (["*"]
    without by_family), family = the family name of every entry, origin = (file number, line number in its `lines`) of every entry,
    inputs = what read_sites returned per file, vcf = is every file a VCF, chroms = the chromosome name by id)."""
    import numpy as np
    from ._abi import COHORT_ENTRY_DTYPE
    names = [_sample_name(p) for p in paths]
    for k, n in enumerate(names):
        if n in names[:k]:
            raise ValueError("%s and %s are both sample %r: sample names come from the file names and must differ" % (paths[names.index(n)], paths[k], n))
    inputs = [read_sites(p, chrom_ids, chrom_lens, report=report, all_lines=True) for p in paths]
    family, origin, raw = [], [], []
    for k, listed in enumerate(inputs):
        for j, ((tid, pos, ln), f) in enumerate(zip(listed["sites"], listed["lines"])):
            family.append(_family_of(f, listed["vcf"]))
            origin.append((k, j))
            raw.append((tid, pos, ln, k))
    families = sorted(set(family)) if by_family else ["*"]
    number = {n: g for g, n in enumerate(families)}
    entries = np.zeros(len(raw), COHORT_ENTRY_DTYPE)
    for i, (tid, pos, ln, k) in enumerate(raw):
        entries[i] = (tid, pos, ln, k, number[family[i]] if by_family else 0)
    chroms = [None] * len(chrom_ids)
    for n, t in chrom_ids.items():
        chroms[t] = n
    return dict(entries=entries, samples=names, families=families, family=family, origin=origin, inputs=inputs, vcf=bool(inputs) and all(x["vcf"] for x in inputs), chroms=chroms)


def merge_site_lists(engine, cohort, opt=None):
    """the entries of `read_cohort` merged on the device (`Engine.merge_sites`, telr_merge_sites, DESIGN.md 5.21: an own definition, NOT
    bcftools merge, SURVIVOR or Jasmine) -> one dict per site in final order, shadowed ones included and marked: COHORT_FIELDS (id =
    chrom:pos0:family, samples = the names of its samples) plus group, rep (the entry that gives its length), members (its entries),
    shadowed, winner (the row that shadows it, or -1)."""
    res = engine.merge_sites(cohort["entries"], len(cohort["chroms"]), opt)
    return cohort_rows(cohort, res.sites, res.members_of, res.samples_of)


def cohort_rows(cohort, sites, members_of, samples_of):
    """the rows of `merge_site_lists` from the merged sites (records with the fields of telr_cohort_site) and the two list accessors"""
    from ._abi import COHORT_SHADOWED, COHORT_CROWDED
    rows = []
    for k, s in enumerate(sites):
        chrom, fam = cohort["chroms"][int(s["tid"])], cohort["families"][int(s["group"])]
        row = dict(chrom=chrom, pos=int(s["pos"]), len=int(s["len"]), id="%s:%d:%s" % (chrom, int(s["pos"]), fam), family=fam)
        row.update({f: int(s[f]) for f in ("n_samples", "n_members", "n_sized", "len_min", "len_max", "pos_min", "pos_max", "group", "rep", "winner")})
        row.update(crowded=bool(int(s["flags"]) & COHORT_CROWDED), shadowed=bool(int(s["flags"]) & COHORT_SHADOWED),
                   samples=[cohort["samples"][int(q)] for q in samples_of(k)], members=[int(i) for i in members_of(k)])
        rows.append(row)
    return rows


def write_cohort_tsv(rows, path):
    """the rows of `merge_site_lists` -> `cohort.sites.tsv`: a header line, then one line per site with COHORT_FIELDS (crowded as 0 / 1, samples
    joined by commas).  chrom, pos0, len, id come first, so `read_sites` reads the file as it stands (and `read_cohort`, the family being the
    fifth column); a shadowed site is a comment line `#shadowed`, which `read_sites` skips: it reads exactly the sites that are not shadowed."""
    with open(path, "w") as fh:
        fh.write("#" + "\t".join(COHORT_FIELDS) + "\n")
        for r in rows:
            cells = [str(int(r[k])) if k == "crowded" else ",".join(r[k]) if k == "samples" else str(r[k]) for k in COHORT_FIELDS]
            fh.write(("#shadowed\t" if r["shadowed"] else "") + "\t".join(cells) + "\n")


COHORT_VCF_META = ('##INFO=<ID=NSAMP,Number=1,Type=Integer,Description="samples of the cohort with a call merged into this site">',
                   '##INFO=<ID=SAMPLES,Number=.,Type=String,Description="their names">')


def write_cohort_vcf(rows, cohort, path):
    """the rows of `merge_site_lists` -> `cohort.sites.vcf`, only when every input was a VCF (ValueError otherwise): the first input's header
    (with the two INFO lines of COHORT_VCF_META before its #CHROM line, which is cut to the eight fixed columns), then one line per site that is
    not shadowed: the eight fixed columns of its `rep` entry's line with POS = pos + 1, ID = the site's id and `;NSAMP=..;SAMPLES=a,b`
    appended to INFO.  `read_sites` reads it as a site list."""
    if not cohort["vcf"]:
        raise ValueError("write_cohort_vcf: every input must be a VCF")
    with open(path, "w") as fh:
        for line in cohort["inputs"][0]["header"]:
            if line.startswith("#CHROM"):
                fh.write("\n".join(COHORT_VCF_META) + "\n")
                line = "\t".join(line.split("\t")[:8])
            fh.write(line + "\n")
        for r in rows:
            if r["shadowed"]:
                continue
            k, j = cohort["origin"][r["rep"]]
            f = list(cohort["inputs"][k]["lines"][j][:8])
            f[1], f[2] = str(r["pos"] + 1), r["id"]
            f[7] = (f[7] + ";" if f[7] not in ("", ".") else "") + "NSAMP=%d;SAMPLES=%s" % (r["n_samples"], ",".join(r["samples"]))
            fh.write("\t".join(f) + "\n")


def join_sites_vcfs(paths, out):
    """the `<sample>.telr.sites.vcf` files of `--sites` runs on ONE site list -> one multi-sample VCF (host glue): the first file's header
    with every file's sample name in the #CHROM line, FORMAT GT:DR:DV, one sample column per file in the order given.  The eight fixed
    columns of every line must be equal across the files, and so must the number of lines; where they are not, ValueError names the file
    and the line.  -> the number of sites written."""
    if not paths:
        raise ValueError("join_sites_vcfs: no input")
    files = []
    for p in paths:
        with open(p, "r") as fh:
            text = fh.read().splitlines()
        head = [(no, l) for no, l in enumerate(text, 1) if l.startswith("#")]
        data = [(no, l.split("\t")) for no, l in enumerate(text, 1) if l.strip() and not l.startswith("#")]
        chrom = [l for _, l in head if l.startswith("#CHROM")]
        if not chrom or len(chrom[0].split("\t")) != 10:
            raise ValueError("%s: no #CHROM line with one sample column" % p)
        for no, f in data:
            if len(f) != 10 or f[8] != "GT:DR:DV":
                raise ValueError("%s line %d: not a line of ten columns with FORMAT GT:DR:DV" % (p, no))
        files.append(dict(path=p, head=[l for _, l in head], data=data, sample=chrom[0].split("\t")[9]))
    first = files[0]
    for x in files[1:]:
        if len(x["data"]) != len(first["data"]):
            raise ValueError("%s: %d sites, but %s has %d: the files must come from one site list" % (x["path"], len(x["data"]), first["path"], len(first["data"])))
        for (no, f), (_, g) in zip(x["data"], first["data"]):
            if f[:8] != g[:8]:
                raise ValueError("%s line %d: the eight fixed columns differ from those of %s" % (x["path"], no, first["path"]))
    with open(out, "w") as fh:
        for line in first["head"]:
            if line.startswith("#CHROM"):
                line = "\t".join(line.split("\t")[:9] + [x["sample"] for x in files])
            fh.write(line + "\n")
        for k, (_, f) in enumerate(first["data"]):
            fh.write("\t".join(f[:8] + ["GT:DR:DV"] + [x["data"][k][1][9] for x in files]) + "\n")
    return len(first["data"])


def write_sites_tsv(rows, ids, path):
    """the dicts of `genotype_sites` -> `<sample>.telr.sites.tsv`: a header line, then one line per site: id, SITE_FIELDS (reads joined by commas, `.` for none)"""
    with open(path, "w") as fh:
        fh.write("#id\t" + "\t".join(SITE_FIELDS) + "\n")
        for sid, r in zip(ids, rows):
            fh.write("\t".join([sid or "."] + [str(r[k]) for k in SITE_FIELDS[:-1]] + [",".join(r["reads"]) or "."]) + "\n")


def write_sites_vcf(rows, listed, sample, path):
    """the input VCF (`listed`: what `read_sites` returned) with this run's genotypes -> `<sample>.telr.sites.vcf`: the header as it was with
    the sample's name in the #CHROM line, the eight fixed columns of every kept input line as they were, FORMAT GT:DR:DV and the sample
    column GT : reference reads : supporting reads.  (This column follows its FORMAT string; `<sample>.telr.vcf` keeps the reference's
    swapped order, telr_output.py.)"""
    with open(path, "w") as fh:
        for line in listed["header"]:
            if line.startswith("#CHROM"):
                line = "\t".join(line.split("\t")[:9] + [sample]) if line.count("\t") >= 8 else line + "\tFORMAT\t" + sample
            fh.write(line + "\n")
        for f, r in zip(listed["lines"], rows):
            fh.write("\t".join(f[:8] + ["GT:DR:DV", "%s:%d:%d" % (r["gt_text"], r["ref"], r["support"])]) + "\n")


def sv_info(rows):
    """rows of the candidate-locus table -> {locus name: (genotype, ref_count, alt_count)}, what
    `locus_pipeline.write_outputs(sv_info=...)` takes (columns 10-12)"""
    return {locus_name(r): (r[10], r[11], r[12]) for r in rows}


def write_locus_table(rows, path):
    """rows -> the tab-separated table `read_locus_table` reads"""
    with open(path, "w") as fh:
        for r in rows:
            fh.write("\t".join(str(v) for v in r) + "\n")


def string2int(lst, integer=True):
    """in-place conversion of a list of numerals, returned for chaining"""
    conv = int if integer else float
    for i, v in enumerate(lst):
        lst[i] = conv(v)
    return lst


def average(lst):
    nums = string2int(lst.split(";"))
    return round(sum(nums) / len(nums))


def af_sum(nums):
    total = sum(nums)
    return 1 if total > 1 else total


def get_unique_list(list1):
    return list(dict.fromkeys(list1))


def id_merge(strings):
    return ",".join(get_unique_list(",".join(strings).split(",")))


def read_locus_table(path):
    """-> list of 14+-column rows (lists of str) in file order"""
    with open(path, "r") as fh:
        return [line.replace("\n", "").split("\t") for line in fh if line.strip()]


def locus_name(row):
    return "_".join(row[0:3])


def create_loci_set(vcf_parsed):
    return set(locus_name(r) for r in read_locus_table(vcf_parsed))


def bedtools_merge_rows(rows, window=20):
    """`bedtools merge -o collapse -c 2,...,14 -delim ";" -d WINDOW` on the (already sorted) table:
    chrom, merged start, merged end, then the 13 collapsed columns."""
    out = []
    for chrom, s, e, members in _groups(rows, window):
        out.append([chrom, str(s), str(e)] + [";".join(m[k] for m in members) for k in range(1, 14)])
    return out


def _groups(rows, window):
    cur = None
    for r in rows:
        s, e = int(r[1]), int(r[2])
        if cur is not None and cur[0] == r[0] and s <= cur[2] + window:
            cur[2] = max(cur[2], e)
            cur[3].append(r)
        else:
            if cur is not None:
                yield cur
            cur = [r[0], s, e, [r]]
    if cur is not None:
        yield cur


def collapse_group(entry):
    """one line of the merge intermediate -> one 14-column locus row (TELR_sv.py:97-138)"""
    if ";" not in entry[3]:
        return [entry[0]] + entry[3:]
    lens = entry[5].split(";")
    idx = lens.index(max(lens))
    reads = ",".join(get_unique_list(entry[10].replace(";", ",").split(",")))
    pick = lambda k: entry[k].split(";")[idx]
    return [entry[0], str(average(entry[3])), str(average(entry[4])), str(lens[idx]),
            str(sum(string2int(entry[6].split(";"), integer=False))), str(af_sum(string2int(entry[7].split(";"), integer=False))),
            pick(8), pick(9), reads, pick(11), pick(12), str(pick(13)), str(len(reads.split(","))), str(pick(15))]


def merge_rows(rows, window=20):
    return [collapse_group(e) for e in bedtools_merge_rows(rows, window)]


def merge_vcf(vcf_in, vcf_out, window=20):
    rows = merge_rows(read_locus_table(vcf_in), window)
    with open(vcf_out, "w") as out:
        for r in rows:
            out.write("\t".join(r) + "\n")


def write_ins_seqs(vcf, out):
    with open(out, "w") as fh:
        for r in read_locus_table(vcf):
            fh.write(">" + locus_name(r) + "\n" + r[7] + "\n")


def swap_coordinate(vcf_in, vcf_out):
    """start/end exchanged where end < start (compared as integers, written back as the original text)"""
    with open(vcf_out, "w") as out:
        for r in read_locus_table_raw(vcf_in):
            if int(r[2]) < int(r[1]):
                r[1], r[2] = r[2], r[1]
            out.write("\t".join(r) + "\n")


def read_locus_table_raw(path):
    """every line, blank ones included, split on tabs (swap_coordinate does not skip anything)"""
    with open(path, "r") as fh:
        return [line.replace("\n", "").split("\t") for line in fh]


def _typed_column(values):
    """column type inference as the table reader of the reference does it (pandas.read_csv on a headerless TSV):
    all integers -> int, else all numbers -> float, else text as is.  Missing-value handling is not reproduced
    (the parsed VCF table has no empty fields)."""
    for conv in (int, float):
        try:
            return [conv(v) for v in values]
        except ValueError:
            pass
    return list(values)


def _cell_text(v):
    return repr(v) if isinstance(v, float) else str(v)


def _column_sum(vals):
    return sum(vals) if not isinstance(vals[0], str) else "".join(vals)


def dedup_rows(rows):
    """rows sharing (chrom, start, end) collapse to one: first length / id / sequence / filter / genotype, summed
    coverage and read counts, capped AF sum, union of read names (TELR_sv.py:209-227).  Returns typed rows sorted
    by (chrom, start, end) as the group-by does; an AF column whose every group sum was capped prints as the integer."""
    cols = [_typed_column([r[k] for r in rows]) for k in range(13)]
    groups = {}
    for i in range(len(rows)):
        groups.setdefault((cols[0][i], cols[1][i], cols[2][i]), []).append(i)
    out = []
    for key in sorted(groups):
        m = groups[key]
        first = lambda k: cols[k][m[0]]
        out.append([key[0], key[1], key[2], first(3), _column_sum([cols[4][i] for i in m]),
                    af_sum([cols[5][i] for i in m]), first(6), first(7), id_merge([str(cols[8][i]) for i in m]),
                    first(9), first(10), _column_sum([cols[11][i] for i in m]), _column_sum([cols[12][i] for i in m])])
    if any(isinstance(r[5], float) for r in out):
        for r in out:
            r[5] = float(r[5])
    return out


def rm_vcf_redundancy(vcf_in, vcf_out):
    rows = dedup_rows(read_locus_table(vcf_in))
    with open(vcf_out, "w") as out:
        for r in rows:
            out.write("\t".join(_cell_text(v) for v in r) + "\n")


def gff_screen(gff_path):
    """RepeatMasker `.out.gff` -> merged TE intervals per ALT sequence: `bedtools sort` then `bedtools merge` on a GFF
    (1-based inclusive features, 0-based starts printed, overlapping and book-ended features joined), TELR_sv.py:283-295"""
    feats = []
    with open(gff_path, "r") as fh:
        for line in fh:
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\n").split("\t")
            feats.append((f[0], int(f[3]) - 1, int(f[4])))
    return merge_intervals(feats)


def merge_intervals(feats):
    out = []
    for name, s, e in sorted(feats, key=lambda f: (f[0], f[1])):
        if out and out[-1][0] == name and s <= out[-1][2]:
            out[-1][2] = max(out[-1][2], e)
        else:
            out.append([name, s, e])
    return out


def engine_screen(backend, presets="ont", min_len=0):
    """-> screen(ins_fasta, te_library, thread) that maps every TE consensus onto every ALT sequence in one engine call
    (library sketched once, chains ranked per ALT sequence) and returns the merged target intervals.  Replaces the
    RepeatMasker run of TELR_sv.py:253-281; hit sets differ from RepeatMasker's, hence opt-in."""
    from . import fasta
    from ._abi import MF_PER_TARGET
    from .presets import preset

    def screen(ins_fasta, te_library, thread):
        names, seqs = fasta.read_fasta(ins_fasta)
        _, lib = fasta.read_fasta(te_library)
        if not names or not lib:
            return []
        io, mo = preset("map-ont" if presets == "ont" else "map-pb")
        mo = mo.copy(); mo.flags |= MF_PER_TARGET
        res = backend.index(list(seqs), io).map(list(lib), mo)
        return merge_intervals([(names[a["tid"]], int(a["ts"]), int(a["te"])) for a in res.alns
                                if int(a["te"]) - int(a["ts"]) >= min_len])
    return screen


def te_proportions(merged, contig_len):
    """per ALT sequence: the SUM over its merged TE intervals of round(interval length / sequence length, 2)
    (rounded per interval, then added as floats, TELR_sv.py:298-309)"""
    props = {}
    for name, s, e in merged:
        p = round((int(e) - int(s)) / contig_len[name], 2)
        props[name] = props[name] + p if name in props else p
    return props


def filter_vcf(ins, ins_filtered, te_library, out, sample_name, thread, loci_eval, screen=None):
    """keep the loci whose ALT sequence carries TE sequence and append the TE proportion as column 14; the others are
    appended to `loci_eval` as "VCF sequence not repeatmasked".  `screen(ins_fasta, te_library, thread)` supplies the
    merged TE intervals; there is no default (RepeatMasker is a hand-off point): pass `engine_screen(engine)` or
    `lambda *a: gff_screen(path)`."""
    import os
    if screen is None:
        raise ValueError("filter_vcf needs a screen: engine_screen(backend) or a RepeatMasker GFF via gff_screen")
    ins_seqs = os.path.join(out, sample_name.replace("+", "plus") + ".vcf_ins.fasta")
    write_ins_seqs(ins, ins_seqs)
    rows = read_locus_table(ins)
    contig_len = {locus_name(r): len(r[7]) for r in rows}
    props = te_proportions(screen(ins_seqs, te_library, thread), contig_len)
    with open(ins_filtered, "w") as fh:
        for r in rows:
            if locus_name(r) in props:
                fh.write("\t".join(r) + "\t" + str(props[locus_name(r)]) + "\n")
    with open(loci_eval, "a") as fh:
        seen = set()
        for r in rows:
            n = locus_name(r)
            if n not in props and n not in seen:
                seen.add(n)
                fh.write(n + "\tVCF sequence not repeatmasked\n")
