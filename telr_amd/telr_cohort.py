"""`python -m telr_amd.telr_cohort`: the two cohort steps around `telr --sites`.

    merge -r reference.fasta -o out [--dist N] [--min_samples N] [--no_family] [--device N] a.telr.vcf b.telr.vcf ...
        several samples' calls -> ONE site list, merged on the device (`Engine.merge_sites`, telr_merge_sites): writes out/cohort.sites.tsv
        and, when every input is a VCF, out/cohort.sites.vcf.  Either is what `telr --sites` takes.
    join -o out.vcf s1.telr.sites.vcf s2.telr.sites.vcf ...
        the per-sample results of `telr --sites` runs on that one list -> one multi-sample VCF (host glue, no device).

The merge is an own, fully specified definition (include/telr_hip.h), NOT bcftools merge, SURVIVOR or Jasmine; its agreement with them is
not pinned.  Stated limits: single linkage can chain; the group is the family NAME the input gives, so one family under two spellings does
not merge; shadowed sites (one position, several families) and crowded sites (another site within --dist) are reported, not resolved --
`telr --sites` assigns signatures by position only; strand and TSD are not compared.
"""
import argparse
import os
import sys
import time

from .telr import _say, make_engine


def get_args(argv=None):
    p = argparse.ArgumentParser(prog="telr_cohort", description="merge several samples' TELR calls into one site list, and join the genotyped lists")
    sub = p.add_subparsers(dest="command", required=True)
    m = sub.add_parser("merge", help="several samples' <sample>.telr.vcf (or site TSVs) -> cohort.sites.tsv (and cohort.sites.vcf)")
    m.add_argument("-r", "--reference", type=str, required=True, help="reference genome in fasta format (its .fai is read when present)")
    m.add_argument("-o", "--out", type=str, default=".", help="directory to output data (default = '.')")
    m.add_argument("--dist", type=int, default=50, help="calls of one family at most N bases apart merge, single linkage (default = 50)")
    m.add_argument("--min_samples", type=int, default=1, help="drop sites seen in fewer than N samples (default = 1)")
    m.add_argument("--no_family", action="store_true", help="merge calls whatever their family (default: calls of different families never merge)")
    m.add_argument("--device", type=int, default=0, help="the GPU to run on (default = 0)")
    m.add_argument("inputs", nargs="+", help="one file per sample: a VCF as telr writes it, or a TSV with the columns chrom, pos0[, len[, id[, family]]]")
    j = sub.add_parser("join", help="the <sample>.telr.sites.vcf of `telr --sites` runs on one list -> one multi-sample VCF")
    j.add_argument("-o", "--out", type=str, required=True, help="the VCF to write")
    j.add_argument("inputs", nargs="+", help="one <sample>.telr.sites.vcf per sample, all from one site list")
    return p.parse_args(argv)


def reference_table(reference):
    """-> (names, lengths) of the reference's sequences: from `reference`.fai when there is one, else from the FASTA"""
    if os.path.isfile(reference + ".fai"):
        with open(reference + ".fai", "r") as fh:
            rows = [l.split("\t") for l in fh.read().splitlines() if l.strip()]
        return [r[0] for r in rows], [int(r[1]) for r in rows]
    from . import fasta
    names, seqs = fasta.read_fasta(reference)
    return names, [len(s) for s in seqs]


def run(args, engine=None):
    """One run with the Namespace of `get_args` -> merge: dict(rows = the dicts of telr_sv.merge_site_lists, files = {sites_tsv[, sites_vcf]},
    counts = {samples, entries, families, sites, shadowed, crowded}, seconds = {stage: wall time}); join: dict(files = {vcf}, counts =
    {samples, sites}).  engine: an aligner.Engine to merge on (default: a new one on args.device, closed at the end).  Engine errors are
    raised as TelrError; a file that does not parse raises ValueError; nothing falls back to another path."""
    from . import telr_sv
    seconds = {}
    clock = [time.time()]

    def done(stage, text):
        now = time.time()
        seconds[stage] = now - clock[0]
        clock[0] = now
        _say("[telr_cohort] %-10s %s (%.2f s)" % (stage, text, seconds[stage]))

    if args.command == "join":
        n = telr_sv.join_sites_vcfs(args.inputs, args.out)
        done("join", "%d sites of %d samples" % (n, len(args.inputs)))
        return dict(files=dict(vcf=args.out), counts=dict(samples=len(args.inputs), sites=n), seconds=seconds)

    from ._abi import CohortOpt
    names, lens = reference_table(args.reference)
    cohort = telr_sv.read_cohort(args.inputs, {n: i for i, n in enumerate(names)}, dict(zip(names, lens)), by_family=not args.no_family,
                                 report=lambda m: _say("[telr_cohort] " + m))
    done("inputs", "%d calls of %d samples, %d %s" % (len(cohort["entries"]), len(cohort["samples"]), len(cohort["families"]),
                                                      "families" if not args.no_family else "group (--no_family)"))
    own_engine = engine is None
    eng = make_engine(args.device) if own_engine else engine
    try:
        rows = telr_sv.merge_site_lists(eng, cohort, CohortOpt.default(dist=args.dist, min_samples=args.min_samples))
    finally:
        if own_engine:
            eng.close()
    counts = dict(samples=len(cohort["samples"]), entries=len(cohort["entries"]), families=len(cohort["families"]), sites=sum(1 for r in rows if not r["shadowed"]),
                  shadowed=sum(1 for r in rows if r["shadowed"]), crowded=sum(1 for r in rows if r["crowded"]))
    done("merge", "%d sites; %d more shadowed by a site at their position, %d crowded by a site within %d bases (reported, not resolved)"
         % (counts["sites"], counts["shadowed"], counts["crowded"], args.dist))
    os.makedirs(args.out, exist_ok=True)
    files = dict(sites_tsv=os.path.join(args.out, "cohort.sites.tsv"))
    telr_sv.write_cohort_tsv(rows, files["sites_tsv"])
    if cohort["vcf"]:
        files["sites_vcf"] = os.path.join(args.out, "cohort.sites.vcf")
        telr_sv.write_cohort_vcf(rows, cohort, files["sites_vcf"])
    done("outputs", ", ".join(os.path.basename(p) for p in files.values()))
    return dict(rows=rows, files=files, counts=counts, seconds=seconds)


def main(argv=None):
    args = get_args(argv)
    t0 = time.time()
    try:
        out = run(args)
    except (OSError, ValueError, RuntimeError) as e:
        _say("telr_cohort: %s: %s" % (type(e).__name__, e))
        return 1
    _say("[telr_cohort] finished in %.2f s: %d sites" % (time.time() - t0, out["counts"]["sites"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
