"""Times telr_call_insertions on a stage-1 result of BASELINE configs[2] shape (bench.py's data set: --coverage / --genome-scale
make it smaller), once with the result's resident CIGAR copy (TELR_MF_KEEP_CIGARS) and once with the CIGAR array uploaded, and the
plain-Python restatement (tests/inscall_ref.py) on a sample of the reads, scaled to the whole set; then Index.genotype_insertions
(telr_genotype_insertions) on the calls of that result, the same two ways, and Index.draft_contigs (telr_draft_contigs) on the same calls.  Writes profiles/inscall_time.json.
Then Index.call_at_sites (telr_call_at_sites) on the positions of the run's own calls, on the resident copy, next to the
call_insertions time of the same run: profiles/sitecall_time.json.

    python tools/inscall_time.py [--coverage 30] [--genome-scale 1.0] [--repeat 5] [--sample-reads 2000] [--out profiles/inscall_time.json] [--sites-out profiles/sitecall_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", type=float, default=0.0)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sample-reads", type=int, default=2000)
    ap.add_argument("--min-support", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inscall_time.json"))
    ap.add_argument("--sites-out", default=os.path.join(ROOT, "profiles", "sitecall_time.json"))
    a = ap.parse_args()
    import numpy as np
    import bench
    cfg = bench.CONFIGS["c2"]
    ba = argparse.Namespace(config="c2", genome_scale=a.genome_scale, insertions=0, coverage=a.coverage, scaling="strong")
    D = bench.build_dataset(ba, cfg, 0, 1, 1)                      # before the GPU is touched: the generator forks workers
    import torch  # noqa: F401
    import inscall_ref as ref
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    from telr_amd._abi import InsOpt, GenoOpt, DraftOpt, MF_KEEP_CIGARS
    eng = Engine(0)
    io, mo = preset(cfg["preset"])
    ix = eng.index([bytes(r).decode() for r in D["ref"]], io)
    qs = eng.seqset(D["reads"])
    opt = InsOpt.default(min_support=a.min_support)
    gopt = GenoOpt.default()
    dopt = DraftOpt.default()

    def timed(r):
        ts = []
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            ic = ix.call_insertions(r, opt)
            ts.append((time.perf_counter() - t0) * 1e3)
        return ic, ts[1:]                                          # the first call sizes the context's scratch

    def timed_geno(r, ic):
        ts = []
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            ig = ix.genotype_insertions(r, ic, gopt)
            ts.append((time.perf_counter() - t0) * 1e3)
        return ig, ts[1:]

    def timed_draft(r, ic):
        ts = []
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            d, s = ix.draft_contigs(r, ic, qs, dopt)
            ts.append((time.perf_counter() - t0) * 1e3)
            out = d, int(s.len.sum())
            s.free()
        return out, ts[1:]

    def timed_sites(r, ic):
        """the run's own calls as sites: (tid, pos, the call's length)"""
        sites = np.ascontiguousarray(np.stack([ic.calls["tid"], ic.calls["pos"], ic.calls["len"]], axis=1), dtype=np.int32)
        ts = []
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            sc = ix.call_at_sites(r, sites, opt)
            ts.append((time.perf_counter() - t0) * 1e3)
        return sc, ts[1:]

    mk = mo.copy(); mk.flags |= MF_KEEP_CIGARS
    r = ix.map_raw(qs, mk)
    res = ix.result_arrays(r)
    ic_res, ms_res = timed(r)
    sc_res, sms_res = timed_sites(r, ic_res)
    ig_res, gms_res = timed_geno(r, ic_res)
    (dr_res, dr_bases), dms_res = timed_draft(r, ic_res)
    ix.free_raw(r)
    r = ix.map_raw(qs, mo)
    ic_up, ms_up = timed(r)
    ig_up, gms_up = timed_geno(r, ic_up)
    (dr_up, _), dms_up = timed_draft(r, ic_up)
    ix.free_raw(r)
    assert ic_res.sigs.tobytes() == ic_up.sigs.tobytes() and ic_res.calls.tobytes() == ic_up.calls.tobytes()
    assert ig_res.gt.tobytes() == ig_up.gt.tobytes() and ig_res.ref_reads.tobytes() == ig_up.ref_reads.tobytes() and ig_res.ambig_reads.tobytes() == ig_up.ambig_reads.tobytes()
    assert dr_res.tobytes() == dr_up.tobytes()
    # the plain restatement on the records of the first --sample-reads reads
    alns = res.alns[res.alns["qid"] < a.sample_reads]
    t0 = time.perf_counter()
    sigs = ref.signatures(alns, res.cigars, dict(min_support=a.min_support))
    ref.calls(sigs, dict(min_support=a.min_support))
    py_s = time.perf_counter() - t0
    ops_sample, ops_all = int(alns["n_cigar"].sum()), int(res.alns["n_cigar"].sum())
    out = {
        "workload": D["text"], "device": eng.device_name(), "preset": cfg["preset"], "options": {k: getattr(opt, k) for k, _ in InsOpt._fields_},
        "reads": int(D["total_reads"]), "read_bases": int(D["total_bases"]), "records": int(len(res.alns)), "cigar_words": int(len(res.cigars)),
        "cigar_words_of_records": ops_all, "signatures": int(len(ic_res.sigs)), "calls": int(len(ic_res.calls)),
        "call_insertions_ms_resident_cigars": {"min": min(ms_res), "median": float(np.median(ms_res)), "all": ms_res},
        "call_insertions_ms_uploaded_cigars": {"min": min(ms_up), "median": float(np.median(ms_up)), "all": ms_up},
        "genotype_options": {k: getattr(gopt, k) for k, _ in GenoOpt._fields_},
        "genotype_reference_reads": int(len(ig_res.ref_reads)), "genotype_ambiguous_reads": int(len(ig_res.ambig_reads)),
        "genotype_gt_counts": [int((ig_res.gt["gt"] == v).sum()) for v in (0, 1, 2)],
        "genotype_insertions_ms_resident_cigars": {"min": min(gms_res), "median": float(np.median(gms_res)), "all": gms_res},
        "genotype_insertions_ms_uploaded_cigars": {"min": min(gms_up), "median": float(np.median(gms_up)), "all": gms_up},
        "draft_options": {k: getattr(dopt, k) for k, _ in DraftOpt._fields_},
        "draft_calls_with_a_draft": int((dr_res["sig"] >= 0).sum()), "draft_bases": dr_bases,
        "draft_contigs_ms_resident_cigars": {"min": min(dms_res), "median": float(np.median(dms_res)), "all": dms_res},
        "draft_contigs_ms_uploaded_cigars": {"min": min(dms_up), "median": float(np.median(dms_up)), "all": dms_up},
        "python_restatement": {"sample_reads": a.sample_reads, "sample_cigar_words": ops_sample, "seconds": py_s,
                               "scaled_to_all_records_seconds": py_s * ops_all / max(1, ops_sample),
                               "note": "tests/inscall_ref.py, one CPU thread; scaled by CIGAR words"},
        "timing": "wall clock of Index.call_insertions (validation, record upload, kernels, the signatures and calls copied back) and of Index.genotype_insertions "
                  "(validation, uploads, kernels, the genotypes and read lists copied back) and of Index.draft_contigs (validation, uploads, kernels, the draft "
                  "records copied back, the set left on the device), %d repeats after one untimed call each" % a.repeat,
    }
    # (a site's support need not be its call's: a single-linkage cluster may reach farther than `reach` from its median position)
    assert len(sc_res.calls) == len(ic_res.calls)
    sites_out = {k: out[k] for k in ("workload", "device", "preset", "options", "reads", "records", "cigar_words", "signatures", "calls")}
    sites_out.update({
        "sites": int(len(sc_res.calls)), "site_options": {"reach": 50, "len_pct": 0}, "kept_signatures": int(len(sc_res.sigs)),
        "sites_with_support": int((sc_res.calls["support"] > 0).sum()),
        "sites_whose_support_is_the_calls": int((sc_res.calls["support"] == ic_res.calls["support"]).sum()),
        "call_insertions_ms_resident_cigars": out["call_insertions_ms_resident_cigars"],
        "call_at_sites_ms_resident_cigars": {"min": min(sms_res), "median": float(np.median(sms_res)), "all": sms_res},
        "timing": "wall clock of Index.call_at_sites on the positions of the run's own calls (validation, record and site upload, kernels, the kept "
                  "signatures and calls copied back), %d repeats after one untimed call, next to Index.call_insertions of the same run" % a.repeat,
    })
    os.makedirs(os.path.dirname(a.sites_out), exist_ok=True)
    with open(a.sites_out, "w") as fh:
        json.dump(sites_out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: sites_out[k] for k in ("sites", "kept_signatures", "sites_with_support", "call_insertions_ms_resident_cigars", "call_at_sites_ms_resident_cigars")}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("records", "cigar_words", "signatures", "calls", "call_insertions_ms_resident_cigars",
                                          "call_insertions_ms_uploaded_cigars", "genotype_insertions_ms_resident_cigars",
                                          "genotype_insertions_ms_uploaded_cigars", "draft_contigs_ms_resident_cigars",
                                          "draft_contigs_ms_uploaded_cigars", "python_restatement")}))


if __name__ == "__main__":
    main()
