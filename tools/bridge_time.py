"""Measures what the bridge step (telr_bridge_contigs + telr_seqset_join) does on a stage-1 result of BASELINE configs[2]
shape (bench.py's data set: --coverage / --genome-scale make it smaller): how many planted insertions have no spanning read (the
generator knows every read's origin), how many calls the caller gains with min_sized = 0, how many of the calls without a draft get a
bridge, and the wall time of Index.bridge_contigs and SeqSet.join on the result's resident CIGAR copy.  Nothing here is asserted by a
test.  Writes profiles/bridge_time.json.

    python tools/bridge_time.py [--coverage 30] [--genome-scale 1.0] [--repeat 5] [--margin 500] [--out profiles/bridge_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spanning_truth(g, plan, margin):
    """per planted insertion: on how many of its haplotype copies does NO read run from `margin` bases before the element to `margin`
    bases behind it -> (insertions, copies, copies without a spanning read, insertions without one on ANY copy)"""
    import numpy as np
    from telr_amd import synth
    n_copies = n_copy_unspanned = n_ins_unspanned = 0
    key = plan["hap"].astype(np.int64) * len(g["ref"]) + plan["chrom"]
    order = np.argsort(key, kind="stable")
    starts = {}
    for h in range(synth.N_HAP):
        for ci in range(len(g["ref"])):
            m = order[np.searchsorted(key[order], h * len(g["ref"]) + ci, "left"):np.searchsorted(key[order], h * len(g["ref"]) + ci, "right")]
            starts[(h, ci)] = (plan["start"][m], plan["start"][m] + plan["length"][m])
    for (c, p, fam, strand, tsd, af) in g["insertions"]:
        spanned_somewhere = False
        for h in range(int(round(af * synth.N_HAP))):
            pos, shift = g["hap_ins"][h][c]
            k = int(np.searchsorted(pos, p))
            he = p + int(shift[k])                          # the element's end on the haplotype (make_genome: ref[.. p + tsd], element, ref[p ..])
            hs = he - len(g["library"][fam])
            s, e = starts[(h, c)]
            ok = bool(((s <= hs - margin) & (e >= he + margin)).any())
            n_copies += 1
            n_copy_unspanned += 0 if ok else 1
            spanned_somewhere |= ok
        n_ins_unspanned += 0 if spanned_somewhere else 1
    return len(g["insertions"]), n_copies, n_copy_unspanned, n_ins_unspanned


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", type=float, default=0.0)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--margin", type=int, default=500, help="bases of flank a spanning read needs on either side (the draft's min_flank)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridge_time.json"))
    a = ap.parse_args()
    import numpy as np
    import bench
    from telr_amd import synth
    cfg = bench.CONFIGS["c2"]
    ba = argparse.Namespace(config="c2", genome_scale=a.genome_scale, insertions=0, coverage=a.coverage, scaling="strong")
    seen = {}
    make_genome, plan_reads = synth.make_genome, synth.plan_reads          # the data set's own genome and read plan, as bench.py makes them
    synth.make_genome = lambda *x, **k: seen.setdefault("g", make_genome(*x, **k))
    synth.plan_reads = lambda *x, **k: seen.setdefault("plan", plan_reads(*x, **k))
    try:
        D = bench.build_dataset(ba, cfg, 0, 1, 1)                  # before the GPU is touched: the generator forks workers
    finally:
        synth.make_genome, synth.plan_reads = make_genome, plan_reads
    n_ins, n_copies, copies_unspanned, ins_unspanned = spanning_truth(seen["g"], seen["plan"], a.margin)
    import torch  # noqa: F401
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    from telr_amd._abi import InsOpt, BridgeOpt, MF_KEEP_CIGARS
    eng = Engine(0)
    io, mo = preset(cfg["preset"])
    ix = eng.index([bytes(r).decode() for r in D["ref"]], io)
    qs = eng.seqset(D["reads"])
    mk = mo.copy(); mk.flags |= MF_KEEP_CIGARS
    r = ix.map_raw(qs, mk)
    ic_default = ix.call_insertions(r)
    ic = ix.call_insertions(r, InsOpt.default(min_sized=0))
    drafts, dset = ix.draft_contigs(r, ic, qs)
    dset.free()
    want = drafts["sig"] < 0
    bopt = BridgeOpt.default()
    ts = []
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        br = ix.bridge_contigs(r, ic, qs, bopt, want)
        ts.append((time.perf_counter() - t0) * 1e3)
    have = br[br["sig_l"] >= 0]
    off = np.arange(len(have) + 1, dtype=np.int64) * 2
    inter = lambda x, y: np.stack([have[x], have[y]], 1).ravel()
    js = []
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        s = qs.join(off, inter("qid_l", "qid_r"), inter("start_l", "start_r"), inter("len_l", "len_r"), inter("rc_l", "rc_r"))
        js.append((time.perf_counter() - t0) * 1e3)
        bases = int(s.len.sum())
        s.free()
    ix.free_raw(r)
    sized0 = ic.calls["n_sized"] == 0
    out = {
        "workload": D["text"], "device": eng.device_name(), "preset": cfg["preset"], "bridge_options": {k: getattr(bopt, k) for k, _ in BridgeOpt._fields_},
        "reads": int(D["total_reads"]), "planted_insertions": n_ins, "planted_copies_on_haplotypes": n_copies, "spanning_margin": a.margin,
        "copies_without_a_spanning_read": copies_unspanned, "insertions_without_a_spanning_read_on_any_copy": ins_unspanned,
        "calls_default": int(len(ic_default.calls)), "calls_min_sized_0": int(len(ic.calls)), "calls_gained": int(len(ic.calls) - len(ic_default.calls)),
        "calls_without_a_sized_read": int(sized0.sum()), "calls_without_a_draft": int(want.sum()),
        "calls_with_both_sides": int(((br["n_left"] > 0) & (br["n_right"] > 0) & want).sum()), "calls_bridged": int(len(have)),
        "bridged_votes": {"min": int(have["votes"].min()) if len(have) else 0, "median": float(np.median(have["votes"])) if len(have) else 0.0,
                          "max": int(have["votes"].max()) if len(have) else 0},
        "bridge_contigs_ms_resident_cigars": {"min": min(ts[1:]), "median": float(np.median(ts[1:])), "all": ts[1:]},
        "join_bases": bases, "join_ms": {"min": min(js[1:]), "median": float(np.median(js[1:])), "all": js[1:]},
        "timing": "wall clock of Index.bridge_contigs (validation, uploads, kernels, the records copied back) on the calls without a draft and of "
                  "SeqSet.join of the bridged calls' two pieces (the set left on the device), %d repeats after one untimed call each" % a.repeat,
        "note": "recall on real elements is not measured: the planted elements are random library sequences, and whether a bridged contig is the "
                "true haplotype is not checked here",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("workload", "timing", "note")}))


if __name__ == "__main__":
    main()
