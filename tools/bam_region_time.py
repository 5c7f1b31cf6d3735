"""Times Engine.load_bam(regions=...) (telr_bam_load_regions) next to the whole-file and the chunked load of the same
tree, on the BAM that telr_map + write_bam_device make of a BASELINE configs[2]-shaped read set (the file of tools/bam_in_time.py;
--coverage / --genome-scale make it smaller), with its .bai.  Legs: whole, chunked_auto, sites (one region [pos - m, pos + m) around
every insertion call of that run, m = the `--region sites` margin of telr_amd/telr.py), target (all of target 0).  Per leg: milliseconds
per phase, wall clock around the Python call (median of --repeat calls after one untimed call), members inflated of the members in the
file, file bytes uploaded, records walked and selected, and the number of the mapped result's records that overlap the leg's regions
(records_expected; a leg that selected another number prints MISMATCH).  Writes profiles/bam_region_time.json.

    python tools/bam_region_time.py [--coverage 15] [--genome-scale 1.0] [--repeat 3] [--out profiles/bam_region_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--legs", default="whole,chunked_auto,sites,target")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_region_time.json"))
    a = ap.parse_args()
    import numpy as np
    import bench
    cfg = bench.CONFIGS["c2"]
    ba = argparse.Namespace(config="c2", genome_scale=a.genome_scale, insertions=0, coverage=a.coverage, scaling="strong")
    D = bench.build_dataset(ba, cfg, 0, 1, 1)                      # before the GPU is touched: the generator forks workers
    import torch  # noqa: F401
    from telr_amd import telr
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    from telr_amd._abi import MF_KEEP_CIGARS
    eng = Engine(0)
    io, mo = preset(cfg["preset"])
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    ix = eng.index([bytes(r).decode() for r in D["ref"]], io)
    qs = eng.seqset(D["reads"])
    qn = ["r%d" % i for i in range(qs.n)]
    tn = ["chr%d" % i for i in range(ix.targets.n)]
    tmp = tempfile.mkdtemp(prefix="bam_region_time_")
    bam = os.path.join(tmp, "in.bam")
    r = ix.map_raw(qs, mo)
    ic = ix.call_insertions(r)
    m = telr.site_region_margin(argparse.Namespace(site_reach=50))
    tlens = [int(x) for x in ix.targets.len]
    res = ix.result_arrays(r)
    alns = res.alns.copy()
    regions = {"sites": [(int(c["tid"]), max(0, int(c["pos"]) - m), min(int(c["pos"]) + m, tlens[int(c["tid"])])) for c in ic.calls],
               "target": [(0, 0, tlens[0])]}
    ix.write_bam_device(r, qs, qn, tn, bam, level=a.level, index=True)
    ix.bam_release_wait()
    ix.free_raw(r)

    def overlapping(reg):
        """records of the mapped result whose [ts, te) overlaps a region (every record here has M or D bases)"""
        hit = np.zeros(len(alns), bool)
        for t, b, e in reg:
            hit |= (alns["tid"] == t) & (alns["ts"] < e) & (np.maximum(alns["te"], alns["ts"] + 1) > b)
        return int(hit.sum())
    members_in_file = None
    legs = {}
    for leg in a.legs.split(","):
        runs = []
        for k in range(a.repeat + 1):
            eng.release_scratch()
            t0 = time.perf_counter()
            if leg == "whole":
                bi = eng.load_bam(bam)
            elif leg == "chunked_auto":
                bi = eng.load_bam(bam, chunk_bytes=0)
            else:
                bi = eng.load_bam(bam, regions=regions[leg])
            wall = (time.perf_counter() - t0) * 1e3
            runs.append(dict(bi.phase_ms, wall_python=wall))
            counters, chunk_info, region_info, region_bytes = bi.counters, bi.chunk_info, bi.region_info, bi.region_bytes
            bi.free()
        if leg == "whole":
            members_in_file = counters["members"]
        expected = overlapping(regions[leg]) if leg in regions else counters["records"]
        if leg in regions and not counters["records"] == region_info["selected"] == expected:
            print("MISMATCH in leg %s: %r %r, %d records of the mapped result overlap" % (leg, counters, region_info, expected))
        runs = runs[1:]                                               # the first call is not timed
        legs[leg] = {"ms_median": {k: float(np.median([x[k] for x in runs])) for k in runs[0]}, "ms_all": runs, "counters": counters, "chunk_info": chunk_info,
                     "regions_given": len(regions.get(leg, [])), "records_expected": expected, "region_info": region_info, "members_inflated": counters["members"] + region_info["header_members"],
                     "members_in_file": members_in_file, "file_bytes_uploaded": region_bytes if leg in regions else os.path.getsize(bam) * (2 if chunk_info["chunks"] > 1 else 1)}
    out = {
        "workload": D["text"], "device": eng.device_name(), "preset": cfg["preset"], "level": a.level, "bam_bytes": int(os.path.getsize(bam)),
        "bai_bytes": int(os.path.getsize(bam + ".bai")), "calls": len(ic.calls), "site_margin": m, "legs": legs,
        "timing": "per leg %d repeats after one untimed call, the context's scratch released before every call; wall_python is the wall clock around "
                  "Engine.load_bam, the phases are those of telr_bam_in_phase_ms (host_hop of a region leg: reading the index, the plan and the hops of the "
                  "intervals; upload and inflate: device time of both passes, overlapping the rest when there is more than one chunk)" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    for leg, v in legs.items():
        print(leg, json.dumps({k: v[k] for k in ("ms_median", "region_info", "members_inflated", "members_in_file", "file_bytes_uploaded", "chunk_info")}))
    for x in (bam, bam + ".bai"):
        if os.path.exists(x):
            os.unlink(x)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
