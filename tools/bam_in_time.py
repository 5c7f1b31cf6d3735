"""Times Engine.load_bam (telr_bam_load) per phase -- host hop, upload, inflate, chain, parse, names on the host,
sequences -- on the BAM that telr_map + write_bam_device make of a BASELINE configs[2]-shaped read set (bench.py's data set:
--coverage / --genome-scale make it smaller), next to the times of that telr_map and that write_bam_device.  Checks that the loaded
records are the mapped ones (count, reads, CIGAR words).  Writes profiles/bam_in_time.json.

    python tools/bam_in_time.py [--coverage 30] [--genome-scale 1.0] [--repeat 3] [--level 1] [--bam /tmp/bam_in_time.bam] [--out profiles/bam_in_time.json]
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
    ap.add_argument("--coverage", type=float, default=0.0)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--bam", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_in_time.json"))
    a = ap.parse_args()
    import numpy as np
    import bench
    cfg = bench.CONFIGS["c2"]
    ba = argparse.Namespace(config="c2", genome_scale=a.genome_scale, insertions=0, coverage=a.coverage, scaling="strong")
    D = bench.build_dataset(ba, cfg, 0, 1, 1)                      # before the GPU is touched: the generator forks workers
    import torch  # noqa: F401
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
    tmp = None
    if a.bam is None:
        tmp = tempfile.mkdtemp(prefix="bam_in_time_")
        a.bam = os.path.join(tmp, "in.bam")
    t0 = time.perf_counter()
    r = ix.map_raw(qs, mo)
    map_ms = (time.perf_counter() - t0) * 1e3
    n_rec = int(eng.L.telr_result_count(r)); n_cig = int(ix.result_arrays(r).alns["n_cigar"].sum(dtype=np.int64))          # (the result's array may hold unreferenced words)
    t0 = time.perf_counter()
    ix.write_bam_device(r, qs, qn, tn, a.bam, level=a.level)
    write_ms = (time.perf_counter() - t0) * 1e3
    ix.bam_release_wait()
    ix.free_raw(r)
    runs = []
    for k in range(a.repeat + 1):
        t0 = time.perf_counter()
        bi = eng.load_bam(a.bam)
        wall = (time.perf_counter() - t0) * 1e3
        assert bi.counters["kept"] == n_rec and bi.counters["reads"] == qs.n and int(eng.L.telr_result_cigar_count(bi.result)) == n_cig, bi.counters
        runs.append(dict(bi.phase_ms, wall_python=wall))
        counters = bi.counters
        bi.free()
    runs = runs[1:]                                                # the first call sizes the context's scratch
    med = {k: float(np.median([x[k] for x in runs])) for k in runs[0]}
    size = os.path.getsize(a.bam)
    out = {
        "workload": D["text"], "device": eng.device_name(), "preset": cfg["preset"], "level": a.level,
        "reads": int(D["total_reads"]), "read_bases": int(D["total_bases"]), "records": n_rec, "cigar_words": n_cig,
        "bam_bytes": int(size), "counters": counters,
        "telr_map_ms": map_ms, "write_bam_device_ms": write_ms,
        "load_bam_ms_median": med, "load_bam_ms_all": runs,
        "chain_share_of_load": med["chain"] / max(med["total"], 1e-9),
        "timing": "wall clock inside telr_bam_load per phase (each phase ends with a stream synchronisation), %d repeats after one untimed call; "
                  "telr_map and write_bam_device are single calls on a fresh context" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("reads", "records", "bam_bytes", "telr_map_ms", "write_bam_device_ms", "load_bam_ms_median", "chain_share_of_load")}))
    if tmp:
        os.unlink(a.bam)
        for x in (a.bam + ".bai",):
            if os.path.exists(x):
                os.unlink(x)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
