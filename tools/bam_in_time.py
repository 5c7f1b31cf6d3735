"""Times Engine.load_bam (telr_bam_load and telr_bam_load_chunked) per phase -- host hop, upload, inflate, chain, parse,
names on the host, sequences -- and samples its peak device memory, leg by leg (the whole file at once, in chunks of the engine's own
size, in chunks of 256 MB), on the BAM that telr_map + write_bam_device make of a BASELINE configs[2]-shaped read set (bench.py's data set:
--coverage / --genome-scale make it smaller), next to the times of that telr_map and that write_bam_device.  Checks that the loaded
records are the mapped ones (count, reads, CIGAR words).  Writes profiles/bam_in_time.json.

    python tools/bam_in_time.py [--coverage 30] [--genome-scale 1.0] [--repeat 3] [--level 1] [--legs whole,chunked_auto,chunked_256MB] [--bam /tmp/bam_in_time.bam] [--out profiles/bam_in_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import threading
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
    ap.add_argument("--legs", default="whole,chunked_auto,chunked_256MB", help="whole, chunked_auto (the engine's own chunk size), chunked_<N>MB")
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
    legs = {}
    for leg in a.legs.split(","):
        chunk_bytes = {"whole": None, "chunked_auto": 0}.get(leg, None if not leg.startswith("chunked_") or leg == "chunked_auto" else int(leg[8:-2]) << 20)
        runs, peaks = [], []
        for k in range(a.repeat + 1):
            eng.release_scratch()                                      # every call sizes its scratch anew: the peak is this leg's own
            free0 = eng.mem_info()[0]
            low = [free0]
            stop = threading.Event()

            def sample():
                while not stop.is_set():
                    low[0] = min(low[0], eng.mem_info()[0])
                    time.sleep(0.002)
            th = threading.Thread(target=sample)
            th.start()
            t0 = time.perf_counter()
            bi = eng.load_bam(a.bam) if chunk_bytes is None else eng.load_bam(a.bam, chunk_bytes=chunk_bytes)
            wall = (time.perf_counter() - t0) * 1e3
            stop.set(); th.join()
            low[0] = min(low[0], eng.mem_info()[0])
            assert bi.counters["kept"] == n_rec and bi.counters["reads"] == qs.n and int(eng.L.telr_result_cigar_count(bi.result)) == n_cig, bi.counters
            runs.append(dict(bi.phase_ms, wall_python=wall))
            peaks.append(int(free0 - low[0]))
            counters, info = bi.counters, getattr(bi, "chunk_info", None)
            bi.free()
        runs, peaks = runs[1:], peaks[1:]                              # the first call is not timed
        med = {k: float(np.median([x[k] for x in runs])) for k in runs[0]}
        tot = [x["total"] for x in runs]
        legs[leg] = {"ms_median": med, "ms_all": runs, "total_ms_spread": [min(tot), max(tot)], "peak_device_bytes": int(max(peaks)), "chunk_info": info}
    med = legs[a.legs.split(",")[0]]["ms_median"]
    size = os.path.getsize(a.bam)
    out = {
        "workload": D["text"], "device": eng.device_name(), "preset": cfg["preset"], "level": a.level,
        "reads": int(D["total_reads"]), "read_bases": int(D["total_bases"]), "records": n_rec, "cigar_words": n_cig,
        "bam_bytes": int(size), "counters": counters,
        "telr_map_ms": map_ms, "write_bam_device_ms": write_ms,
        "legs": legs,
        "chain_share_of_load": med["chain"] / max(med["total"], 1e-9),
        "timing": "per leg %d repeats after one untimed call, the context's scratch released before every call.  whole: the load of one chunk -- upload, "
                  "inflate and chain are device times between events, parse, names and sequences host wall clock, nothing is inflated twice.  chunked_*: sums over "
                  "the chunks -- upload and inflate are device times of both "
                  "passes on the second stream and overlap with the rest, chain is device time, parse the host time of pass 1 behind the chain, sequences "
                  "the whole second pass; total is wall clock and not the sum of the others.  peak_device_bytes: free device memory (telr_device_mem) before "
                  "the call minus its minimum during the call, sampled every 2 ms by a host thread; the result and the set are part of it.  telr_map and "
                  "write_bam_device are single calls on a fresh context" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("reads", "records", "bam_bytes", "telr_map_ms", "write_bam_device_ms", "chain_share_of_load")}))
    for leg, v in legs.items():
        print(leg, json.dumps({"ms_median": v["ms_median"], "total_ms_spread": v["total_ms_spread"], "peak_device_bytes": v["peak_device_bytes"], "chunk_info": v["chunk_info"]}))
    if tmp:
        os.unlink(a.bam)
        for x in (a.bam + ".bai",):
            if os.path.exists(x):
                os.unlink(x)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
