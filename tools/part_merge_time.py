"""Times the multi-part index on a configs[1]-shaped read set (synth.make_stage1_dataset: a chr2L-sized genome, ONT-like
reads): the genome is cut into eight equal targets, and the same reads are mapped against ONE index over them (telr_map) and against a
PartIndex forced into 2 and 4 parts -- the map of every part, and the phases of telr_merge_parts (checks, upload, select, scans,
the allocation of the result's arrays, gather, host assembly, the mirror copy; TELR_TRACE=merge separates the device phases by stream waits).  It also reports how many records
each route returns.  Nothing asserts these numbers.  Writes profiles/part_merge_time.json.

    python tools/part_merge_time.py [--genome-len 23513712] [--reads 10000] [--bases 470000000] [--repeat 3] [--out profiles/part_merge_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TELR_TRACE"] = ",".join(x for x in (os.environ.get("TELR_TRACE"), "merge") if x)

PHASES = ("checks", "upload", "select", "scans", "gather", "assemble_host", "mirror", "total", "alloc_result")
N_TARGETS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=23513712)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--bases", type=int, default=470_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_merge_time.json"))
    a = ap.parse_args()
    import numpy as np
    from telr_amd import synth
    D = synth.make_stage1_dataset(genome_len=a.genome_len, n_reads=a.reads, total_bases=a.bases)
    import torch  # noqa: F401
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    from telr_amd._abi import MF_CIGAR, MF_KEEP_CIGARS
    eng = Engine(0)
    ref = D["ref"]
    cut = [len(ref) * k // N_TARGETS for k in range(N_TARGETS + 1)]
    tlen = np.array([cut[k + 1] - cut[k] for k in range(N_TARGETS)], np.int32)
    tset = eng.seqset((ref, np.array(cut[:-1], np.int64), tlen))
    qset = eng.seqset(D["reads"])
    io, mo = preset("map-ont")
    mo = mo.copy(); mo.flags |= MF_CIGAR | MF_KEEP_CIGARS
    med = lambda x: float(np.median(x[1:] if len(x) > 1 else x))          # the first pass sizes the context's scratch
    # the extent of one target (all are equal to within a base): k of them per part
    ext1 = (int(tlen.max()) + 16384 + 63) & ~63
    rows = {}
    ix = eng.index(tset, io)
    t = []
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        r = ix.map_raw(qset, mo)
        t.append(time.perf_counter() - t0)
        n_whole = int(eng.L.telr_result_count(r))
        ix.free_raw(r)
    ix.free()
    rows["unsplit"] = dict(map_ms=1e3 * med(t), records=n_whole)
    for n_parts in (2, 4):
        per = N_TARGETS // n_parts
        pix = eng.index_parts(tset, io, max_part_bases=per * ext1 + 1)
        assert pix.n_parts == n_parts, (pix.n_parts, n_parts)
        t_map, t_merge, ph = [], [], []
        for _ in range(a.repeat + 1):
            raws, tm = [], []
            for part in pix.parts:
                t0 = time.perf_counter()
                raws.append(part.map_raw(qset, mo))
                tm.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r = pix.merge_raw(raws, qset.n, mo)
            t_merge.append(time.perf_counter() - t0)
            p = np.zeros(len(PHASES), np.float32)
            eng.L.telr_debug_merge_ms(p.ctypes.data)
            ph.append(p); t_map.append(tm)
            pooled = sum(int(eng.L.telr_result_count(x)) for x in raws)
            n_rec, n_words = int(eng.L.telr_result_count(r)), int(eng.L.telr_result_cigar_count(r))
            for x in raws + [r]:
                pix.free_raw(x)
        pix.free()
        tm = np.array(t_map[1:] if len(t_map) > 1 else t_map); php = np.array(ph[1:] if len(ph) > 1 else ph)
        rows["%d parts" % n_parts] = dict(map_ms_per_part=[float(x) for x in 1e3 * np.median(tm, axis=0)], map_ms=float(1e3 * np.median(tm.sum(axis=1))),
                                          merge_ms=1e3 * med(t_merge), merge_phase_ms=dict(zip(PHASES, (float(x) for x in np.median(php, axis=0)))),
                                          pooled_records=pooled, records=n_rec, cigar_words=n_words)
    out = dict(device=eng.device_name(), genome_len=int(len(ref)), targets=N_TARGETS, reads=int(qset.n), read_bases=int(qset.bases()), preset="map-ont",
               repeat=a.repeat, rows=rows)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
