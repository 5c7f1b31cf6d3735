"""telr_map with and without TELR_MF_SEED_RESCUE (minimap2's high-occurrence seed rescue) on configs[2]-shaped reads (the dm6-size
synthetic genome of bench.py): ONT-like reads with map-ont and ngmlr-ont, where nothing is expected to be rescued (the price of the pass
alone), and near-exact reads (0.4 % substitutions, 0.05 % insertions and deletions) with map-ont and asm10, where the rule fires.
Per leg: Gbp/s of the whole call (median of --steps after one warm-up), stage_ms of `seed` and `sort`, the anchors of the call and
how many records differ between the two modes.  One JSON line per leg, then a table.

usage: python tools/seed_rescue_bench.py [--coverage 2] [--steps 3] [--out profiles/seed_rescue_bench.json]"""
import argparse
import collections
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def _records(r):
    fl = [n for n in r.alns.dtype.names if n != "cigar_off"]
    return collections.Counter((tuple(int(x[n]) for n in fl), r.cigar(i).tobytes()) for i, x in enumerate(r.alns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", type=float, default=2.0, help="read coverage of the genome (configs[2]: 30; the modes scale alike)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)
    from telr_amd import synth
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    # every read set first: the generator forks worker processes, which must happen before the process touches the GPU
    g = synth.make_genome(20261002, synth.DM6_ARMS, n_fam=127, n_ins=1000, threads=8)
    ref = [bytes(x).decode() for x in g["ref"]]
    legs = []
    for reads_name, err, presets in (("ONT-like", (0.04, 0.02, 0.04), ("map-ont", "ngmlr-ont")), ("near-exact", (0.004, 0.0005, 0.0005), ("map-ont", "asm10"))):
        plan = synth.plan_reads(g, a.coverage)
        buf, off, ln, _ = synth.materialize_reads(g, plan, err=err, procs=8)
        reads = [buf[off[i]:off[i] + ln[i]] for i in range(len(ln))]
        for pname in presets:
            legs.append((reads_name, pname, reads, ln))
    eng = Engine(0)
    rows = []
    for reads_name, pname, reads, ln in legs:
        nb = int(ln.sum())
        io, _ = preset(pname)
        ix = eng.index(ref, io)
        qs = eng.seqset(reads)
        res = {}
        for on in (False, True):
            _, mo = preset(pname, seed_rescue=on)
            ix.map(qs, mo)
            ts, sd, so = [], [], []
            for _ in range(a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); r = ix.map(qs, mo); ts.append(time.perf_counter() - t0)
                sm = eng.stage_ms(); sd.append(sm.get("seed", 0.0)); so.append(sm.get("sort", 0.0))
            res[on] = (r, float(np.median(ts)), float(np.median(sd)), float(np.median(so)), int(eng.counters()["anchors"]))
        ndiff = sum((_records(res[False][0]) - _records(res[True][0])).values())
        row = dict(reads=reads_name, preset=pname, n_reads=len(ln), gbp=nb / 1e9, records_default=len(res[False][0].alns),
                   records_rescue=len(res[True][0].alns), records_differ=ndiff)
        for on, tag in ((False, "default"), (True, "seed_rescue")):
            _, dt, s, o, na = res[on]
            row[tag] = dict(gbp_s=round(nb / dt / 1e9, 3), wall_ms=round(dt * 1e3, 1), seed_ms=round(s, 2), sort_ms=round(o, 2), anchors=na)
        print(json.dumps(row), flush=True)
        rows.append(row)
        qs.free(); ix.free()
    print("| reads | preset | Gbp | Gbp/s default | Gbp/s rescue | seed ms default | seed ms rescue | sort ms default | sort ms rescue | anchors default | anchors rescue | records differ |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        d, s = r["default"], r["seed_rescue"]
        print("| %s | %s | %.2f | %.2f | %.2f | %.1f | %.1f | %.1f | %.1f | %d | %d | %d of %d |" % (
            r["reads"], r["preset"], r["gbp"], d["gbp_s"], s["gbp_s"], d["seed_ms"], s["seed_ms"], d["sort_ms"], s["sort_ms"], d["anchors"], s["anchors"],
            r["records_differ"], r["records_default"]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(coverage=a.coverage, steps=a.steps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
