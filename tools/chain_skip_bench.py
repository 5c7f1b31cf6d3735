"""telr_map with and without TELR_MF_CHAIN_SKIP (minimap2's chaining scan) on configs[2]-shaped reads (the dm6-size synthetic genome of
bench.py, ONT-like reads) and on the same genome made HARD (synth.HARD: tandem arrays, satellites, segmental duplications, error
bursts), presets map-ont and map-pb.  Per leg: Gbp/s of the whole call (median of --steps after one warm-up), stage_ms of `chain`
and `backtrack`, and how many records differ between the two modes.  One JSON line per leg, then a table.

usage: python tools/chain_skip_bench.py [--coverage 4] [--steps 3] [--out profiles/chain_skip_bench.json]"""
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
    ap.add_argument("--coverage", type=float, default=4.0, help="read coverage of the genome (configs[2]: 30; the modes scale alike)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)
    from telr_amd import synth
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    # every read set first: the generator forks worker processes, which must happen before the process touches the GPU
    legs = []
    for hard in (False, True):
        hd = synth.HARD if hard else None
        g = synth.make_genome(20261002, synth.DM6_ARMS, n_fam=127, n_ins=1000, threads=8, hard=hd)
        for pname, err in (("map-ont", (0.04, 0.02, 0.04)), ("map-pb", (0.013, 0.065, 0.052))):
            plan = synth.plan_reads(g, a.coverage)
            buf, off, ln, _ = synth.materialize_reads(g, plan, err=err, procs=8, burst=hd["burst"] if hd else None)
            legs.append((hard, pname, [bytes(x).decode() for x in g["ref"]], [buf[off[i]:off[i] + ln[i]] for i in range(len(ln))], ln))
    eng = Engine(0)
    rows = []
    for hard, pname, ref, reads, ln in legs:
        nb = int(ln.sum())
        io, _ = preset(pname)
        ix = eng.index(ref, io)
        qs = eng.seqset(reads)
        res = {}
        for skip in (False, True):
            _, mo = preset(pname, chain_skip=skip)
            ix.map(qs, mo)
            ts, ch, bt = [], [], []
            for _ in range(a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); r = ix.map(qs, mo); ts.append(time.perf_counter() - t0)
                sm = eng.stage_ms(); ch.append(sm.get("chain", 0.0)); bt.append(sm.get("backtrack", 0.0))
            res[skip] = (r, float(np.median(ts)), float(np.median(ch)), float(np.median(bt)))
        a0, a1 = res[False][0].alns, res[True][0].alns
        # records of the default run without an identical record (every field but the CIGAR offset, and the CIGAR) in the scan's run
        ndiff = sum((_records(res[False][0]) - _records(res[True][0])).values())
        row = dict(genome="hard" if hard else "configs[2]-shaped", preset=pname, reads=len(ln), gbp=nb / 1e9, records_default=len(a0),
                   records_skip=len(a1), records_differ=ndiff)
        for skip, tag in ((False, "default"), (True, "chain_skip")):
            _, dt, c, b = res[skip]
            row[tag] = dict(gbp_s=round(nb / dt / 1e9, 3), wall_ms=round(dt * 1e3, 1), chain_ms=round(c, 2), backtrack_ms=round(b, 2))
        row["chain_ratio"] = round(row["chain_skip"]["chain_ms"] / max(row["default"]["chain_ms"], 1e-6), 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
        qs.free(); ix.free()
    print("| genome | preset | Gbp | Gbp/s default | Gbp/s scan | chain ms default | chain ms scan | ratio | backtrack ms default | backtrack ms scan | records differ |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %.2f | %.2f | %.2f | %.1f | %.1f | %.2f | %.1f | %.1f | %d of %d |" % (
            r["genome"], r["preset"], r["gbp"], r["default"]["gbp_s"], r["chain_skip"]["gbp_s"], r["default"]["chain_ms"], r["chain_skip"]["chain_ms"],
            r["chain_ratio"], r["default"]["backtrack_ms"], r["chain_skip"]["backtrack_ms"], r["records_differ"], r["records_default"]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(coverage=a.coverage, steps=a.steps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
