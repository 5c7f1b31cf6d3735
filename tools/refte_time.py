"""Times the reference TE annotation (telr_te.annotate_reference) on the genome of synth.make_stage1_dataset -- the one
generator that reports the TE copies it plants (te_copies / te_copy_info: 5'-truncated copies, 0 - 15 % substitutions, either strand, over
15 % of a chr2L-sized genome) -- in its three steps: the tile set (Engine.tile_plan + SeqSet.pieces), the map of the tiles against the
library's index, the features (Engine.annotate_hits).  It also reports, against the planted copies binned by their divergence, the share
of copies at least half of whose bases a feature of the copy's family and strand covers (a copy that a later copy overwrites in part is
left out).  Nothing asserts these numbers.  Writes profiles/refte_time.json.

    python tools/refte_time.py [--genome-len 23513712] [--tile 32768] [--stride 16384] [--repeat 3] [--out profiles/refte_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = (0.0, 0.025, 0.05, 0.075, 0.10, 0.125, 0.15)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=23513712)
    ap.add_argument("--tile", type=int, default=32768)
    ap.add_argument("--stride", type=int, default=16384)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refte_time.json"))
    a = ap.parse_args()
    import numpy as np
    from telr_amd import synth
    D = synth.make_stage1_dataset(genome_len=a.genome_len, n_reads=2, total_bases=4000, n_ins=2)          # the reads are not used
    import torch  # noqa: F401
    from telr_amd.aligner import Engine
    from telr_amd.presets import preset
    from telr_amd._abi import MF_CIGAR
    eng = Engine(0)
    ref = D["ref"]
    lib = [bytes(x).decode() for x in D["library"]]
    tset = eng.seqset((ref, np.zeros(1, np.int64), np.array([len(ref)], np.int32)))
    io, mo = preset("map-ont")
    mo = mo.copy(); mo.bw_long = 0; mo.secondary = 0; mo.flags |= MF_CIGAR
    t_tiles, t_map, t_feat = [], [], []
    feats = None
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        tiles = eng.tile_plan(tset.len, a.tile, a.stride)
        q = tset.pieces(tiles["tid"], tiles["start"], tiles["len"])
        t1 = time.perf_counter()
        ix = eng.index(lib, io)
        r = ix.map_raw(q, mo)
        t2 = time.perf_counter()
        feats = eng.annotate_hits(r, tiles, tset.len, len(lib))
        t3 = time.perf_counter()
        n_rec = int(eng.L.telr_result_count(r))
        ix.free_raw(r); ix.free(); ix.targets.free(); q.free()
        t_tiles.append(t1 - t0); t_map.append(t2 - t1); t_feat.append(t3 - t2)
    med = lambda x: float(np.median(x[1:]))                        # the first pass sizes the context's scratch
    # the planted copies a feature covers: bases of the copy under features of its family and strand
    info = D["te_copy_info"]
    later = np.zeros(len(ref) + 1, np.int32)
    whole = []
    for k in range(len(info) - 1, -1, -1):                         # from the last copy back: a copy is whole iff no later copy touches it
        s, e = info[k][0], info[k][1]
        whole.append(not later[s:e].any())
        later[s:e] = 1
    whole.reverse()
    by = {}
    for f in feats:
        by.setdefault((int(f["family"]), int(f["strand"])), []).append((int(f["start"]), int(f["end"])))
    rows = []
    for b in range(len(BINS) - 1):
        n = hit = 0
        for (s, e, fam, strand, cut, div), w in zip(info, whole):
            if not w or not (BINS[b] <= div < BINS[b + 1]) or e - s < 100:
                continue
            n += 1
            cov = sum(max(0, min(e, fe) - max(s, fs)) for fs, fe in by.get((fam, strand), ()))
            hit += 2 * cov >= e - s
        rows.append(dict(divergence=[BINS[b], BINS[b + 1]], copies=n, covered=hit, share=(hit / n if n else None)))
    out = {
        "genome_bases": int(len(ref)), "library_sequences": len(lib), "planted_copies": len(info), "whole_copies": int(sum(whole)),
        "tile": a.tile, "stride": a.stride, "tiles": int(len(tiles)), "records": n_rec, "features": int(len(feats)), "device": eng.device_name(),
        "tile_set_s_median": med(t_tiles), "map_s_median": med(t_map), "features_s_median": med(t_feat),
        "tile_set_s_all": t_tiles[1:], "map_s_all": t_map[1:], "features_s_all": t_feat[1:],
        "covered_by_divergence": rows,
        "timing": "wall clock around the Python calls (each ends in a stream synchronisation); the map step includes the library's index build; "
                  "%d repeats after one untimed pass, same process, same resident reference" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("tiles", "records", "features", "tile_set_s_median", "map_s_median", "features_s_median", "covered_by_divergence")}))
    tset.free()


if __name__ == "__main__":
    main()
