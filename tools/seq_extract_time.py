"""Times SeqSet.extract (telr_seqset_extract) for 1,000 pieces of 8,000 bases of a BASELINE configs[2]-shaped read set
next to the route it replaces, in the same process: the whole set decoded to text as BamInput.reads() does it (telr_bam_in_ascii: decode
on the device, one copy of every base to the host), then the same pieces sliced out of that text (reverse-complemented on the host where
rc is set).  The set is the one Engine.load_bam makes of the BAM that telr_map + write_bam_device write for the data set of bench.py
(--coverage / --genome-scale make it smaller).  Checks that both routes give the same pieces.  Writes profiles/seq_extract_time.json.

    python tools/seq_extract_time.py [--coverage 30] [--genome-scale 1.0] [--pieces 1000] [--piece-len 8000] [--repeat 3] [--out profiles/seq_extract_time.json]
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
    ap.add_argument("--pieces", type=int, default=1000)
    ap.add_argument("--piece-len", type=int, default=8000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_extract_time.json"))
    a = ap.parse_args()
    import numpy as np
    import bench
    cfg = bench.CONFIGS["c2"]
    ba = argparse.Namespace(config="c2", genome_scale=a.genome_scale, insertions=0, coverage=a.coverage, scaling="strong")
    D = bench.build_dataset(ba, cfg, 0, 1, 1)                      # before the GPU is touched: the generator forks workers
    import torch  # noqa: F401
    from telr_amd.aligner import Engine
    from telr_amd.fasta import revcomp
    from telr_amd.presets import preset
    from telr_amd._abi import MF_KEEP_CIGARS
    eng = Engine(0)
    io, mo = preset(cfg["preset"])
    mo = mo.copy(); mo.flags |= MF_KEEP_CIGARS
    ix = eng.index([bytes(r).decode() for r in D["ref"]], io)
    qs = eng.seqset(D["reads"])
    tmp = tempfile.mkdtemp(prefix="seq_extract_time_")
    bam = os.path.join(tmp, "in.bam")
    r = ix.map_raw(qs, mo)
    ix.write_bam_device(r, qs, ["r%d" % i for i in range(qs.n)], ["chr%d" % i for i in range(ix.targets.n)], bam, level=1)
    ix.bam_release_wait()
    ix.free_raw(r); qs.free()
    bi = eng.load_bam(bam)
    rs = bi.read_set
    # the pieces: reads long enough, spread over the set, every other one reverse-complemented
    rng = np.random.RandomState(1)
    want = min(a.piece_len, int(rs.len.max()))
    long_enough = np.nonzero(rs.len >= want)[0]
    idx = long_enough[rng.randint(0, len(long_enough), a.pieces)].astype(np.int32)
    start = np.array([rng.randint(0, int(rs.len[i]) - want + 1) for i in idx], np.int32)
    ln = np.full(a.pieces, want, np.int32)
    rc = (np.arange(a.pieces) & 1).astype(np.uint8)
    ext, dec, sli = [], [], []
    for k in range(a.repeat + 1):
        t0 = time.perf_counter()
        got = rs.extract(idx, start, ln, rc)
        ext.append((time.perf_counter() - t0) * 1e3)
        bi._reads = None                                           # reads() keeps its product: decode again
        t0 = time.perf_counter()
        buf, off, _ = bi.reads()
        t1 = time.perf_counter()
        old = []
        for i, s, l, c in zip(idx, start, ln, rc):
            p = buf[int(off[i]) + int(s):int(off[i]) + int(s) + int(l)].tobytes()
            old.append(revcomp(p) if c else p)
        t2 = time.perf_counter()
        dec.append((t1 - t0) * 1e3); sli.append((t2 - t1) * 1e3)
        assert got == old, "the two routes disagree"
    med = lambda x: float(np.median(x[1:]))                        # the first call sizes the context's scratch
    out = {
        "workload": D["text"], "device": eng.device_name(), "reads": int(rs.n), "read_bases": int(rs.len.sum(dtype=np.int64)),
        "pieces": int(a.pieces), "piece_len": int(want), "piece_bytes": int(ln.sum(dtype=np.int64)),
        "extract_ms_median": med(ext), "extract_ms_all": ext[1:],
        "decode_whole_set_ms_median": med(dec), "slice_ms_median": med(sli), "decode_then_slice_ms_median": med(dec) + med(sli),
        "decode_whole_set_ms_all": dec[1:], "slice_ms_all": sli[1:],
        "timing": "wall clock around SeqSet.extract and around BamInput.reads() + the host slicing, %d repeats after one untimed call, same process, "
                  "same resident set" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("reads", "read_bases", "piece_bytes", "extract_ms_median", "decode_whole_set_ms_median", "slice_ms_median")}))
    bi.free()
    for x in (bam, bam + ".bai"):
        if os.path.exists(x):
            os.unlink(x)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
