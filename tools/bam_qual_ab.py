#!/usr/bin/env python3
"""What base qualities in QUAL cost the device BAM writer: file size (bytes per read base at level 1) and the writer's phases
(Index.bam_stage_ms), with and without attached qualities, on the stage1_to_sorted_bam input of `bench.py --full` (the same
seeded data set: bench.build_dataset with bench.py's own defaults).

One process measures ONE mode (the writer's buffers, the file mapping and the HIP runtime's state are per process); run it once
per mode with the same --data-cache and compare the JSON lines:

    python tools/bam_qual_ab.py --data-cache DIR --mode plain  --out plain.json
    python tools/bam_qual_ab.py --data-cache DIR --mode qual   --out qual.json
    TELR_LIB=/path/to/another/libtelrhip.so python tools/bam_qual_ab.py --data-cache DIR --mode plain --out other.json

The plain mode uses nothing a build without the option lacks, so the script also runs inside a checkout of an earlier commit
(copy it there): that is how the default path is held to its earlier time and the file to its earlier bytes (`sha256`).

Qualities: the reads of the data set carry none, so they are drawn here -- Phred = Binomial(40, 0.3) (mean 12, s.d. 2.9, values
0..40: the peaked shape of an ONT read's qualities, entropy 3.6 bits), from a seeded pool of 2^26 draws repeated over the read
set.  The writer's matching is run-length only, so the repetition of the pool (64 MB apart) is invisible to it.

Every pass is what bench.py's BAM leg times: bam_prepare -> telr_map -> telr_write_bam_dev; the first pass sizes and pins the
writer's buffers and is reported apart; the phases are the median over the --repeats passes that follow, with min and max, and
`spread` = (max - min) / median of the writer's total."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "qual"], required=True)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--coverage", type=float, default=0.0, help="override the configuration's coverage (0 = bench.py's)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--data-cache", default="")
    ap.add_argument("--bam-dir", default="/dev/shm")
    ap.add_argument("--keep", default="", help="keep the last BAM at this path")
    ap.add_argument("--out", default="")
    o = ap.parse_args()
    import numpy as np
    import bench
    a = bench.parse(["--config", o.config] + (["--coverage", str(o.coverage)] if o.coverage else []))
    cfg = bench.CONFIGS[a.config]
    cache = ""
    if o.data_cache:
        os.makedirs(o.data_cache, exist_ok=True)
        cache = os.path.join(o.data_cache, "bam_qual_ab_%s_%g.npz" % (a.config, a.coverage))
    t0 = time.time()
    if cache and os.path.exists(cache):
        D = bench.load_dataset(cache)
    else:
        D = bench.build_dataset(a, cfg, 0, 1, 1)          # CPU only; forks workers: before any GPU initialisation
        if cache:
            bench.save_dataset(cache, D)
    t_data = time.time() - t0
    import torch  # noqa: F401  (first: the process binds to its HIP runtime)
    from telr_amd.aligner import Engine, Index
    from telr_amd.presets import preset
    from telr_amd._abi import MF_KEEP_CIGARS
    buf, off, ln = D["reads"]
    n_bases = int(np.asarray(ln, np.int64).sum())
    io, mo = preset(cfg["preset"])
    mo.flags |= MF_KEEP_CIGARS
    eng = Engine(0)
    ix = eng.index([bytes(r).decode() for r in D["ref"]], io)
    t0 = time.time()
    qs = eng.seqset(D["reads"])
    t_upload = time.time() - t0
    t_attach = None
    if o.mode == "qual":
        pool = (np.random.default_rng(20261002).binomial(40, 0.3, 1 << 26) + 33).astype(np.uint8)
        qbuf = np.resize(pool, len(buf))          # the quality of base i of the read buffer: same offsets as the bases
        t0 = time.time()
        qs.attach_qual((qbuf, np.asarray(off, np.int64)))
        t_attach = time.time() - t0
        assert qs.has_qual
    qnames = Index._cstr_array(["read%d" % g for g in D["read_gid"]])
    bam_dir = o.bam_dir if os.path.isdir(o.bam_dir) and os.access(o.bam_dir, os.W_OK) else "/tmp"
    path = os.path.join(bam_dir, "bam_qual_ab_%s_%d.bam" % (o.mode, os.getpid()))
    est = (0.95 if o.level else 2.9) + (0.85 if o.mode == "qual" else 0.0)
    passes = []
    for rep in range(1 + o.repeats):
        for f in (path, path + ".bai"):
            if os.path.exists(f):
                os.unlink(f)
        ix.bam_release_wait()
        t0 = time.time()
        ix.bam_prepare(path, int(est * n_bases) + (64 << 20))
        r = ix.map_raw(qs, mo)
        t_map = time.time() - t0
        ix.write_bam_device(r, qs, qnames, D["names"], path, md=True, cs=True, softclip=True, cmdline="bench", index=True, level=o.level)
        t_all = time.time() - t0
        ix.free_raw(r)
        st = ix.bam_stage_ms()
        st["wall_map_s"] = t_map; st["wall_bam_s"] = t_all - t_map
        passes.append(st)
    size = os.path.getsize(path)
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(64 << 20), b""):
            h.update(blk)
    if o.keep:
        os.replace(path, o.keep)
        if os.path.exists(path + ".bai"):
            os.replace(path + ".bai", o.keep + ".bai")
    else:
        for f in (path, path + ".bai"):
            if os.path.exists(f):
                os.unlink(f)
    keys = ("upload", "scan_size", "sort_offsets", "write_records", "bgzf", "d2h_file", "total", "sink_mapping_used", "wall_bam_s")
    timed = passes[1:]
    med = {k: float(np.median([p[k] for p in timed])) for k in keys}
    lo = {k: float(min(p[k] for p in timed)) for k in keys}
    hi = {k: float(max(p[k] for p in timed)) for k in keys}
    out = dict(mode=o.mode, library=os.environ.get("TELR_LIB", "in-tree"), device=eng.device_name(), config=a.config, coverage=a.coverage or cfg.get("coverage"), level=o.level,
               read_bases=n_bases, reads=int(len(ln)), bam_bytes=size, bytes_per_read_base=size / n_bases, sha256=h.hexdigest(),
               qualities="Binomial(40, 0.3) Phred, seeded pool of 2^26 draws" if o.mode == "qual" else None,
               repeats=o.repeats, bam_stage_ms_median=med, bam_stage_ms_min=lo, bam_stage_ms_max=hi,
               spread_of_total=(hi["total"] - lo["total"]) / med["total"] if med["total"] else None,
               first_pass_ms=passes[0], dataset_s=t_data, pack_upload_s=t_upload, attach_qual_s=t_attach,
               note="write_records is the host's time to enqueue k_bam_write at level >= 1 (the kernel overlaps the coder: see the kernel trace); bgzf + d2h_file hold the device's and the copy-out's time")
    line = json.dumps(out)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
