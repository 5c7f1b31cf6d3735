"""Times Engine.load_reads (telr_reads_load) on a BASELINE configs[2]-shaped read set written as FASTQ -- gzip at levels 1
and 6, and BGZF -- next to the route it replaces for the same file, fasta.read_fasta(with_qual=True) + Engine.seqset, in the same session,
and next to the plain file through fasta.load + Engine.seqset for scale.  --coverage makes the set a stated fraction of configs[2] (writing
30x as gzip in Python takes longer than the measurement is worth).  Per leg: one untimed load, then --repeat timed ones, the context's
scratch released before each; the median and the spread, the loader's phase columns, and the peak device memory sampled by a host thread.
Writes profiles/reads_in_time.json.

    python tools/reads_in_time.py [--coverage 5] [--repeat 3] [--dir /tmp] [--out profiles/reads_in_time.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import threading
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", type=float, default=5.0)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_in_time.json"))
    a = ap.parse_args()
    import numpy as np
    import bench
    import bam_in_ref as B
    cfg = bench.CONFIGS["c2"]
    ba = argparse.Namespace(config="c2", genome_scale=a.genome_scale, insertions=0, coverage=a.coverage, scaling="strong")
    D = bench.build_dataset(ba, cfg, 0, 1, 1)                      # before the GPU is touched: the generator forks workers
    buf, off, ln = D["reads"]
    tmp = tempfile.mkdtemp(prefix="reads_in_time_", dir=a.dir)
    # the FASTQ text: ONT-shaped qualities (seeded), one line per read
    rng = np.random.default_rng(20261020)
    parts = []
    for i in range(len(ln)):
        s = buf[int(off[i]):int(off[i]) + int(ln[i])].tobytes()
        q = (rng.integers(2, 41, int(ln[i]), dtype=np.uint8) + 33).tobytes()
        parts.append(b"@r%d\n%s\n+\n%s\n" % (i, s, q))
    text = b"".join(parts)
    del parts
    files = {"plain": os.path.join(tmp, "reads.fastq"), "gzip1": os.path.join(tmp, "reads.l1.fastq.gz"), "gzip6": os.path.join(tmp, "reads.l6.fastq.gz"),
             "bgzf": os.path.join(tmp, "reads.bgzf.fastq.gz")}
    t_write = {}
    t0 = time.perf_counter(); open(files["plain"], "wb").write(text); t_write["plain"] = time.perf_counter() - t0
    for k, lv in (("gzip1", 1), ("gzip6", 6)):
        t0 = time.perf_counter()
        with open(files[k], "wb") as f:
            c = zlib.compressobj(lv, zlib.DEFLATED, 31)
            for p in range(0, len(text), 1 << 24):
                f.write(c.compress(text[p:p + (1 << 24)]))
            f.write(c.flush())
        t_write[k] = time.perf_counter() - t0
    t0 = time.perf_counter()
    with open(files["bgzf"], "wb") as f:
        for p in range(0, len(text), 65280):
            raw = text[p:p + 65280]
            f.write(B.member(B.deflate_raw(raw, 6), raw))
        f.write(B.EOF_MARKER)
    t_write["bgzf"] = time.perf_counter() - t0
    n_text = len(text)
    del text
    import torch  # noqa: F401
    from telr_amd import fasta
    from telr_amd.aligner import Engine
    eng = Engine(0)

    def timed(fn):
        """-> (wall ms of every run, peak device bytes, what the last run returned through `keep`)"""
        walls, peaks, last = [], [], None
        for k in range(a.repeat + 1):
            eng.release_scratch()
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
            last = fn()
            walls.append((time.perf_counter() - t0) * 1e3)
            stop.set(); th.join()
            low[0] = min(low[0], eng.mem_info()[0])
            peaks.append(int(free0 - low[0]))
        return walls[1:], int(max(peaks[1:])), last

    def summary(walls, peak, extra=None):
        d = {"wall_ms_median": float(np.median(walls)), "wall_ms_spread": [min(walls), max(walls)], "wall_ms_all": walls, "peak_device_bytes": peak}
        d.update(extra or {})
        return d
    legs = {}

    def parent_route(path):
        names, seqs, quals = fasta.read_fasta(path, with_qual=True)
        s = eng.seqset(seqs, qual=quals)
        n = (s.n, s.bases())
        s.free()
        return n

    def device_route(path, keep_qual):
        ri = eng.load_reads(path, keep_qual=keep_qual)
        out = (ri.read_set.n, ri.n_bases, dict(ri.phase_ms), dict(ri.chunk_info), dict(ri.counters))
        ri.read_set.free(); ri.free()
        return out

    def plain_route(path):
        f = fasta.load(path)
        s = eng.seqset(f.triple, qual=f.qual)
        n = (s.n, s.bases())
        s.free(); f.close()
        return n
    want = (len(ln), int(ln.sum(dtype=np.int64)))
    for k in ("gzip1", "gzip6", "bgzf"):
        w, pk, got = timed(lambda: parent_route(files[k]))
        assert got == want, got
        legs[k + "_parent_read_fasta_seqset"] = summary(w, pk)
        for kq in (True, False):
            w, pk, got = timed(lambda: device_route(files[k], kq))
            assert got[:2] == want, got[:2]
            legs[k + ("_load_reads_keep_qual" if kq else "_load_reads")] = summary(w, pk, {"phase_ms_last": got[2], "chunk_info": got[3], "counters": got[4]})
    w, pk, got = timed(lambda: plain_route(files["plain"]))
    assert got == want
    legs["plain_fasta_load_seqset_keep_qual"] = summary(w, pk)
    w, pk, got = timed(lambda: device_route(files["plain"], True))
    legs["plain_load_reads_keep_qual"] = summary(w, pk, {"phase_ms_last": got[2], "chunk_info": got[3], "counters": got[4]})
    out = {
        "workload": D["text"], "fraction": "coverage %.3g of configs[2]'s %s" % (a.coverage, cfg["coverage"]), "device": eng.device_name(),
        "reads": want[0], "read_bases": want[1], "text_bytes": n_text, "file_bytes": {k: os.path.getsize(p) for k, p in files.items()},
        "write_seconds": t_write, "legs": legs,
        "timing": "per leg %d timed runs after one untimed one, the context's scratch released before each; wall clock around the Python call, set freed "
                  "inside it.  *_parent_read_fasta_seqset: fasta.read_fasta(with_qual=True) + Engine.seqset(seqs, qual) -- the route a .gz took before; "
                  "*_load_reads*: Engine.load_reads at the engine's own chunk size, phase columns of the last run (upload and inflate overlap with the "
                  "rest); plain_*: the plain file through fasta.load + Engine.seqset, and through load_reads, for scale.  peak_device_bytes: free device "
                  "memory before the call minus its minimum during it, sampled every 2 ms" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    for k, v in legs.items():
        print(k, json.dumps({x: v[x] for x in ("wall_ms_median", "wall_ms_spread", "peak_device_bytes")}), json.dumps(v.get("phase_ms_last", {})))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
