"""bench.py --dump-outputs (CPU): the files hold the sampled reads' records and CIGAR words exactly, as float64, within the
byte budget, and the same inputs give the same files."""
import glob
import os

import numpy as np

import bench
from oracle import binding as ob
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def _oracle_result(data_dir):
    _, ts = read_fasta(os.path.join(data_dir, "ref_38kb.fasta"))
    _, qs = read_fasta(os.path.join(data_dir, "reads.fasta"))
    io, mo = preset("map-ont")
    r = ob.OracleIndex(ts, io).map(qs, mo)
    return r["alns"], r["cigars"], len(qs)


def test_dump_holds_the_records_and_cigars_exactly(data_dir, tmp_path):
    al, cg, n_reads = _oracle_result(data_dir)
    info = bench.dump_outputs(str(tmp_path / "a"), al, cg, n_reads)
    d = _load(str(tmp_path / "a"))
    assert sorted(k + ".npy" for k in d) == info["files"]
    assert all(v.dtype == np.float64 for v in d.values())
    assert info["bytes"] == sum(v.nbytes for v in d.values()) <= bench.DUMP_MAX_BYTES
    assert info["reads"] == n_reads and info["records"] == len(al) > 0          # 18 reads: the sample is the whole set
    assert np.all(np.diff(d["alns_qid"]) >= 0)
    assert int(d["alns_n_cigar"].sum()) == len(d["cigars"]) == len(cg)
    for i in range(info["records"]):
        j = np.flatnonzero((al["qid"] == d["alns_qid"][i]) & (al["qs"] == d["alns_qs"][i]) & (al["ts"] == d["alns_ts"][i]) & (al["tid"] == d["alns_tid"][i]))
        assert len(j) == 1
        j = j[0]
        for f in al.dtype.names:
            if f != "cigar_off":
                assert d["alns_" + f][i] == al[f][j], f
        o, n = int(d["alns_cigar_off"][i]), int(d["alns_n_cigar"][i])
        assert np.array_equal(d["cigars"][o:o + n].astype(np.uint32), cg[al["cigar_off"][j]:al["cigar_off"][j] + n])
    bench.dump_outputs(str(tmp_path / "b"), al, cg, n_reads)
    e = _load(str(tmp_path / "b"))
    assert all(np.array_equal(d[k], e[k]) for k in d)


def test_dump_keeps_within_the_byte_budget(data_dir, tmp_path, monkeypatch):
    al, cg, n_reads = _oracle_result(data_dir)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 50000)
    info = bench.dump_outputs(str(tmp_path), al, cg, n_reads)
    d = _load(str(tmp_path))
    assert 0 < info["reads"] < n_reads and info["bytes"] == sum(v.nbytes for v in d.values()) <= 50000
    assert int(d["alns_n_cigar"].sum()) == len(d["cigars"])
