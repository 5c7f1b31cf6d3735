"""The device BAM writer at its kernels' edges (tests/bam_edges.py) against the plain encoder of tests/bam_reference.py: every
hand-built case goes through telr_result_from_arrays and then through
  * telr_write_bam_dev at level 0 (stored blocks) and level 1 (the device's deflate),
  * telr_write_bam (the host writer),
  * telr_write_bam_slice + telr_bam_segment_write + telr_bai_write on one device, the records dealt to 2 and 3 pretended
    ranks (halves and thirds of the coordinate order with an empty rank in the middle or in front: the file and the index of
    one writer; alternating records: every rank's records in coordinate order, one rank after the other, no index),
and every file, inflated block by block with zlib (CRC-32, ISIZE, BSIZE <= 65,536, ISIZE <= 65,280 checked), must hold the
reference stream byte for byte; every .bai, its virtual offsets translated through the file's own block table, the reference
index (chunks of a bin may be joined where the first ends in the BGZF block the next begins in, as samtools joins them: see
bam_reference.compare_bai).  The short last blocks must come out stored at level 1.  No tolerance anywhere: bytes.
The writer's two TELR_AB switches run the same set in a process of their own (they are read once per process).
tests/test_bam_reference.py holds the reference to hand-derived strings and every case to its edge, on the CPU."""
import os
import subprocess
import sys

import pytest

import bam_edges as be

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return be.cases()


@pytest.mark.parametrize("group", ["walk", "layout", "sort", "sa", "framing", "deflate"])
def test_writers_equal_the_plain_encoder(engine, cases, tmp_path, group):
    mine = [c for c in cases if c["group"] == group]
    assert len(mine) >= 2
    # (a comparison only means something where the case reaches its edge: checked first, on the same set)
    missed = [(c["name"], c["reach"](be.stream_of(c), c)) for c in mine]
    assert not [m for m in missed if m[1]], missed
    if group == "sort":
        free, total = engine.mem_info()
        print("device memory before the 8-Mb and 64-Mb targets: %.1f of %.1f GB free" % (free / 1e9, total / 1e9))
    bad = be.run_all(engine, mine, str(tmp_path))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


@pytest.mark.parametrize("switch", ["bam_no_populate", "bam_no_twin"])
def test_switches_keep_the_edges(switch):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bam_edges.py"), "--engine"], env=dict(os.environ, TELR_AB=switch), cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "bam edges ok" in p.stdout
