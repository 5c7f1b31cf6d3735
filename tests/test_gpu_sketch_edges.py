"""The first stage at its kernel edges (tests/sketch_edges.py): every case of the table through telr_index_build -- the three
sketch kernels, the homopolymer pre-pass, the radix sort, the entry, count and probe-table kernels -- against the plain reference
(ref_index, ref_mid_occ), array for array; the staged query-side sketch and the probe table as far as the anchor offsets and the
sorted anchors show them, against the oracle (compare_all of tests/test_gpu_parity.py) and against a plain occurrence count; the
index without entries; argument errors.  The two switches that change the index path -- TELR_AB=sketch64 (k_sketch with the
unrolled HALO = 9 selection at k <= 15) and TELR_AB=index_sort_lib (rocPRIM's sort, an independent witness of the hand-written
one) -- run the index comparison over the whole table in a process of their own (switches are read once per process).  The
reference itself is held to hand-derived answers, and every case to the edge it is built for, in
tests/test_sketch_reference.py (CPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from telr_amd._abi import IdxOpt, MF_CIGAR
from telr_amd._lib import TelrError
from telr_amd.presets import preset
import sketch_edges as se
from test_gpu_parity import compare_all

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = se.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_index_equals_the_reference(engine, case):
    se.check_index(engine, case, se.reference(case))


@pytest.mark.parametrize("k,w,hpc", se.forms(), ids=["k%dw%d%s" % (k, w, "h" if h else "") for k, w, h in se.forms()])
def test_query_sketch_and_probe_table(engine, k, w, hpc):
    """a form's targets mapped against their own index, plus three queries that share nothing with it: no occurrence is cut
    (min_mid_occ = max_mid_occ = 10^6), so the anchor count is the plain sum over the query minimizers of their hashes'
    occurrences in the reference index, and the foreign queries bring none"""
    targets, foreign = se.query_set(k, w, hpc)
    queries = targets + foreign
    io = IdxOpt(k=k, w=w, is_hpc=hpc, bucket_bits=0)
    _, mo = preset("map-ont")
    mo.flags &= ~MF_CIGAR
    mo.min_mid_occ = mo.max_mid_occ = 10 ** 6
    ent_hash, ent_off, _, _, _ = se.ref_index(targets, k, w, hpc)
    occ = dict(zip(ent_hash.tolist(), np.diff(ent_off.astype(np.int64)).tolist()))
    per_query = [sum(occ.get(x >> 8, 0) for x, _ in se.brute(q, k, w, hpc)) for q in queries]
    assert sum(per_query[:len(targets)]) > 0 and per_query[len(targets):] == [0, 0, 0]
    _, oref = compare_all(engine, targets, queries, io, mo, stages=True)        # q_aoff, skeys == the oracle's (asserted in there)
    assert engine.counters()["minimizers"] == sum(len(se.brute(q, k, w, hpc)) for q in queries)
    np.testing.assert_array_equal(np.diff(oref["anchor_off"]), per_query)
    assert int(oref["anchor_off"][-1]) == sum(per_query)


@pytest.mark.parametrize("k,w", se.CONTENT_FORMS, ids=["k%dw%d" % f for f in se.CONTENT_FORMS])
def test_empty_index_maps_to_nothing(engine, k, w):
    case = [c for c in CASES if c[0] == "k%dw%d-empty_index" % (k, w)][0]
    _, mo = preset("map-ont")
    ix = engine.index(case[4], IdxOpt(k=k, w=w, is_hpc=0, bucket_bits=0))
    assert ix.stats() == (0, 0)
    query = se.rnd(np.random.default_rng(k), 3000)
    res = ix.map([query, "", "ACGT"], mo)
    assert len(res.alns) == 0 and len(res.cigars) == 0
    assert ix.debug_mid_occ(mo) == mo.min_mid_occ


@pytest.mark.parametrize("k,w", [(3, 10), (29, 10), (15, 0), (15, 256)])
def test_argument_errors(engine, k, w):
    with pytest.raises(TelrError, match="invalid argument"):          # TELR_E_ARG, through Engine._chk
        engine.index(["ACGTACGTTGCAAGGCTTAACCGGTTAGC" * 4], IdxOpt(k=k, w=w, is_hpc=0, bucket_bits=0))


@pytest.mark.parametrize("ab", ["sketch64", "index_sort_lib"])
def test_switches_keep_the_edges(ab):
    env = dict(os.environ, TELR_AB=ab)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sketch_child.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.rstrip().endswith("sketch edges ok: %d cases" % len(CASES)), p.stdout[-2000:]
