"""End-to-end inputs of the TELR_MF_CHAIN_SKIP tests (tests/test_gpu_chain_skip.py): the small HARD genome of telr_amd/synth.py
(tandem arrays, satellites, segmental duplications, reads with error bursts), where minimap2's scan and the fixed look-back differ."""
import functools

import numpy as np

from telr_amd import synth


@functools.lru_cache(maxsize=None)
def hard_genome():
    return synth.make_genome(11, [("a", 1_200_000), ("b", 400_000)], n_ins=20, hard=synth.HARD)


def _reads(g, coverage, seed, err=(0.04, 0.02, 0.04), mean_len=9000):
    plan = synth.plan_reads(g, coverage, mean_len=mean_len, read_seed=seed)
    buf, off, ln, _ = synth.materialize_reads(g, plan, err=err, burst=synth.HARD["burst"])
    return [buf[off[i]:off[i] + ln[i]] for i in range(len(ln))]


@functools.lru_cache(maxsize=None)
def hard_ont_reads(n=2000):
    """at least n ONT-like reads of the hard genome"""
    g = hard_genome()
    cov = 1.0
    while True:
        r = _reads(g, cov, 5)
        if len(r) >= n:
            return r[:n]
        cov *= 1.5 * n / max(len(r), 1)


@functools.lru_cache(maxsize=None)
def hard_clr_reads(n=80):
    """CLR-like reads (the map-pb error profile of tests/test_gpu_parity.py) of the hard genome"""
    return _reads(hard_genome(), 0.6, 6, err=(0.013, 0.065, 0.052), mean_len=7000)[:n]


def hard_contigs_and_windows(n_win=40, seed=8):
    """per-target shape (S5 / S7): windows of the reads' sequence as queries against the hard genome's chromosomes as targets"""
    rng = np.random.default_rng(seed)
    reads = hard_ont_reads()
    out = []
    for _ in range(n_win):
        r = reads[int(rng.integers(0, len(reads)))]
        if len(r) < 3000:
            continue
        s = int(rng.integers(0, len(r) - 2500))
        out.append(r[s:s + 2500])
    return [bytes(c).decode() for c in hard_genome()["ref"]], out
