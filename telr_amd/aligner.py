"""Object layer over the C ABI: Engine (context), SeqSet, Index, MapResult.

This is the in-process replacement of the reference's `subprocess.call(["minimap2", ...])`
boundary (TELR_alignment.py:69-82 and the five other sites listed in include/telr_hip.h).
"""
import ctypes as C
import numpy as np
from . import _lib
from ._abi import CohortOpt, COHORT_ENTRY_DTYPE, COHORT_SITE_DTYPE, COHORT_SHADOWED
from ._abi import IdxOpt, MapOpt, Counters, InsOpt, SiteOpt, GenoOpt, DraftOpt, BridgeOpt, RefTeOpt, ALN_DTYPE, INS_SIG_DTYPE, INS_CALL_DTYPE, GENO_DTYPE, DRAFT_DTYPE, BRIDGE_DTYPE, TILE_DTYPE, \
    TE_FEAT_DTYPE, TELR_E_ARG, TELR_E_RANGE, MF_PER_TARGET, MF_KEEP_CIGARS, N_STAGES, N_DPCLS, STITCH_CHAIN_COLUMNS, ALIGN_CHAIN_COLUMNS, ALIGN_PROB_COLUMNS
from .fasta import concat

BAM_CHUNK_FIT = -1        # TELR_BAM_CHUNK_FIT (include/telr_hip.h): Engine.load_bam decides between the whole-file and the chunked load

def _np_from(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    dt = np.dtype(dtype)
    buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dt, count=n).copy()


def _ic_arrays(entry, ic, with_sigs=False):
    """an InsCalls (or anything with calls / read_off / reads / sigs of that form) as the C ABI takes it ->
    contiguous (calls, read_off, reads, sigs or None); `entry` opens the error text"""
    calls = np.ascontiguousarray(ic.calls, dtype=INS_CALL_DTYPE)
    sigs = np.ascontiguousarray(ic.sigs, dtype=INS_SIG_DTYPE) if with_sigs else None
    read_off = np.ascontiguousarray(ic.read_off, dtype=np.int64)
    reads = np.ascontiguousarray(ic.reads, dtype=np.int32)
    if len(read_off) != len(calls) + 1 or (len(calls) and int(read_off[-1]) > len(reads)):
        raise _lib.TelrError("%s: read_off must hold len(calls) + 1 offsets into reads" % entry)
    return calls, read_off, reads, sigs


def _qual_arrays(qual):
    """base qualities as the C ABI takes them: a list of quality strings (str / bytes, Phred + 33, one per sequence) or the
    (buffer, offsets) pair of fasta.FastaFile.qual -> (uint8 buffer, int64 offsets)"""
    if isinstance(qual, tuple) and len(qual) == 2:
        buf, off = qual
    else:
        buf, off, _ = concat([q.encode("latin-1") if isinstance(q, str) else q for q in qual])
    return np.ascontiguousarray(buf, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)


_DEFERRED = None          # list of (free function, handle) while deferred_frees() is active


class deferred_frees:
    """`with deferred_frees():` -- sequence sets and indexes freed inside the block (explicitly or by the garbage collector) give
    their device memory back when the block ends.  hipFree waits for the whole device, so a free on one context stalls its host
    thread behind whatever another context of the process is running (the loci bundle: S4 / S5 / S7 next to S6)."""

    def __enter__(self):
        global _DEFERRED
        self.outer = _DEFERRED
        if _DEFERRED is None:
            _DEFERRED = []
        return self

    def __exit__(self, *exc):
        global _DEFERRED
        if self.outer is None:
            todo, _DEFERRED = _DEFERRED, None
            for fn, h in todo:
                fn(h)
        return False


class Engine:
    """One per process per device."""

    def __init__(self, device=0, background=False):
        self.L = _lib.lib()
        h = C.c_void_p()
        rc = (self.L.telr_init_background if background else self.L.telr_init)(device, C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_init(%d): %s" % (device, self.L.telr_strerror(rc).decode()))
        self.h = h
        self.device = device

    def _chk(self, rc, what):
        if rc != 0:
            raise _lib.TelrError("%s: %s [%s]" % (what, self.L.telr_strerror(rc).decode(),
                                                  self.L.telr_last_error(self.h).decode()), rc)

    def device_name(self):
        b = C.create_string_buffer(256)
        self.L.telr_device_name(self.h, b, 256)
        return b.value.decode()

    def seqset(self, seqs, qual=None):
        """qual: the sequences' base qualities (see SeqSet.attach_qual), kept on the device for the QUAL field of write_bam_device"""
        return SeqSet(self, seqs, qual)

    def index(self, targets, io):
        return Index(self, targets, io)

    @staticmethod
    def part_plan(lengths, max_bases=0):
        """-> part_of (int32, one part number per target): how targets of these lengths are cut into parts that each fit an index of at
        most max_bases bases of padded extent (0: the engine's own limit, 2^31) -- contiguous runs in target order, chosen greedily
        (telr_part_plan; include/telr_hip.h has the definition; no device needed)"""
        a = np.ascontiguousarray(lengths, dtype=np.int32)
        L = _lib.lib()
        part_of = np.zeros(max(len(a), 1), np.int32); n = C.c_int32(0)
        rc = L.telr_part_plan(len(a), a.ctypes.data, int(max_bases), part_of.ctypes.data, C.byref(n))
        if rc != 0:
            raise _lib.TelrError("telr_part_plan: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_part_plan_error().decode()), rc)
        return part_of[:len(a)]

    def merge_sites(self, entries, n_targets, opt=None):
        """several samples' insertion calls merged into one site list on the device (telr_merge_sites; include/telr_hip.h has the
        definition, which is not bcftools merge, SURVIVOR or Jasmine): entries a COHORT_ENTRY_DTYPE array or a list of
        (tid, pos, len, sample, group) tuples in any order, opt an _abi.CohortOpt (None: the defaults) -> CohortSites.  No index is
        needed: the merge reads no sequence."""
        o = CohortOpt.default() if opt is None else opt
        if isinstance(entries, np.ndarray) and entries.dtype == COHORT_ENTRY_DTYPE:
            e = np.ascontiguousarray(entries)
        else:
            e = np.ascontiguousarray(np.asarray(entries, dtype=np.int32).reshape(-1, 5)).view(COHORT_ENTRY_DTYPE).reshape(-1)
        h = C.c_void_p()
        self._chk(self.L.telr_merge_sites(self.h, e.ctypes.data if len(e) else None, len(e), int(n_targets), C.byref(o), C.byref(h)), "telr_merge_sites")
        try:
            L = self.L
            k = int(L.telr_cohort_sites_count(h))
            member_off = _np_from(L.telr_cohort_sites_member_off(h), k + 1, np.int64)
            sample_off = _np_from(L.telr_cohort_sites_sample_off(h), k + 1, np.int64)
            return CohortSites(_np_from(L.telr_cohort_sites_sites(h), k, COHORT_SITE_DTYPE), member_off, _np_from(L.telr_cohort_sites_members(h), int(member_off[-1]), np.int32),
                               sample_off, _np_from(L.telr_cohort_sites_samples(h), int(sample_off[-1]), np.int32))
        finally:
            self.L.telr_cohort_sites_free(h)

    def index_parts(self, targets, io, max_part_bases=0, like=None):
        """a multi-part index over targets of any total size -> PartIndex.  like: another PartIndex over the same
        targets (and the same max_part_bases), whose resident target set and subsets are used again"""
        return PartIndex(self, targets, io, max_part_bases, like)

    @staticmethod
    def bam_chunk_plan(isize, chunk_bytes):
        """-> first_member_of_chunk (int64): how a file whose BGZF members inflate to these ISIZE is cut into chunks of at most
        chunk_bytes inflated bytes (telr_bam_chunk_plan; include/telr_hip.h has the definition; no device needed)"""
        a = np.ascontiguousarray(isize, dtype=np.int32)
        L = _lib.lib()
        first = np.zeros(max(len(a), 1), np.int64); n = C.c_int64(0)
        rc = L.telr_bam_chunk_plan(len(a), a.ctypes.data, int(chunk_bytes), first.ctypes.data, len(a), C.byref(n))
        if rc != 0:
            raise _lib.TelrError("telr_bam_chunk_plan: %s" % L.telr_strerror(rc).decode(), rc)
        return first[:int(n.value)]

    @staticmethod
    def _regions(regions):
        """(tid, beg, end[, reserved]) tuples -> the telr_region array"""
        a = np.zeros((len(regions), 4), np.int32)
        for i, r in enumerate(regions):
            a[i, :len(r)] = [int(x) for x in r]
        return a

    @staticmethod
    def bai_plan(bai, n_ref, regions):
        """-> (vbeg, vend) (uint64): the intervals of virtual offsets that the index file `bai` names for `regions`, a list of
        (tid, beg, end) -- sorted and merged, but not clipped to target lengths (telr_bai_plan; include/telr_hip.h has the definition;
        no device needed)"""
        L = _lib.lib()
        reg = Engine._regions(regions)
        n = C.c_int64(0)
        rc = L.telr_bai_plan(str(bai).encode(), int(n_ref), len(reg), reg.ctypes.data, None, None, 0, C.byref(n))
        vb, ve = np.zeros(max(int(n.value), 1), np.uint64), np.zeros(max(int(n.value), 1), np.uint64)
        if rc == -4:          # TELR_E_RANGE: the count is exact, call again
            rc = L.telr_bai_plan(str(bai).encode(), int(n_ref), len(reg), reg.ctypes.data, vb.ctypes.data, ve.ctypes.data, len(vb), C.byref(n))
        if rc != 0:
            raise _lib.TelrError("telr_bai_plan: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_bai_plan_error().decode()), rc)
        return vb[:int(n.value)], ve[:int(n.value)]

    def load_bam(self, path, keep_qual=False, chunk_bytes=None, regions=None, bai=None):
        """a BAM file as stage-1 input, inflated and parsed on the device (telr_bam_load; include/telr_hip.h has the definition)
        -> BamInput.  keep_qual: attach the reads' base qualities to the read set when every sequence-bearing record has them.
        chunk_bytes: None = the whole file at once (it must fit into device memory next to its inflated stream); n > 0 = in chunks of
        at most n inflated bytes, 0 = in chunks of the engine's own size (telr_bam_load_chunked: a file of any size, the same result);
        BAM_CHUNK_FIT = the whole file when it fits into half the free device memory, else as 0.
        regions: a list of (tid, beg, end), 0-based and half-open: only the records that overlap one of them are loaded, and only the
        BGZF members that the index `bai` (None: path + ".bai") names for them are inflated (telr_bam_load_regions; chunk_bytes None
        stands for BAM_CHUNK_FIT there).  A read whose sequence-bearing record lies outside the regions is no read of the result, and
        its records inside are orphans.  None: the whole file, as ever"""
        return BamInput(self, path, keep_qual, chunk_bytes, regions, bai)

    def load_reads(self, path, keep_qual=False, chunk_bytes=0):
        """a FASTA / FASTQ file -- plain, gzip or BGZF, decided by content -- as a resident read set, parsed and packed on the device
        in chunks (telr_reads_load; include/telr_hip.h has the definition) -> ReadsInput.  keep_qual: a FASTQ's qualities stay with
        the set.  chunk_bytes: at most that many bytes of text per chunk, 0 = the engine's own size; the result does not depend on it"""
        return ReadsInput(self, path, keep_qual, chunk_bytes)

    def stage_ms(self):
        a = np.zeros(N_STAGES, np.float32)
        self.L.telr_stage_ms(self.h, a.ctypes.data)
        return {self.L.telr_stage_name(i).decode(): float(a[i]) for i in range(N_STAGES)}

    def counters(self):
        c = Counters()
        self.L.telr_last_counters(self.h, C.byref(c))
        return {k: getattr(c, k) for k, _ in Counters._fields_}

    def dp_classes(self):
        """per DP class: (problems, cells, steps, algorithmic bytes) of the last map call"""
        a = np.zeros(N_DPCLS * 4, np.int64)
        self.L.telr_last_dp_classes(self.h, a.ctypes.data)
        return a.reshape(N_DPCLS, 4)

    # the eight host bounds of the packed int16 DP classes for `mo` (telr_engine.hip: dp_limits)
    DP_LIMITS = ("pk_steps_limit", "pk_wide_limit", "pk_wide_maxd", "pk_ext_limit", "pk_ext_maxd", "tb4_mask", "tb4_steps", "tag8_steps")

    @staticmethod
    def dp_limits(mo):
        """-> {name: value} of DP_LIMITS (no device needed)"""
        a = np.zeros(8, np.int32)
        rc = _lib.lib().telr_debug_dp_limits(C.byref(mo), a.ctypes.data)
        if rc != 0:
            raise _lib.TelrError("telr_debug_dp_limits: %d" % rc, rc)
        return dict(zip(Engine.DP_LIMITS, (int(v) for v in a)))

    DP_CLASS_COLUMNS = ("maxd", "lanes", "regs", "row_dwords", "interleaved", "tiled")

    @staticmethod
    def dp_class_table():
        """-> (N_DPCLS, 6) int32, columns DP_CLASS_COLUMNS: what defines each DP class (no device needed)"""
        a = np.zeros((N_DPCLS, 6), np.int32)
        rc = _lib.lib().telr_debug_dp_class_table(a.ctypes.data)
        if rc != 0:
            raise _lib.TelrError("telr_debug_dp_class_table: %d" % rc, rc)
        return a

    MAP_PLAN_MODES = ("serial", "in_turn", "two_in_flight")

    @staticmethod
    def map_plan(lengths, per_base=0.0, qtarget=False, vote=False, debug=0, pipe_nomem=False):
        """-> (mode, batch_bases, range ends): how telr_map would cut reads of these lengths into ranges and run them, under the
        TELR_BATCH_MBP / TELR_BATCH_KBP / TELR_PIPELINE of the moment (no device needed).  mode: one of MAP_PLAN_MODES"""
        a = np.ascontiguousarray(lengths, dtype=np.int32)
        out = np.zeros(3, np.int64); ends = np.zeros(max(len(a), 1), np.int32)
        rc = _lib.lib().telr_debug_map_plan(a.ctypes.data, len(a), int(a.max()) if len(a) else 0, float(per_base), int(bool(qtarget)),
                                            int(bool(vote)), int(debug), int(bool(pipe_nomem)), out.ctypes.data, ends.ctypes.data)
        if rc != 0:
            raise _lib.TelrError("telr_debug_map_plan: %d" % rc, rc)
        return Engine.MAP_PLAN_MODES[int(out[0])], int(out[1]), [int(e) for e in ends[:int(out[2])]]

    @staticmethod
    def tile_plan(lengths, tile, stride):
        """-> TILE_DTYPE array (tid, start, len): the overlapping tiles of targets of these lengths, in (tid, start) order (telr_tile_plan;
        include/telr_hip.h has the definition; no device needed)"""
        a = np.ascontiguousarray(lengths, dtype=np.int32)
        L = _lib.lib()
        need = C.c_int64(0)
        rc = L.telr_tile_plan(len(a), a.ctypes.data, int(tile), int(stride), None, 0, C.byref(need))
        if rc != 0 and not (rc == TELR_E_RANGE and need.value > 0):
            raise _lib.TelrError("telr_tile_plan: %s" % L.telr_strerror(rc).decode(), rc)
        out = np.zeros(need.value, TILE_DTYPE)
        if need.value:
            rc = L.telr_tile_plan(len(a), a.ctypes.data, int(tile), int(stride), out.ctypes.data, len(out), C.byref(need))
            if rc != 0:
                raise _lib.TelrError("telr_tile_plan: %s" % L.telr_strerror(rc).decode(), rc)
        return out

    def annotate_hits(self, r, tiles, target_len, n_families, opt=None):
        """the records of a tile map as reference TE features (telr_annotate_hits; include/telr_hip.h has the definition, which is not
        RepeatMasker's): r a raw result whose queries are `tiles` (a TILE_DTYPE array as tile_plan returns it) and whose targets are the
        n_families library sequences; target_len the lengths of the tiled targets; opt an _abi.RefTeOpt (None: the defaults)
        -> TE_FEAT_DTYPE array in (tid, start, end, family, strand) order"""
        o = RefTeOpt.default() if opt is None else opt
        tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        tl = np.ascontiguousarray(target_len, dtype=np.int32)
        h = C.c_void_p()
        L = self.L
        rc = L.telr_annotate_hits(self.h, r, len(tiles), tiles.ctypes.data, len(tl), tl.ctypes.data, int(n_families), C.byref(o), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_annotate_hits: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_last_error(self.h).decode()), rc)
        try:
            return _np_from(L.telr_te_feats_data(h), int(L.telr_te_feats_count(h)), TE_FEAT_DTYPE)
        finally:
            L.telr_te_feats_free(h)

    def debug_dp(self, queries, targets, mo, probs):
        """one DP pass (the map path's dp_pass) over a list of problems -- test tap.  probs: (np, 12) int32 rows
        {qid, q_off, tid, t_off, m, n, dlo, dhi, kind, qstep, tstep, qcomp}; queries / targets: SeqSet.
        -> dict of per-problem arrays cls, retry, score, bi, bj, mlen, tb_off, and cigars (a list of uint32 arrays, start to end)"""
        P = np.ascontiguousarray(probs, dtype=np.int32).reshape(-1, 12)
        npb = len(P)
        res = np.zeros((npb, 8), np.int32); tb = np.zeros(npb, np.int64)
        steps = P[:, 4].astype(np.int64) + P[:, 5]
        cap = int((6 * steps + 16).sum()) + 16
        cig = np.zeros(cap, np.uint32)
        self._chk(self.L.telr_debug_dp(self.h, queries.h, targets.h, C.byref(mo), P.ctypes.data, npb, res.ctypes.data,
                                       tb.ctypes.data, cig.ctypes.data, cap), "telr_debug_dp")
        out = {k: res[:, i].copy() for i, k in enumerate(("cls", "retry", "score", "bi", "bj", "mlen"))}
        out["tb_off"] = tb
        out["cigars"] = [cig[res[x, 7]:res[x, 7] + res[x, 6]].copy() for x in range(npb)]
        return out

    def debug_stitch(self, p_off, has_left, prob, cigars, cx_scale=0):
        """CIGAR stitching and the per-chain sums (the map path's stitch_count and k_stitch_write) on hand-made per-problem
        results -- test tap.  p_off: n_chain + 1 problem offsets; has_left: per chain; prob: (np, 5) int32 rows STITCH_PROB_COLUMNS;
        cigars: per problem its words (len << 4 | op) in storage order, as the trace-back leaves them (end to start of the DP problem).
        -> dict of per-chain arrays dp, mlen, blen, l_bi, l_bj, r_bi, r_bj, n_cigar, and cigars (a list of uint32 arrays)"""
        O = np.ascontiguousarray(p_off, dtype=np.int32)
        HL = np.ascontiguousarray(has_left, dtype=np.int32)
        P = np.ascontiguousarray(prob, dtype=np.int32).reshape(-1, 5)
        if len(O) < 1 or len(HL) != len(O) - 1 or len(cigars) != len(P) or (len(O) > 1 and int(O[-1]) != len(P)):
            raise _lib.TelrError("telr_debug_stitch: p_off must hold n_chain + 1 offsets ending at the problem count", TELR_E_ARG)
        co = np.zeros(len(P) + 1, np.int64)
        co[1:] = np.cumsum([len(c) for c in cigars])
        raw = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32) for c in cigars]) if len(cigars) else np.zeros(0), dtype=np.uint32)
        nk, cap = len(O) - 1, len(raw) + 1
        out = np.zeros((nk, len(STITCH_CHAIN_COLUMNS)), np.int32); cig = np.zeros(cap, np.uint32)
        self._chk(self.L.telr_debug_stitch(self.h, nk, O.ctypes.data, HL.ctypes.data, P.ctypes.data, co.ctypes.data, raw.ctypes.data, int(cx_scale),
                                           out.ctypes.data, cig.ctypes.data, cap), "telr_debug_stitch")
        r = {k: out[:, i].copy() for i, k in enumerate(STITCH_CHAIN_COLUMNS[:-1])}
        r["cigars"] = [cig[out[k, 8]:out[k, 8] + out[k, 7]].copy() for k in range(nk)]
        return r

    def debug_align(self, queries, targets, mo, chains, prob_off, probs):
        """both DP passes, stitching and the records' numbers (the map path's dp_passes, stitch_count, k_stitch_write and
        chain_numbers) of a caller's chains -- test tap.  chains: (n_chain, 7) int32 rows ALIGN_CHAIN_IN_COLUMNS (the query interval on
        the chain's strand); prob_off: n_chain + 1 offsets into probs, (np, 12) rows as debug_dp takes them; queries / targets: SeqSet.
        -> dict: `chains` {ALIGN_CHAIN_COLUMNS but the last: arrays}, `cigars` (a list of uint32 arrays), `probs` {ALIGN_PROB_COLUMNS:
        arrays}, n_retry, and acc, the (N_DPCLS * 4 + 1) int64 accounts of the call"""
        Cn = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1, 7)
        O = np.ascontiguousarray(prob_off, dtype=np.int32)
        P = np.ascontiguousarray(probs, dtype=np.int32).reshape(-1, 12)
        if len(O) != len(Cn) + 1 or (len(Cn) and int(O[-1]) != len(P)):
            raise _lib.TelrError("telr_debug_align: prob_off must hold n_chain + 1 offsets ending at the problem count", TELR_E_ARG)
        nk, npb = len(Cn), len(P)
        cap = int((P[:, 4].astype(np.int64) + P[:, 5] + 2).sum()) + 16
        co = np.zeros((nk, len(ALIGN_CHAIN_COLUMNS)), np.int32); po = np.zeros((npb, len(ALIGN_PROB_COLUMNS)), np.int32)
        cig = np.zeros(cap, np.uint32); acc = np.zeros(N_DPCLS * 4 + 1, np.int64); n_retry = C.c_int32(0)
        self._chk(self.L.telr_debug_align(self.h, queries.h, targets.h, C.byref(mo), nk, Cn.ctypes.data, O.ctypes.data, P.ctypes.data, co.ctypes.data,
                                          po.ctypes.data, cig.ctypes.data, cap, C.byref(n_retry), acc.ctypes.data), "telr_debug_align")
        return dict(chains={k: co[:, i].copy() for i, k in enumerate(ALIGN_CHAIN_COLUMNS[:-1])},
                    cigars=[cig[co[k, 8]:co[k, 8] + co[k, 7]].copy() for k in range(nk)],
                    probs={k: po[:, i].copy() for i, k in enumerate(ALIGN_PROB_COLUMNS)}, n_retry=int(n_retry.value), acc=acc)

    def debug_chain(self, keys, q_aoff, mo):
        """the chaining stage of map() on sorted anchor lists -- test tap.  keys: uint64 anchors in the engine's layout (strand << 63 |
        global reference position << 32 | query position << 8 | span), query q's at [q_aoff[q], q_aoff[q + 1]), ascending.
        -> (f, p) int32 arrays (p relative to the query's first anchor, -1 for none)"""
        K = np.ascontiguousarray(keys, dtype=np.uint64)
        O = np.ascontiguousarray(q_aoff, dtype=np.int32)
        if len(O) < 1 or int(O[-1]) != len(K):
            raise ValueError("q_aoff must hold nq + 1 offsets ending at len(keys)")
        f = np.zeros(len(K), np.int32); p = np.zeros(len(K), np.int32)
        self._chk(self.L.telr_debug_chain(self.h, len(O) - 1, K.ctypes.data, O.ctypes.data, C.byref(mo), f.ctypes.data, p.ctypes.data),
                  "telr_debug_chain")
        return f, p

    def debug_radix_sort(self, keys, nbits, vals=None):
        """the LSD radix sort of the index build and the call stages (radix_sort_passes) on host arrays -- test tap.  keys: uint64 with
        vals (uint32), or uint32 without; sorted stably by the low 8 * ceil(nbits / 8) bits.  -> (keys, vals or None)"""
        K = np.ascontiguousarray(keys)
        if K.dtype not in (np.uint64, np.uint32):
            raise ValueError("keys must be uint64 or uint32")
        V = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
        if V is not None and len(V) != len(K):
            raise ValueError("one value per key")
        ok = np.zeros_like(K); ov = None if V is None else np.zeros_like(V)
        self._chk(self.L.telr_debug_radix_sort(self.h, K.itemsize, K.ctypes.data, None if V is None else V.ctypes.data, len(K), nbits,
                                               ok.ctypes.data, None if ov is None else ov.ctypes.data), "telr_debug_radix_sort")
        return ok, ov

    def debug_qscan(self, cnt, out_dtype, cap=0, want_tot=True, want_n_over=False, want_list=False, n_over_in=0):
        """the tiled exclusive scan (dev_qscan) on host counts -- test tap.  cnt: int32 or int64; out_dtype np.int32 or np.int64 (int32
        -> int32 / int64, int64 -> int64).  n_over_in: what the counter of over-cap counts holds on entry.
        -> dict: out (n + 1), tot64 (or None), n_over (or None), over_list (the reported indices in arrival order, or None)"""
        A = np.ascontiguousarray(cnt)
        if A.dtype not in (np.int32, np.int64):
            raise ValueError("cnt must be int32 or int64")
        out = np.full(len(A) + 1, -1, out_dtype)
        tot = C.c_int64(-1); nov = C.c_int32(n_over_in); lst = np.full(max(len(A), 1), -1, np.int32)
        self._chk(self.L.telr_debug_qscan(self.h, A.itemsize, out.itemsize, A.ctypes.data, len(A), out.ctypes.data, C.byref(tot) if want_tot else None, cap,
                                          C.byref(nov) if want_n_over else None, lst.ctypes.data if want_list else None), "telr_debug_qscan")
        return dict(out=out, tot64=int(tot.value) if want_tot else None, n_over=int(nov.value) if want_n_over else None,
                    over_list=lst[:max(0, min(int(nov.value), len(A)))].copy() if want_list else None)

    def debug_backtrack(self, keys, q_aoff, f, p, qlen, goff, tlen, mo):
        """peaks and back-tracking, pass-1 chain selection and DP segmenting of map() on anchor lists with their chaining scores -- test
        tap.  keys / q_aoff as debug_chain takes them, f / p per anchor (p relative to the query's first anchor, -1 for none), qlen per
        query, goff (n_targets + 1 ascending global offsets) and tlen per target.
        -> dict: chains (n, 9) {qid, score, cnt, rev, tid, rs, re, qs, qe} in discovery order with ch_off per query; canch, the chains'
        anchors back to back, with ch_aoff per chain; kept (k, 10), the same nine fields and the chain's row, query-major in rank order;
        probs (np, 12) rows as debug_dp takes them with prob_off per kept chain (empty without TELR_MF_CIGAR)"""
        K = np.ascontiguousarray(keys, dtype=np.uint64)
        O = np.ascontiguousarray(q_aoff, dtype=np.int32)
        F = np.ascontiguousarray(f, dtype=np.int32); P = np.ascontiguousarray(p, dtype=np.int32)
        QL = np.ascontiguousarray(qlen, dtype=np.int32)
        G = np.ascontiguousarray(goff, dtype=np.uint32); TL = np.ascontiguousarray(tlen, dtype=np.int32)
        nq, nt, na = len(O) - 1, len(TL), len(K)
        if nq < 0 or len(F) != na or len(P) != na or len(QL) != nq or len(G) != nt + 1:
            raise ValueError("array lengths: q_aoff nq + 1, f / p one per key, qlen nq, goff n_targets + 1")
        if nq < 1 or int(O[-1]) != na:
            raise _lib.TelrError("telr_debug_backtrack: q_aoff must hold nq + 1 >= 2 offsets ending at len(keys)")
        cap = 3 * na + 8
        ch_off = np.zeros(nq + 1, np.int32); chains = np.zeros((na + 1, 9), np.int32); ch_aoff = np.zeros(na + 2, np.int32)
        canch = np.zeros(na + 1, np.uint64); kept = np.zeros((na + 1, 10), np.int32); prob_off = np.zeros(na + 2, np.int32)
        probs = np.zeros((cap, 12), np.int32); n_out = np.zeros(3, np.int64)
        self._chk(self.L.telr_debug_backtrack(self.h, nq, O.ctypes.data, K.ctypes.data, F.ctypes.data, P.ctypes.data, QL.ctypes.data, nt,
                                              G.ctypes.data, TL.ctypes.data, C.byref(mo), ch_off.ctypes.data, chains.ctypes.data,
                                              ch_aoff.ctypes.data, canch.ctypes.data, kept.ctypes.data, prob_off.ctypes.data,
                                              probs.ctypes.data, cap, n_out.ctypes.data), "telr_debug_backtrack")
        nch, nk, npb = (int(v) for v in n_out)
        return dict(chains=chains[:nch].copy(), ch_off=ch_off, ch_aoff=ch_aoff[:nch + 1].copy(), canch=canch[:int(ch_aoff[nch])].copy(),
                    kept=kept[:nk].copy(), prob_off=prob_off[:nk + 1].copy(), probs=probs[:npb].copy())

    def release_scratch(self):
        """give the context's grow-only scratch back to the device (the next call allocates what it needs again)"""
        self._chk(self.L.telr_release_scratch(self.h), "telr_release_scratch")

    def mem_info(self):
        """(free, total) bytes of the device"""
        fr, tot = C.c_int64(), C.c_int64()
        self._chk(self.L.telr_device_mem(self.h, C.byref(fr), C.byref(tot)), "telr_device_mem")
        return fr.value, tot.value

    def worker(self):
        """A second context on the same device (created on first use, closed with this one): a host thread can run an engine
        call on it while this context runs another -- contexts are not re-entrant, different contexts are independent
        (the second range slot of a large call is such a context).  Sequence sets and indexes are plain device data and may be
        used from either."""
        w = getattr(self, "_worker", None)
        if w is None:
            w = self._worker = Engine(self.device, background=True)      # its kernels queue behind this context's
        return w

    def close(self):
        w = getattr(self, "_worker", None)
        if w is not None:
            self._worker = None
            w.close()
        if getattr(self, "h", None):
            self.L.telr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DevWords:
    """`n` int32 words of library-owned device memory, presented through the CUDA array interface (torch.as_tensor takes it
    without a copy); keeps the owning set alive"""
    def __init__(self, ptr, n, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i4", "data": (int(ptr), False), "version": 2}


class SeqSet:
    def __init__(self, eng, seqs, qual=None):
        self.eng = eng
        if isinstance(seqs, tuple) and len(seqs) == 3:
            buf, off, ln = seqs
        else:
            buf, off, ln = concat(seqs)
        self.len = np.ascontiguousarray(ln, dtype=np.int32)
        off = np.ascontiguousarray(off, dtype=np.int64)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        h = C.c_void_p()
        eng._chk(eng.L.telr_seqset_create(eng.h, len(self.len), buf.ctypes.data, off.ctypes.data, self.len.ctypes.data,
                                          C.byref(h)), "telr_seqset_create")
        self.h = h
        self.n = len(self.len)
        if qual is not None:
            self.attach_qual(qual)

    def bases(self):
        return int(self.eng.L.telr_seqset_bases(self.h))

    def attach_qual(self, qual, phred_offset=33):
        """one quality character per base: a list of strings (one per sequence) or a (buffer, offsets) pair such as
        fasta.FastaFile.qual; 1 byte of device memory per base (telr_seqset_attach_qual).  Sets made by subset() / from_packed()
        carry none.  A character outside phred_offset .. phred_offset + 93 raises and leaves the set without qualities."""
        if not (isinstance(qual, tuple) and len(qual) == 2):
            if len(qual) != self.n or any(len(q) != int(l) for q, l in zip(qual, self.len)):
                raise ValueError("attach_qual: one quality character per base of every sequence")
        buf, off = _qual_arrays(qual)
        if len(off) != self.n:
            raise ValueError("attach_qual: one offset per sequence")
        self.eng._chk(self.eng.L.telr_seqset_attach_qual(self.eng.h, self.h, buf.ctypes.data, off.ctypes.data, int(phred_offset)), "telr_seqset_attach_qual")

    @property
    def has_qual(self):
        return bool(self.eng.L.telr_seqset_has_qual(self.h))

    def subset(self, idx, eng=None, rc=None):
        """new set = copies of sequences idx (repeats allowed), gathered on the device from the packed form
        (eng: the context whose stream does the gather; default the one the set was made on); rc: one flag per copy, set = the copy
        is the reverse complement of its source (telr_seqset_subset_rc)"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        eng = self.eng if eng is None else eng
        sub = SeqSet.__new__(SeqSet)
        sub.eng = eng
        h = C.c_void_p()
        if rc is None:
            eng._chk(eng.L.telr_seqset_subset(eng.h, self.h, len(idx), idx.ctypes.data, C.byref(h)), "telr_seqset_subset")
        else:
            rc = np.ascontiguousarray(rc, dtype=np.uint8)
            if len(rc) != len(idx):
                raise ValueError("subset: one rc flag per index")
            eng._chk(eng.L.telr_seqset_subset_rc(eng.h, self.h, len(idx), idx.ctypes.data, rc.ctypes.data, C.byref(h)), "telr_seqset_subset_rc")
        sub.h = h; sub.len = self.len[idx].copy(); sub.n = len(idx)
        return sub

    def extract(self, idx, start, length, rc=None):
        """pieces of the resident set as text, cut on the device in ONE engine call (telr_seqset_extract; include/telr_hip.h has the
        definition): piece k = bases [start[k], start[k] + length[k]) of sequence idx[k], reverse-complemented where rc[k] != 0 (rc None:
        all forward) -> list of bytes, the letters A C G T and N as the set holds them.  Only the pieces come to the host."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        n = len(idx)
        if len(start) != n or len(length) != n:
            raise ValueError("extract: one start and one length per index")
        if rc is not None:
            rc = np.ascontiguousarray(rc, dtype=np.uint8)
            if len(rc) != n:
                raise ValueError("extract: one rc flag per index")
        off = np.zeros(n + 1, np.int64)
        np.cumsum(length, dtype=np.int64, out=off[1:])
        out = np.zeros(max(1, int(off[-1])), np.uint8)          # (a negative length is refused before anything is written)
        L = self.eng.L
        code = L.telr_seqset_extract(self.eng.h, self.h, n, idx.ctypes.data, start.ctypes.data, length.ctypes.data,
                                     None if rc is None else rc.ctypes.data, out.ctypes.data, off.ctypes.data)
        if code != 0:
            raise _lib.TelrError("telr_seqset_extract: %s [%s]" % (L.telr_strerror(code).decode(), L.telr_last_error(self.eng.h).decode()), code)
        buf = out.tobytes()
        return [buf[int(off[k]):int(off[k + 1])] for k in range(n)]

    def pieces(self, idx, start, length, rc=None, eng=None):
        """new set whose sequence k is bases [start[k], start[k] + length[k]) of sequence idx[k], reverse-complemented where rc[k] != 0
        (rc None: all forward), cut on the device from the packed form (telr_seqset_pieces): N stays N, no qualities are carried"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        n = len(idx)
        if len(start) != n or len(length) != n:
            raise ValueError("pieces: one start and one length per index")
        if rc is not None:
            rc = np.ascontiguousarray(rc, dtype=np.uint8)
            if len(rc) != n:
                raise ValueError("pieces: one rc flag per index")
        eng = self.eng if eng is None else eng
        h = C.c_void_p()
        code = eng.L.telr_seqset_pieces(eng.h, self.h, n, idx.ctypes.data, start.ctypes.data, length.ctypes.data,
                                        None if rc is None else rc.ctypes.data, C.byref(h))
        if code != 0:
            raise _lib.TelrError("telr_seqset_pieces: %s [%s]" % (eng.L.telr_strerror(code).decode(), eng.L.telr_last_error(eng.h).decode()), code)
        out = SeqSet.__new__(SeqSet)
        out.eng = eng; out.h = h; out.len = length.copy(); out.n = n
        return out

    def join(self, piece_off, idx, start, length, rc=None, eng=None):
        """new set whose sequence o is pieces piece_off[o] .. piece_off[o + 1] one after the other, each piece as in `pieces` (bases
        [start, start + length) of sequence idx, reverse-complemented where rc != 0; rc None: all forward), joined on the device from the
        packed form (telr_seqset_join): N stays N, a sequence may have no pieces, no qualities are carried"""
        piece_off = np.ascontiguousarray(piece_off, dtype=np.int64)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        n = len(idx)
        if len(piece_off) < 1:
            raise ValueError("join: piece_off holds one offset more than there are sequences")
        if len(start) != n or len(length) != n or int(piece_off[-1]) != n:
            raise ValueError("join: one start and one length per index, piece_off[-1] of them")
        if rc is not None:
            rc = np.ascontiguousarray(rc, dtype=np.uint8)
            if len(rc) != n:
                raise ValueError("join: one rc flag per index")
        eng = self.eng if eng is None else eng
        h = C.c_void_p()
        code = eng.L.telr_seqset_join(eng.h, self.h, len(piece_off) - 1, piece_off.ctypes.data, idx.ctypes.data, start.ctypes.data, length.ctypes.data,
                                      None if rc is None else rc.ctypes.data, C.byref(h))
        if code != 0:
            raise _lib.TelrError("telr_seqset_join: %s [%s]" % (eng.L.telr_strerror(code).decode(), eng.L.telr_last_error(eng.h).decode()), code)
        out = SeqSet.__new__(SeqSet)
        out.eng = eng; out.h = h; out.n = len(piece_off) - 1
        ends = np.concatenate([[0], np.cumsum(length, dtype=np.int64)])
        out.len = (ends[piece_off[1:]] - ends[piece_off[:-1]]).astype(np.int32)
        return out

    def packed(self):
        """the set's two word arrays as torch int32 tensors ON THE DEVICE, zero-copy views of the library's memory (valid while
        the set lives): what the N > 1 hand-offs put on the wire (telr_seqset_packed)"""
        import torch
        if not torch.cuda.is_available():
            raise _lib.TelrError("SeqSet.packed: torch sees no GPU in this process -- import torch BEFORE the first telr_amd call "
                                 "(the torch wheel carries its own HIP runtime; a process initialises only one)")
        p2, pn, n2, nn = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
        self.eng._chk(self.eng.L.telr_seqset_packed(self.h, C.byref(p2), C.byref(pn), C.byref(n2), C.byref(nn)), "telr_seqset_packed")
        dev = "cuda:%d" % self.eng.device

        def view(ptr, n):
            if n == 0:
                return torch.zeros(0, dtype=torch.int32, device=dev)
            return torch.as_tensor(_DevWords(ptr, n, self), device=dev)
        return view(p2.value, n2.value), view(pn.value, nn.value)

    @classmethod
    def from_packed(cls, eng, lengths, seq2, nmask):
        """a set built from packed words that are already on the device (torch int32 tensors, e.g. what an all-to-all delivered):
        one device-to-device copy, nothing is unpacked (telr_seqset_from_packed)"""
        import torch
        s = cls.__new__(cls)
        s.eng = eng
        s.len = np.ascontiguousarray(lengths, dtype=np.int32)
        seq2 = seq2.contiguous(); nmask = nmask.contiguous()
        torch.cuda.current_stream(seq2.device).synchronize()      # the words were produced on torch's stream (RCCL), the copy runs on the context's
        h = C.c_void_p()
        eng._chk(eng.L.telr_seqset_from_packed(eng.h, len(s.len), s.len.ctypes.data, C.c_void_p(seq2.data_ptr() if seq2.numel() else 0), int(seq2.numel()),
                                               C.c_void_p(nmask.data_ptr() if nmask.numel() else 0), int(nmask.numel()), C.byref(h)), "telr_seqset_from_packed")
        s.h = h; s.n = len(s.len)
        return s

    def free(self):
        if getattr(self, "h", None):
            if _DEFERRED is not None:               # hipFree waits for the device: not while another context's call is running on it
                _DEFERRED.append((self.eng.L.telr_seqset_free, self.h))
            else:
                self.eng.L.telr_seqset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MapResult:
    def __init__(self, alns, cigars):
        self.alns = alns
        self.cigars = cigars

    def cigar(self, i):
        a = self.alns[i]
        return self.cigars[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]

    def cigar_string(self, i):
        return "".join("%d%s" % (c >> 4, "MID"[c & 0xf]) for c in self.cigar(i))


class BamInput:
    """what Engine.load_bam returns: tnames / tlens (the header's references), qnames (the reads, in file order of their first
    sequence-bearing record), read_set (a SeqSet resident on the device, qualities attached when kept), result (a raw result handle with
    its CIGARs resident: Index.call_insertions, genotype_insertions, draft_contigs, write_bam_device, result_arrays, ...), counters
    (dict: members, records, mapped, kept, reads, orphans, len_mismatch, no_cigar, no_eof), phase_ms (dict) and chunk_info (dict: chunks,
    passes, largest_buffer, largest_carry; all 0 after a whole-file load), region_info (dict: regions (merged), intervals, members
    (inflated for the intervals), header_members, walked, selected; all 0 unless `regions` was given) and region_bytes (file bytes
    that a region load uploaded)"""
    COUNTERS = ("members", "records", "mapped", "kept", "reads", "orphans", "len_mismatch", "no_cigar", "no_eof")
    PHASES = ("host_hop", "upload", "inflate", "chain", "parse", "names_host", "sequences", "total")
    CHUNK_INFO = ("chunks", "passes", "largest_buffer", "largest_carry")
    REGION_INFO = ("regions", "intervals", "members", "header_members", "walked", "selected")

    def __init__(self, eng, path, keep_qual=False, chunk_bytes=None, regions=None, bai=None):
        L = eng.L
        self.eng = eng
        h = C.c_void_p()
        if regions is not None:
            reg = Engine._regions(regions)
            rc = L.telr_bam_load_regions(eng.h, str(path).encode(), None if bai is None else str(bai).encode(), 1 if keep_qual else 0,
                                         BAM_CHUNK_FIT if chunk_bytes is None else int(chunk_bytes), len(reg), reg.ctypes.data, C.byref(h))
        elif chunk_bytes is None:
            rc = L.telr_bam_load(eng.h, str(path).encode(), 1 if keep_qual else 0, C.byref(h))
        else:
            rc = L.telr_bam_load_chunked(eng.h, str(path).encode(), 1 if keep_qual else 0, int(chunk_bytes), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_bam_load: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_last_error(eng.h).decode()), rc)
        self.h = h
        ci = np.zeros(len(self.CHUNK_INFO), np.int64)
        L.telr_bam_in_chunk_info(h, ci.ctypes.data)
        self.chunk_info = dict(zip(self.CHUNK_INFO, (int(x) for x in ci)))
        ri = np.zeros(len(self.REGION_INFO), np.int64)
        L.telr_bam_in_region_info(h, ri.ctypes.data)
        self.region_info = dict(zip(self.REGION_INFO, (int(x) for x in ri)))
        self.region_bytes = int(L.telr_bam_in_region_bytes(h))
        nt, nq = int(L.telr_bam_in_target_count(h)), int(L.telr_bam_in_read_count(h))
        self.tnames = [x.decode("latin-1") for x in _cstrs(L.telr_bam_in_target_names(h), nt)]
        self.tlens = _np_from(L.telr_bam_in_target_lens(h), nt, np.int32)
        self.qnames = [x.decode("latin-1") for x in _cstrs(L.telr_bam_in_read_names(h), nq)]
        c = np.zeros(len(self.COUNTERS), np.int64); ph = np.zeros(len(self.PHASES), np.float32)
        L.telr_bam_in_counters(h, c.ctypes.data); L.telr_bam_in_phase_ms(h, ph.ctypes.data)
        self.counters = dict(zip(self.COUNTERS, (int(x) for x in c)))
        self.phase_ms = dict(zip(self.PHASES, (float(x) for x in ph)))
        # the set and the result become this object's: a SeqSet like any other, and a raw handle freed with the object
        rs = SeqSet.__new__(SeqSet)
        rs.eng = eng; rs.len = _np_from(L.telr_bam_in_read_lens(h), nq, np.int32); rs.n = nq
        rs.h = C.c_void_p(L.telr_bam_in_detach_seqset(h))
        self.read_set = rs
        self.result = C.c_void_p(L.telr_bam_in_detach_result(h))
        self._reads = None

    def reads(self):
        """the `bam2fasta` product as the (buffer, offsets, lengths) triple that seqset() and telr_sv.call_insertions take,
        decoded on the device from the packed set (telr_bam_in_ascii), once"""
        if self._reads is None:
            ln = self.read_set.len
            buf = np.zeros(max(1, int(ln.sum(dtype=np.int64))), np.uint8); off = np.zeros(max(1, len(ln)), np.int64)
            self.eng._chk(self.eng.L.telr_bam_in_ascii(self.h, buf.ctypes.data, off.ctypes.data), "telr_bam_in_ascii")
            self._reads = (buf[:int(ln.sum(dtype=np.int64))], off[:len(ln)], ln)
        return self._reads

    def map_result(self):
        """-> MapResult: the records and CIGAR words on the host"""
        L = self.eng.L
        return MapResult(_np_from(L.telr_result_alns(self.result), L.telr_result_count(self.result), ALN_DTYPE),
                         _np_from(L.telr_result_cigars(self.result), L.telr_result_cigar_count(self.result), np.uint32))

    def write_fasta(self, path):
        """the reads as FASTA, one line per sequence (what bam2fasta leaves behind, TELR_input.py:329-361)"""
        buf, off, ln = self.reads()
        with open(path, "wb") as f:
            for n, o, l in zip(self.qnames, off, ln):
                f.write(b">" + n.encode("latin-1") + b"\n" + buf[int(o):int(o) + int(l)].tobytes() + b"\n")

    def check_targets(self, tnames, tlens):
        """raises ValueError unless the file's references equal these by name, length and order (there is no remapping)"""
        if list(self.tnames) != [n.decode() if isinstance(n, bytes) else str(n) for n in tnames] or [int(x) for x in self.tlens] != [int(x) for x in tlens]:
            raise ValueError("the BAM's references are not the index's targets (names, lengths and order must agree)")

    def free(self):
        if getattr(self, "result", None):
            self.eng.L.telr_result_free(self.result); self.result = None
        if getattr(self, "h", None):
            self.eng.L.telr_bam_in_free(self.h); self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ReadsInput:
    """what Engine.load_reads returns: read_set (a SeqSet resident on the device, qualities attached when kept), qnames (list of str),
    names_c (the C array of names for the writers, valid while this object lives), n_bases, kind ("fastq", "fasta", or None for an
    empty text), container ("plain", "gzip", "bgzf"), counters, chunk_info and phase_ms (dicts)"""
    COUNTERS = ("container", "fastq", "members", "text_bytes", "lines", "records", "bases", "no_eof")
    CHUNK_INFO = ("chunks", "largest_buffer", "largest_carry", "peak_transient_bytes")
    PHASES = ("host_hop", "upload", "inflate", "lines", "records", "names", "pack", "join", "total")
    CONTAINERS = ("plain", "gzip", "bgzf")

    def __init__(self, eng, path, keep_qual=False, chunk_bytes=0):
        L = eng.L
        self.eng = eng
        h = C.c_void_p()
        rc = L.telr_reads_load(eng.h, str(path).encode(), 1 if keep_qual else 0, int(chunk_bytes), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_reads_load: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_last_error(eng.h).decode()), rc)
        self.h = h
        n = int(L.telr_reads_in_count(h))
        c = np.zeros(len(self.COUNTERS), np.int64); ci = np.zeros(len(self.CHUNK_INFO), np.int64); ph = np.zeros(len(self.PHASES), np.float32)
        L.telr_reads_in_counters(h, c.ctypes.data); L.telr_reads_in_chunk_info(h, ci.ctypes.data); L.telr_reads_in_phase_ms(h, ph.ctypes.data)
        self.counters = dict(zip(self.COUNTERS, (int(x) for x in c)))
        self.chunk_info = dict(zip(self.CHUNK_INFO, (int(x) for x in ci)))
        self.phase_ms = dict(zip(self.PHASES, (float(x) for x in ph)))
        self.n_bases = self.counters["bases"]
        self.container = self.CONTAINERS[self.counters["container"]]
        self.kind = None if self.counters["text_bytes"] == 0 else "fastq" if self.counters["fastq"] else "fasta"
        self.names_c = C.cast(L.telr_reads_in_names(h), C.POINTER(C.c_char_p * max(1, n))).contents if n else (C.c_char_p * 1)()
        self.qnames = [self.names_c[i].decode("latin-1") for i in range(n)]
        rs = SeqSet.__new__(SeqSet)
        rs.eng = eng; rs.len = _np_from(L.telr_reads_in_lens(h), n, np.int32); rs.n = n
        rs.h = C.c_void_p(L.telr_reads_in_detach_seqset(h))
        self.read_set = rs

    def free(self):
        """the handle and its names; the read set is the caller's (read_set.free())"""
        if getattr(self, "h", None):
            self.names_c = None
            self.eng.L.telr_reads_in_free(self.h); self.h = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _cstrs(ptr, n):
    if n == 0 or not ptr:
        return []
    return list((C.c_char_p * n).from_address(ptr))


class InsCalls:
    """what Index.call_insertions returns: calls (INS_CALL_DTYPE), sigs (INS_SIG_DTYPE, in key order; a call's `rep` indexes it),
    and the ascending distinct read ids of call i at reads[read_off[i]:read_off[i + 1]]"""
    def __init__(self, calls, sigs, read_off, reads):
        self.calls, self.sigs, self.read_off, self.reads = calls, sigs, read_off, reads

    def reads_of(self, i):
        return self.reads[self.read_off[i]:self.read_off[i + 1]]


class CohortSites:
    """what Engine.merge_sites returns: sites (COHORT_SITE_DTYPE, in final order, shadowed ones included), the input indices of site
    k's members in key order at members[member_off[k]:member_off[k + 1]], its ascending distinct sample numbers at
    samples[sample_off[k]:sample_off[k + 1]]"""
    def __init__(self, sites, member_off, members, sample_off, samples):
        self.sites, self.member_off, self.members, self.sample_off, self.samples = sites, member_off, members, sample_off, samples

    def members_of(self, k):
        return self.members[self.member_off[k]:self.member_off[k + 1]]

    def samples_of(self, k):
        return self.samples[self.sample_off[k]:self.sample_off[k + 1]]

    def site_list(self):
        """the sites that are not shadowed as an (n, 3) int32 array of (tid, pos, len), strictly ascending by (tid, pos): what
        Index.call_at_sites takes"""
        s = self.sites[(self.sites["flags"] & COHORT_SHADOWED) == 0]
        return np.stack([s["tid"], s["pos"], s["len"]], axis=1).astype(np.int32).reshape(-1, 3)


class InsGenotypes:
    """what Index.genotype_insertions returns: gt (GENO_DTYPE: ref, ambig, alt, gt with 0 = 0/0, 1 = 0/1, 2 = 1/1) per call, and the
    ascending distinct ids of call i's reference reads at ref_reads[ref_off[i]:ref_off[i + 1]], of its ambiguous reads likewise"""
    def __init__(self, gt, ref_off, ref_reads, ambig_off, ambig_reads):
        self.gt, self.ref_off, self.ref_reads, self.ambig_off, self.ambig_reads = gt, ref_off, ref_reads, ambig_off, ambig_reads

    def ref_reads_of(self, i):
        return self.ref_reads[self.ref_off[i]:self.ref_off[i + 1]]

    def ambig_reads_of(self, i):
        return self.ambig_reads[self.ambig_off[i]:self.ambig_off[i + 1]]


class Index:
    def __init__(self, eng, targets, io):
        self.eng = eng
        self.targets = targets if isinstance(targets, SeqSet) else SeqSet(eng, targets)
        self.io = io
        h = C.c_void_p()
        eng._chk(eng.L.telr_index_build(eng.h, self.targets.h, C.byref(io), C.byref(h)), "telr_index_build")
        self.h = h

    def stats(self):
        a, b = C.c_int64(0), C.c_int64(0)
        self.eng.L.telr_index_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def map_raw(self, queries, mo, qtarget=None):
        """-> opaque result handle (caller frees with free_raw)."""
        q = queries if isinstance(queries, SeqSet) else SeqSet(self.eng, queries)
        qt = None if qtarget is None else np.ascontiguousarray(qtarget, dtype=np.int32)
        r = C.c_void_p()
        self.eng._chk(self.eng.L.telr_map(self.eng.h, self.h, q.h, None if qt is None else qt.ctypes.data,
                                          C.byref(mo), C.byref(r)), "telr_map")
        return r

    def result_from_arrays(self, alns, cigars):
        """raw result handle over caller-held records + CIGAR words (copied): for the writers on records mapped elsewhere"""
        alns = np.ascontiguousarray(alns, dtype=ALN_DTYPE); cigars = np.ascontiguousarray(cigars, dtype=np.uint32)
        r = C.c_void_p()
        self.eng._chk(self.eng.L.telr_result_from_arrays(self.eng.h, alns.ctypes.data, len(alns), cigars.ctypes.data, len(cigars), C.byref(r)), "telr_result_from_arrays")
        return r

    def result_from_device_cigars(self, alns, cigars_t):
        """the same over CIGAR words that are on the device already (a torch int32 / uint8 tensor, e.g. what an all-to-all
        delivered): they become the result's device copy as they are (telr_result_from_device_cigars)"""
        import torch
        alns = np.ascontiguousarray(alns, dtype=ALN_DTYPE)
        t = cigars_t.contiguous()
        n = t.numel() * t.element_size() // 4
        torch.cuda.current_stream(t.device).synchronize()
        r = C.c_void_p()
        self.eng._chk(self.eng.L.telr_result_from_device_cigars(self.eng.h, alns.ctypes.data, len(alns), C.c_void_p(t.data_ptr() if n else 0), n, C.byref(r)),
                      "telr_result_from_device_cigars")
        return r

    def free_raw(self, r):
        self.eng.L.telr_result_free(r)

    # ---- one BAM written by N ranks: the slice of this rank (include/telr_hip.h: telr_write_bam_slice ...) ----
    def write_bam_slice(self, r, queries, qnames, tnames, emit, with_header, md=True, cs=True, softclip=True, rg=None, cmdline="telr_map", level=1, unmapped=True):
        """-> segment handle: the BGZF blocks of the records with emit[i] != 0 (+ the unmapped reads of `queries` when `unmapped`)
        as an image on the device; the other records only feed the SA tags"""
        qa, ta = self._cstr_array(qnames), self._cstr_array(tnames)
        flags = (1 if md else 0) | (2 if cs else 0) | (4 if softclip else 0) | (0 if unmapped else 8)
        rg_id, rg_sm, rg_lb = (None, None, None) if rg is None else tuple(x.encode() for x in rg)
        emit = np.ascontiguousarray(emit, dtype=np.uint8)
        seg = C.c_void_p()
        self.eng._chk(self.eng.L.telr_write_bam_slice(self.eng.h, r, queries.h, self.h, qa, ta, flags, rg_id, rg_sm, rg_lb, cmdline.encode(),
                                                      emit.ctypes.data, 1 if with_header else 0, level, C.byref(seg)), "telr_write_bam_slice")
        return seg

    def segment_info(self, seg):
        out = np.zeros(4, np.int64)
        self.eng._chk(self.eng.L.telr_bam_segment_info(seg, out.ctypes.data), "telr_bam_segment_info")
        return dict(zip(("bytes", "mapped_records", "unmapped_reads", "uncompressed_bytes"), (int(x) for x in out)))

    def segment_entries(self, seg, file_off):
        """-> (tid, start, end, virtual offset) arrays of the slice's mapped records in file order, and the virtual offset behind them"""
        n = self.segment_info(seg)["mapped_records"]
        tid, ts, te = (np.zeros(n, np.int32) for _ in range(3)); vb = np.zeros(n, np.uint64); v_end = C.c_uint64()
        self.eng._chk(self.eng.L.telr_bam_segment_entries(seg, int(file_off), tid.ctypes.data, ts.ctypes.data, te.ctypes.data, vb.ctypes.data, C.byref(v_end)), "telr_bam_segment_entries")
        return tid, ts, te, vb, int(v_end.value)

    def segment_write(self, seg, path, file_off, is_last):
        self.eng._chk(self.eng.L.telr_bam_segment_write(self.eng.h, seg, path.encode(), int(file_off), 1 if is_last else 0), "telr_bam_segment_write")

    def segment_free(self, seg):
        self.eng.L.telr_bam_segment_free(seg)

    def bai_write(self, path, tid, ts, te, vb, v_end, n_unmapped, tlens):
        tid, ts, te = (np.ascontiguousarray(x, np.int32) for x in (tid, ts, te)); vb = np.ascontiguousarray(vb, np.uint64); tl = np.ascontiguousarray(tlens, np.int32)
        self.eng._chk(self.eng.L.telr_bai_write(path.encode(), len(tid), tid.ctypes.data, ts.ctypes.data, te.ctypes.data, vb.ctypes.data, int(v_end), int(n_unmapped), len(tl), tl.ctypes.data), "telr_bai_write")

    def result_arrays(self, r):
        L = self.eng.L
        alns = _np_from(L.telr_result_alns(r), L.telr_result_count(r), ALN_DTYPE)
        cig = _np_from(L.telr_result_cigars(r), L.telr_result_cigar_count(r), np.uint32)
        return MapResult(alns, cig)

    def map(self, queries, mo, qtarget=None):
        r = self.map_raw(queries, mo, qtarget)
        try:
            return self.result_arrays(r)
        finally:
            self.free_raw(r)

    # ---- text emitters (the reference's own boundary: PAF / SAM files) -----------------------
    @staticmethod
    def _cstr_array(names):
        if isinstance(names, C.Array):          # already built (a caller that writes many files with the same names)
            return names
        arr = (C.c_char_p * max(1, len(names)))()
        for i, n in enumerate(names):
            arr[i] = n.encode() if isinstance(n, str) else bytes(n)
        return arr

    def write_paf(self, r, qnames, tnames, path, with_cigar=True, append=False):
        qa, ta = self._cstr_array(qnames), self._cstr_array(tnames)
        self.eng._chk(self.eng.L.telr_write_paf(r, qa, ta, 1 if with_cigar else 0, path.encode(), 1 if append else 0), "telr_write_paf")

    def write_sam(self, r, qnames, queries, tnames, targets, path, md=True, cs=True, softclip=True, rg=None, cmdline="telr_map",
                  primary_only=False, coordinate_sorted=False, header=True, unmapped=True, qual=None):
        """queries / targets: lists of sequences (str) or (buf, off, len) triples as given to seqset().
        qual: the queries' base qualities (a list of Phred + 33 strings or a (buffer, offsets) pair) for column 11; None: `*`.
        primary_only + coordinate_sorted + header=False = the text of `samtools view -F0x900 sorted.bam`
        (the polishing hand-off to wtpoa-cns, TELR_assembly.py:208,228)."""
        qb, qo, ql = queries if isinstance(queries, tuple) else concat(queries)
        tb, to, tl = targets if isinstance(targets, tuple) else concat(targets)
        qb = np.ascontiguousarray(qb, np.uint8); tb = np.ascontiguousarray(tb, np.uint8)
        qo = np.ascontiguousarray(qo, np.int64); to = np.ascontiguousarray(to, np.int64)
        ql = np.ascontiguousarray(ql, np.int32); tl = np.ascontiguousarray(tl, np.int32)
        qa, ta = self._cstr_array(qnames), self._cstr_array(tnames)
        flags = (1 if md else 0) | (2 if cs else 0) | (4 if softclip else 0) | (0 if unmapped else 8) | (16 if primary_only else 0) | \
            (32 if coordinate_sorted else 0) | (0 if header else 64)
        rg_id, rg_sm, rg_lb = (None, None, None) if rg is None else tuple(x.encode() for x in rg)
        if qual is None:
            self.eng._chk(self.eng.L.telr_write_sam(r, len(ql), qa, qb.ctypes.data, qo.ctypes.data, ql.ctypes.data, len(tl), ta,
                                                    tb.ctypes.data, to.ctypes.data, tl.ctypes.data, flags, rg_id, rg_sm, rg_lb,
                                                    cmdline.encode(), path.encode()), "telr_write_sam")
        else:
            qq, qqo = _qual_arrays(qual)
            self.eng._chk(self.eng.L.telr_write_sam_qual(r, len(ql), qa, qb.ctypes.data, qo.ctypes.data, ql.ctypes.data, len(tl), ta,
                                                         tb.ctypes.data, to.ctypes.data, tl.ctypes.data, flags, rg_id, rg_sm, rg_lb,
                                                         cmdline.encode(), path.encode(), qq.ctypes.data, qqo.ctypes.data, 33), "telr_write_sam_qual")

    def write_bam(self, r, qnames, queries, tnames, targets, path, md=True, cs=True, softclip=True, rg=None, cmdline="telr_map",
                  index=True, level=1, qual=None):
        """coordinate-sorted BAM + .bai (samtools sort + index, TELR_alignment.py:103-114); qual as in write_sam (None: QUAL 0xff)"""
        qb, qo, ql = queries if isinstance(queries, tuple) else concat(queries)
        tb, to, tl = targets if isinstance(targets, tuple) else concat(targets)
        qb = np.ascontiguousarray(qb, np.uint8); tb = np.ascontiguousarray(tb, np.uint8)
        qo = np.ascontiguousarray(qo, np.int64); to = np.ascontiguousarray(to, np.int64)
        ql = np.ascontiguousarray(ql, np.int32); tl = np.ascontiguousarray(tl, np.int32)
        qa, ta = self._cstr_array(qnames), self._cstr_array(tnames)
        flags = (1 if md else 0) | (2 if cs else 0) | (4 if softclip else 0)
        rg_id, rg_sm, rg_lb = (None, None, None) if rg is None else tuple(x.encode() for x in rg)
        if qual is None:
            self.eng._chk(self.eng.L.telr_write_bam(r, len(ql), qa, qb.ctypes.data, qo.ctypes.data, ql.ctypes.data, len(tl), ta,
                                                    tb.ctypes.data, to.ctypes.data, tl.ctypes.data, flags, rg_id, rg_sm, rg_lb,
                                                    cmdline.encode(), path.encode(), 1 if index else 0, level), "telr_write_bam")
        else:
            qq, qqo = _qual_arrays(qual)
            self.eng._chk(self.eng.L.telr_write_bam_qual(r, len(ql), qa, qb.ctypes.data, qo.ctypes.data, ql.ctypes.data, len(tl), ta,
                                                         tb.ctypes.data, to.ctypes.data, tl.ctypes.data, flags, rg_id, rg_sm, rg_lb,
                                                         cmdline.encode(), path.encode(), 1 if index else 0, level, qq.ctypes.data, qqo.ctypes.data, 33), "telr_write_bam_qual")

    def write_bam_device(self, r, queries, qnames, tnames, path, md=True, cs=True, softclip=True, rg=None, cmdline="telr_map",
                         index=True, level=1, unmapped=True):
        """the same file built on the device from the resident reads / reference / CIGARs (telr_write_bam_dev);
        queries = the SeqSet the result was mapped from; its attached qualities, if any, become QUAL"""
        qa, ta = self._cstr_array(qnames), self._cstr_array(tnames)
        flags = (1 if md else 0) | (2 if cs else 0) | (4 if softclip else 0) | (0 if unmapped else 8)
        rg_id, rg_sm, rg_lb = (None, None, None) if rg is None else tuple(x.encode() for x in rg)
        self._write_bam_dev(r, queries, qa, ta, flags, rg_id, rg_sm, rg_lb, cmdline.encode(), path.encode(), 1 if index else 0, level)

    def _write_bam_dev(self, r, queries, *rest):
        self.eng._chk(self.eng.L.telr_write_bam_dev(self.eng.h, r, queries.h, self.h, *rest), "telr_write_bam_dev")

    def bam_prepare(self, path, est_bytes):
        """start creating the output file in the background (call before map_raw; see telr_bam_prepare)"""
        self.eng._chk(self.eng.L.telr_bam_prepare(self.eng.h, path.encode(), int(est_bytes)), "telr_bam_prepare")

    def bam_discard(self):
        """drop a prepared output file that will not be written (telr_bam_discard; the caller unlinks the file)"""
        if getattr(self.eng, "h", None):
            self.eng.L.telr_bam_discard(self.eng.h)

    def bam_release_wait(self):
        """wait until the mappings of earlier output files are taken apart (telr_bam_release_wait)"""
        self.eng.L.telr_bam_release_wait()

    def bam_stage_ms(self):
        a = np.zeros(8, np.float32); b = np.zeros(12, np.float32)
        self.eng.L.telr_debug_bam_ms(a.ctypes.data); self.eng.L.telr_debug_bam_sink_ms(b.ctypes.data)
        d = dict(zip(("upload", "scan_size", "sort_offsets", "write_records", "bgzf", "d2h_file", "bai_host_overlapped", "total"), (float(x) for x in a)))
        d.update(zip(("sink_allocate_bg", "sink_map_bg", "sink_wait", "sink_mapping_used", "stream_wait_coder", "stream_wait_dma", "stream_host_copy", "stream_wait_slot", "stream_loop", "sink_stop", "sink_truncate"), (float(x) for x in b)))
        return d

    def consensus(self, r, queries, min_depth=3, poa=False):
        """consensus of this index's targets from the primary records of raw result r -> list of str: the pile-up vote
        (telr_consensus_build) or, poa=True, the window partial-order consensus (telr_poa_build)"""
        h = C.c_void_p()
        fn, what = (self.eng.L.telr_poa_build, "telr_poa_build") if poa else (self.eng.L.telr_consensus_build, "telr_consensus_build")
        self.eng._chk(fn(self.eng.h, r, queries.h, self.h, int(min_depth), C.byref(h)), what)
        try:
            L = self.eng.L
            n = int(L.telr_consensus_count(h))
            off = _np_from(L.telr_consensus_off(h), n, np.int64); ln = _np_from(L.telr_consensus_len(h), n, np.int32)
            tot = int(off[-1] + ln[-1]) if n else 0
            buf = _np_from(L.telr_consensus_seq(h), tot, np.uint8)
            return [bytes(buf[off[i]:off[i] + ln[i]]).decode() for i in range(n)]
        finally:
            self.eng.L.telr_consensus_free(h)

    def depth_medians(self, r, iv_tid, iv_s, iv_e):
        """Medians over 0-based inclusive intervals, from a raw result handle."""
        tl = self.targets.len
        a, b, c = (np.ascontiguousarray(x, dtype=np.int32) for x in (iv_tid, iv_s, iv_e))
        out = np.zeros(len(a), np.float64)
        self.eng._chk(self.eng.L.telr_depth_medians(self.eng.h, r, len(tl), tl.ctypes.data, len(a), a.ctypes.data,
                                                    b.ctypes.data, c.ctypes.data, out.ctypes.data), "telr_depth_medians")
        return out

    def call_insertions(self, r, opt=None):
        """insertion candidates of raw result r (telr_call_insertions; include/telr_hip.h has the definition): opt an
        _abi.InsOpt (None: the defaults) -> InsCalls: calls / sigs as numpy structured arrays, read_off / reads the calls' read ids"""
        o = InsOpt.default() if opt is None else opt
        h = C.c_void_p()
        rc = self.eng.L.telr_call_insertions(self.eng.h, r, self.targets.n, C.byref(o), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_call_insertions: %s [%s]" % (self.eng.L.telr_strerror(rc).decode(), self.eng.L.telr_last_error(self.eng.h).decode()), rc)
        return self._ins_calls(h)

    def call_at_sites(self, r, sites, opt=None, site_opt=None):
        """the supporters of the insertion sites the caller names, on raw result r (telr_call_at_sites; include/telr_hip.h has the
        definition, which is not Sniffles' forced genotyping): sites an (n, 3) int32 array or a list of (tid, pos, len) triples,
        strictly ascending by (tid, pos), len = the expected insertion length or 0; opt an _abi.InsOpt, site_opt an _abi.SiteOpt
        (None: the defaults) -> InsCalls with one call per site in site order, whatever its support, and only the kept signatures:
        what genotype_insertions takes"""
        o = InsOpt.default() if opt is None else opt
        so = SiteOpt.default() if site_opt is None else site_opt
        s = np.ascontiguousarray(np.asarray(sites, dtype=np.int32).reshape(-1, 3))
        h = C.c_void_p()
        rc = self.eng.L.telr_call_at_sites(self.eng.h, r, self.targets.n, C.byref(o), s.ctypes.data if len(s) else None, len(s), C.byref(so), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_call_at_sites: %s [%s]" % (self.eng.L.telr_strerror(rc).decode(), self.eng.L.telr_last_error(self.eng.h).decode()), rc)
        return self._ins_calls(h)

    def _ins_calls(self, h):
        """a telr_ins_calls handle copied into an InsCalls, and freed"""
        try:
            L = self.eng.L
            nc, ns = int(L.telr_ins_calls_count(h)), int(L.telr_ins_calls_sig_count(h))
            read_off = _np_from(L.telr_ins_calls_read_off(h), nc + 1, np.int64)
            return InsCalls(_np_from(L.telr_ins_calls_calls(h), nc, INS_CALL_DTYPE), _np_from(L.telr_ins_calls_sigs(h), ns, INS_SIG_DTYPE),
                            read_off, _np_from(L.telr_ins_calls_reads(h), int(read_off[-1]), np.int32))
        finally:
            self.eng.L.telr_ins_calls_free(h)

    def genotype_insertions(self, r, ic, opt=None):
        """reference reads, ambiguous reads and GT of the calls `ic` (an InsCalls of call_insertions, or anything with calls /
        read_off / reads of that form) on raw result r (telr_genotype_insertions; include/telr_hip.h has the definition, which is
        not Sniffles'): opt an _abi.GenoOpt (None: the defaults) -> InsGenotypes"""
        o = GenoOpt.default() if opt is None else opt
        calls, read_off, reads, _ = _ic_arrays("telr_genotype_insertions", ic)
        h = C.c_void_p()
        rc = self.eng.L.telr_genotype_insertions(self.eng.h, r, self.targets.n, len(calls), calls.ctypes.data, read_off.ctypes.data, reads.ctypes.data,
                                                 C.byref(o), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_genotype_insertions: %s [%s]" % (self.eng.L.telr_strerror(rc).decode(), self.eng.L.telr_last_error(self.eng.h).decode()), rc)
        try:
            L = self.eng.L
            nc = int(L.telr_ins_geno_count(h))
            ref_off = _np_from(L.telr_ins_geno_ref_off(h), nc + 1, np.int64)
            ambig_off = _np_from(L.telr_ins_geno_ambig_off(h), nc + 1, np.int64)
            return InsGenotypes(_np_from(L.telr_ins_geno_gt(h), nc, GENO_DTYPE), ref_off, _np_from(L.telr_ins_geno_ref_reads(h), int(ref_off[-1]), np.int32),
                                ambig_off, _np_from(L.telr_ins_geno_ambig_reads(h), int(ambig_off[-1]), np.int32))
        finally:
            self.eng.L.telr_ins_geno_free(h)

    def draft_contigs(self, r, ic, read_set, opt=None):
        """a draft contig per call of `ic` (an InsCalls of call_insertions on raw result r: calls, sigs, read_off, reads), cut out of
        one of the call's supporting reads on the device (telr_draft_contigs; include/telr_hip.h has the definition -- not an assembler):
        read_set the SeqSet r was mapped from, opt an _abi.DraftOpt (None: the defaults) -> (drafts, set): one DRAFT_DTYPE record per
        call (sig = set_index = -1: no draft) and the SeqSet of the drafts, in call order, on the reference strand"""
        o = DraftOpt.default() if opt is None else opt
        calls, read_off, reads, sigs = _ic_arrays("telr_draft_contigs", ic, True)
        h, hs = C.c_void_p(), C.c_void_p()
        L = self.eng.L
        rc = L.telr_draft_contigs(self.eng.h, r, self.targets.n, len(calls), calls.ctypes.data, read_off.ctypes.data, reads.ctypes.data,
                                  len(sigs), sigs.ctypes.data, read_set.h, C.byref(o), C.byref(h), C.byref(hs))
        if rc != 0:
            raise _lib.TelrError("telr_draft_contigs: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_last_error(self.eng.h).decode()), rc)
        try:
            drafts = _np_from(L.telr_drafts_data(h), int(L.telr_drafts_count(h)), DRAFT_DTYPE)
        finally:
            L.telr_draft_contigs_free(h)
        out = SeqSet.__new__(SeqSet)
        out.eng = self.eng; out.h = hs
        out.len = np.ascontiguousarray(drafts["len"][drafts["sig"] >= 0], dtype=np.int32); out.n = len(out.len)
        return drafts, out

    def bridge_contigs(self, r, ic, read_set, opt=None, want=None):
        """a bridge of two reads per call of `ic` that no single read spans (telr_bridge_contigs; include/telr_hip.h has the definition --
        not an assembler): a read entering the insertion from the left and one entering it from the right, joined at one shared k-mer of
        their clips.  read_set the SeqSet r was mapped from, opt an _abi.BridgeOpt (None: the defaults), want one flag per call (None:
        every call) -> one BRIDGE_DTYPE record per call (sig_l = sig_r = -1: no bridge).  Records only: SeqSet.join makes the sequences
        of the two pieces (qid_l, start_l, len_l, rc_l) and (qid_r, start_r, len_r, rc_r)."""
        o = BridgeOpt.default() if opt is None else opt
        calls, read_off, reads, sigs = _ic_arrays("telr_bridge_contigs", ic, True)
        if want is not None:
            want = np.ascontiguousarray(np.asarray(want) != 0, dtype=np.uint8)
            if len(want) != len(calls):
                raise _lib.TelrError("telr_bridge_contigs: one want flag per call")
        h = C.c_void_p()
        L = self.eng.L
        rc = L.telr_bridge_contigs(self.eng.h, r, self.targets.n, len(calls), calls.ctypes.data, read_off.ctypes.data, reads.ctypes.data,
                                   len(sigs), sigs.ctypes.data, read_set.h, None if want is None else want.ctypes.data, C.byref(o), C.byref(h))
        if rc != 0:
            raise _lib.TelrError("telr_bridge_contigs: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_last_error(self.eng.h).decode()), rc)
        try:
            return _np_from(L.telr_bridges_data(h), int(L.telr_bridges_count(h)), BRIDGE_DTYPE)
        finally:
            L.telr_bridge_contigs_free(h)

    # ---- debug taps for the stage-level parity tests ----------------------------------
    def debug_dump(self):
        L = self.eng.L
        n_mz, n_ent = self.stats()
        eh = np.zeros(n_ent, np.uint64); eo = np.zeros(n_ent + 1, np.uint32); pos = np.zeros(n_mz, np.uint32)
        self.eng._chk(L.telr_debug_index(self.eng.h, self.h, eh.ctypes.data, eo.ctypes.data, pos.ctypes.data), "debug_index")
        return eh, eo, pos

    def debug_mid_occ(self, mo):
        return int(self.eng.L.telr_debug_mid_occ(self.h, C.byref(mo)))

    def debug_dp(self, queries, mo, probs):
        """Engine.debug_dp against this index's targets"""
        q = queries if isinstance(queries, SeqSet) else SeqSet(self.eng, queries)
        return self.eng.debug_dp(q, self.targets, mo, probs)

    def debug_last_batch(self, nq):
        L = self.eng.L
        na = int(L.telr_debug_n_anchor(self.eng.h))
        out = {}
        for name, dt, n in (("skeys", np.uint64, na), ("chain_f", np.int32, na), ("chain_p", np.int32, na), ("q_aoff", np.int32, nq + 1)):
            a = np.zeros(n, dt)
            if n:
                self.eng._chk(L.telr_debug_fetch(self.eng.h, name.encode(), a.ctypes.data, a.nbytes), "debug_fetch " + name)
            out[name] = a
        nc = int(L.telr_debug_n_chain(self.eng.h))
        out["chains"] = _np_from(L.telr_debug_chains(self.eng.h), nc * 9, np.int32).reshape(-1, 9)
        return out

    def free(self):
        if getattr(self, "h", None):
            if _DEFERRED is not None:
                _DEFERRED.append((self.eng.L.telr_index_free, self.h))
            else:
                self.eng.L.telr_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PartIndex(Index):
    """An index over a target set of any total size: one Index per part (Engine.part_plan), the reads mapped against every part in turn
    and the per-part results merged on the device (telr_merge_parts; include/telr_hip.h has the definition).  `targets` is the full
    resident set and the merged result carries global target ids, so call_insertions, call_at_sites, genotype_insertions, draft_contigs,
    bridge_contigs, depth_medians, result_arrays, write_bam_device and the text writers work as on an Index.  Not for a multi-part index: qtarget /
    MF_PER_TARGET, write_bam_slice, consensus, the debug taps.  All part indexes are resident together, and during a map the part
    results and the merged one live side by side."""

    def __init__(self, eng, targets, io, max_part_bases=0, like=None):
        self.eng = eng
        self.io = io
        self.h = None
        self.parts = []
        self.max_part_bases = int(max_part_bases)
        if like is not None:
            if not isinstance(like, PartIndex) or like.max_part_bases != self.max_part_bases:
                raise ValueError("index_parts: like= must be a PartIndex cut with the same max_part_bases")
            self.targets, self.part_of, self.part_sets, self._owner = like.targets, like.part_of, like.part_sets, like
        else:
            self.targets = targets if isinstance(targets, SeqSet) else SeqSet(eng, targets)
            self.part_of = Engine.part_plan(self.targets.len, self.max_part_bases)
            self._owner = None
            self.part_sets = []
        n_parts = int(self.part_of.max()) + 1 if len(self.part_of) else 0
        self.tid_maps = [np.ascontiguousarray(np.flatnonzero(self.part_of == p), dtype=np.int32) for p in range(n_parts)]
        try:
            if like is None:
                for m in self.tid_maps:
                    self.part_sets.append(self.targets.subset(m))
            for sub in self.part_sets:
                self.parts.append(Index(eng, sub, io))
        except BaseException:
            self.free()
            raise

    @property
    def n_parts(self):
        return len(self.parts)

    def stats(self):
        a = [ix.stats() for ix in self.parts]
        return sum(x[0] for x in a), sum(x[1] for x in a)

    def map_raw(self, queries, mo, qtarget=None):
        """-> opaque handle of the merged result (caller frees with free_raw); its CIGAR words are resident on the device"""
        if qtarget is not None or (mo.flags & MF_PER_TARGET):
            raise _lib.TelrError("PartIndex.map_raw: qtarget / TELR_MF_PER_TARGET are not for a multi-part index", TELR_E_ARG)
        q = queries if isinstance(queries, SeqSet) else SeqSet(self.eng, queries)
        mp = mo.copy(); mp.flags |= MF_KEEP_CIGARS
        raws = []
        try:
            for ix in self.parts:
                raws.append(ix.map_raw(q, mp))
            return self.merge_raw(raws, q.n, mo)
        finally:
            for r in raws:
                self.free_raw(r)

    def merge_raw(self, raws, n_queries, mo):
        """telr_merge_parts over one raw result per part (in part order) -> the merged handle; the part results stay the caller's"""
        n = len(raws)
        if n != len(self.parts):
            raise ValueError("merge_raw: one result per part")
        ra = (C.c_void_p * max(1, n))(*[r.value if isinstance(r, C.c_void_p) else r for r in raws])
        ma = (C.c_void_p * max(1, n))(*[m.ctypes.data for m in self.tid_maps])
        nt = np.ascontiguousarray([len(m) for m in self.tid_maps], dtype=np.int32)
        out = C.c_void_p()
        L = self.eng.L
        rc = L.telr_merge_parts(self.eng.h, n, ra, ma, nt.ctypes.data if n else None, int(n_queries), C.byref(mo), C.byref(out))
        if rc != 0:
            raise _lib.TelrError("telr_merge_parts: %s [%s]" % (L.telr_strerror(rc).decode(), L.telr_last_error(self.eng.h).decode()), rc)
        return out

    def _write_bam_dev(self, r, queries, *rest):
        """the writer reads nothing of an index but its targets: the full set stands in (telr_write_bam_dev_targets)"""
        self.eng._chk(self.eng.L.telr_write_bam_dev_targets(self.eng.h, r, queries.h, self.targets.h, *rest), "telr_write_bam_dev_targets")

    def _not_here(self, what):
        raise _lib.TelrError("%s is not for a multi-part index" % what, TELR_E_ARG)

    def write_bam_slice(self, *a, **k):
        self._not_here("write_bam_slice")

    def consensus(self, *a, **k):
        self._not_here("consensus")

    def debug_dump(self):
        self._not_here("debug_dump")

    def debug_mid_occ(self, mo):
        self._not_here("debug_mid_occ")

    def free(self):
        for ix in getattr(self, "parts", []):
            ix.free()
        self.parts = []
        if getattr(self, "_owner", None) is None:
            for s in getattr(self, "part_sets", []):
                s.free()
            self.part_sets = []
