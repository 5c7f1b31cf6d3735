"""ctypes mirrors of the plain-C structs declared in include/telr_hip.h."""
import ctypes as C


class IdxOpt(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("is_hpc", C.c_int32), ("bucket_bits", C.c_int32)]


class MapOpt(C.Structure):
    _fields_ = [
        ("mid_occ_frac", C.c_float), ("min_mid_occ", C.c_int32), ("max_mid_occ", C.c_int32),
        ("max_gap", C.c_int32), ("bw", C.c_int32), ("chain_lookback", C.c_int32), ("min_cnt", C.c_int32),
        ("min_chain_score", C.c_int32), ("chain_gap_q8", C.c_int32), ("chain_skip_q8", C.c_int32),
        ("mask_level", C.c_float), ("pri_ratio", C.c_float), ("best_n", C.c_int32), ("secondary", C.c_int32),
        ("a", C.c_int32), ("b", C.c_int32), ("q", C.c_int32), ("e", C.c_int32), ("q2", C.c_int32), ("e2", C.c_int32),
        ("sc_ambi", C.c_int32), ("zdrop", C.c_int32), ("min_dp_max", C.c_int32), ("min_ksw_len", C.c_int32),
        ("ext_max", C.c_int32), ("ext_band", C.c_int32), ("flags", C.c_int32), ("fill_band_q4", C.c_int32), ("fill_margin", C.c_int32),
        ("vote_len", C.c_int32), ("vote_bin_shift", C.c_int32), ("vote_min", C.c_int32), ("vote_frac_q8", C.c_int32), ("bw_long", C.c_int32),
        ("cx_scale", C.c_int32), ("cx_open", C.c_int32), ("cx_ext_max", C.c_int32), ("cx_ext_min", C.c_int32), ("cx_decay", C.c_int32),
    ]

    def copy(self):
        o = MapOpt()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(MapOpt))
        return o


class Aln(C.Structure):
    _fields_ = [
        ("qid", C.c_int32), ("tid", C.c_int32), ("qlen", C.c_int32), ("qs", C.c_int32), ("qe", C.c_int32),
        ("tlen", C.c_int32), ("ts", C.c_int32), ("te", C.c_int32), ("mlen", C.c_int32), ("blen", C.c_int32),
        ("score", C.c_int32), ("subsc", C.c_int32), ("dp_score", C.c_int32), ("cnt", C.c_int32),
        ("n_sub", C.c_int32), ("parent", C.c_int32), ("n_cigar", C.c_int32), ("flags", C.c_int32),
        ("cigar_off", C.c_int64), ("mapq", C.c_int32), ("n_ambi", C.c_int32),
    ]


class InsOpt(C.Structure):
    """telr_ins_opt: the options of telr_call_insertions (defaults: InsOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("min_len", "min_mapq", "min_clip", "max_ref_gap", "cluster_dist", "min_support", "min_sized", "reserved")]

    @classmethod
    def default(cls, **kw):
        o = cls(50, 20, 200, 200, 50, 10, 1, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("InsOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class SiteOpt(C.Structure):
    """telr_site_opt: the options of telr_call_at_sites (defaults: SiteOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("reach", "len_pct", "reserved0", "reserved1")]

    @classmethod
    def default(cls, **kw):
        o = cls(50, 0, 0, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("SiteOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class InsSite(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "pos", "len")]


class CohortOpt(C.Structure):
    """telr_cohort_opt: the options of telr_merge_sites (defaults: CohortOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("dist", "min_samples", "reserved0", "reserved1")]

    @classmethod
    def default(cls, **kw):
        o = cls(50, 1, 0, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("CohortOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class CohortEntry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "pos", "len", "sample", "group")]


class CohortSite(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "pos", "len", "group", "n_samples", "n_members", "n_sized", "len_min", "len_max", "pos_min", "pos_max",
                                         "rep", "flags", "winner")]


class InsSig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "pos", "len", "qid", "kind", "rec", "mate", "seg_start", "seg_len")]


class InsCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "pos", "len", "support", "n_sized", "rep")]


class GenoOpt(C.Structure):
    """telr_geno_opt: the options of telr_genotype_insertions (defaults: GenoOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("flank", "min_mapq", "max_window_indel", "het_pct", "hom_pct", "reserved0", "reserved1", "reserved2")]

    @classmethod
    def default(cls, **kw):
        o = cls(50, 20, 20, 30, 80, 0, 0, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("GenoOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class InsGt(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ref", "ambig", "alt", "gt")]


class DraftOpt(C.Structure):
    """telr_draft_opt: the options of telr_draft_contigs (defaults: DraftOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("flank", "min_flank", "reach", "max_len", "reserved0", "reserved1", "reserved2", "reserved3")]

    @classmethod
    def default(cls, **kw):
        o = cls(2000, 500, 50, 100000, 0, 0, 0, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("DraftOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class Draft(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sig", "qid", "start", "len", "rc", "ins_off", "ins_len", "set_index")]


class BridgeOpt(C.Structure):
    """telr_bridge_opt: the options of telr_bridge_contigs (defaults: BridgeOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("flank", "min_flank", "reach", "max_len", "k", "window", "min_votes", "pairs")]

    @classmethod
    def default(cls, **kw):
        o = cls(2000, 500, 50, 100000, 13, 4096, 8, 4)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("BridgeOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class Bridge(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sig_l", "sig_r", "qid_l", "start_l", "len_l", "rc_l", "qid_r", "start_r", "len_r", "rc_r",
                                         "votes", "diag", "ins_off", "ins_len", "n_left", "n_right")]


class RefTeOpt(C.Structure):
    """telr_refte_opt: the options of telr_annotate_hits (defaults: RefTeOpt.default())"""
    _fields_ = [(n, C.c_int32) for n in ("min_len", "min_mapq", "join_gap", "reserved")]

    @classmethod
    def default(cls, **kw):
        o = cls(100, 0, 0, 0)
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError("RefTeOpt has no field %r" % k)
            setattr(o, k, int(v))
        return o


class Tile(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "start", "len")]


class TeFeat(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "start", "end", "family", "strand", "score", "n_hits")]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "query_bases", "minimizers", "probes", "anchors", "chains", "dp_problems", "dp_cells",
        "window_bases", "cigar_ops", "records", "over_queries", "over_ranges")]


# return codes (include/telr_hip.h)
TELR_OK, TELR_E_NODEVICE, TELR_E_HIP, TELR_E_ARG, TELR_E_RANGE, TELR_E_NOMEM, TELR_E_IO = 0, -1, -2, -3, -4, -5, -6
F_PRIMARY, F_SECONDARY, F_SUPPL, F_REV = 1, 2, 4, 8
MF_CIGAR, MF_PER_TARGET, MF_FAITHFUL, MF_KEEP_CIGARS = 1, 2, 4, 8
MF_CHAIN_SKIP = 0x1000          # minimap2's chaining scan (max_chain_iter 5000, max_chain_skip 25); overrides chain_lookback
MF_SEED_RESCUE = 0x2000         # minimap2's high-occurrence seed rescue (mm_seed_select: one seed per 500 bases of a skipped stretch)
MF_MM2_MAPQ = 0x20000           # minimap2's MAPQ (mm_set_mapq without the second-best DP score) instead of the Li-2018 formula
N_STAGES = 16
N_DPCLS = 25
# the rows of the two test taps behind the DP (include/telr_hip.h: telr_debug_stitch, telr_debug_align)
STITCH_PROB_COLUMNS = ("score", "bi", "bj", "mlen", "mcols")
STITCH_CHAIN_COLUMNS = ("dp", "mlen", "blen", "l_bi", "l_bj", "r_bi", "r_bj", "n_cigar", "cig_first")
ALIGN_CHAIN_IN_COLUMNS = ("qid", "tid", "rev", "qs", "qe", "rs", "re")
ALIGN_CHAIN_COLUMNS = ("qs", "qe", "ts", "te", "mlen", "blen", "dp_score", "n_cigar", "cig_first")
ALIGN_PROB_COLUMNS = ("cls", "retried", "score", "bi", "bj", "mlen", "mcols", "nops", "cells")

import numpy as _np

ALN_DTYPE = _np.dtype([(n, _np.int64 if t is C.c_int64 else _np.int32) for n, t in Aln._fields_], align=True)
assert ALN_DTYPE.itemsize == C.sizeof(Aln) == 88, (ALN_DTYPE.itemsize, C.sizeof(Aln))
INS_SIG_DTYPE = _np.dtype([(n, _np.int32) for n, _ in InsSig._fields_])
INS_CALL_DTYPE = _np.dtype([(n, _np.int32) for n, _ in InsCall._fields_])
assert INS_SIG_DTYPE.itemsize == C.sizeof(InsSig) == 36 and INS_CALL_DTYPE.itemsize == C.sizeof(InsCall) == 24
INS_SITE_DTYPE = _np.dtype([(n, _np.int32) for n, _ in InsSite._fields_])
assert INS_SITE_DTYPE.itemsize == C.sizeof(InsSite) == 12 and C.sizeof(SiteOpt) == 16
COHORT_ENTRY_DTYPE = _np.dtype([(n, _np.int32) for n, _ in CohortEntry._fields_])
COHORT_SITE_DTYPE = _np.dtype([(n, _np.int32) for n, _ in CohortSite._fields_])
assert COHORT_ENTRY_DTYPE.itemsize == C.sizeof(CohortEntry) == 20 and COHORT_SITE_DTYPE.itemsize == C.sizeof(CohortSite) == 56 and C.sizeof(CohortOpt) == 16
COHORT_SHADOWED, COHORT_CROWDED = 1, 2          # TELR_COHORT_* (telr_cohort_site.flags)
GENO_DTYPE = _np.dtype([(n, _np.int32) for n, _ in InsGt._fields_])
assert GENO_DTYPE.itemsize == C.sizeof(InsGt) == 16 and C.sizeof(GenoOpt) == 32
DRAFT_DTYPE = _np.dtype([(n, _np.int32) for n, _ in Draft._fields_])
assert DRAFT_DTYPE.itemsize == C.sizeof(Draft) == 32 and C.sizeof(DraftOpt) == 32
BRIDGE_DTYPE = _np.dtype([(n, _np.int32) for n, _ in Bridge._fields_])
assert BRIDGE_DTYPE.itemsize == C.sizeof(Bridge) == 64 and C.sizeof(BridgeOpt) == 32
TILE_DTYPE = _np.dtype([(n, _np.int32) for n, _ in Tile._fields_])
TE_FEAT_DTYPE = _np.dtype([(n, _np.int32) for n, _ in TeFeat._fields_])
assert TILE_DTYPE.itemsize == C.sizeof(Tile) == 12 and TE_FEAT_DTYPE.itemsize == C.sizeof(TeFeat) == 28 and C.sizeof(RefTeOpt) == 16
