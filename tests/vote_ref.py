"""Sub-read voting restated in plain numpy from the words of include/telr_hip.h (vote_len .. vote_frac_q8) and DESIGN's spec 3.10:

    The hits of the minimizers whose last base lies in query bases [s * vote_len, (s + 1) * vote_len) vote into diagonal bins of
    2^vote_bin_shift bases (per strand; 1,024 bins, folded); a hit stays an anchor iff its bin and the two next to it hold at least
    max(vote_min, ceil(vote_frac_q8 / 256 * votes of the sub-read's fullest bin)) hits.

Input: the anchor keys of ONE query before voting (rev << 63 | reference position << 32 | strand-adjusted query position << 8 |
span: the position is that of the minimizer's last base; for a reverse hit the query position is counted from the read's other end,
qlen - (qpos + 1 - span) - 1), the query's length and the options.  No table walk, no chunks, no caps: one pass with np.add.at."""
import numpy as np

BINS = 1024


def fields(keys):
    """-> (rev, gp, qadj, span) of every key, int64"""
    k = np.asarray(keys, np.uint64)
    rev = (k >> np.uint64(63)).astype(np.int64)
    gp = ((k >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(np.int64)
    qadj = ((k >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.int64)
    span = (k & np.uint64(0xff)).astype(np.int64)
    return rev, gp, qadj, span


def forward_qpos(keys, qlen):
    """the forward position of the minimizer's last base: a reverse key holds qadj = qlen - (qpos + 1 - span) - 1"""
    rev, _, qadj, span = fields(keys)
    return np.where(rev == 1, qlen - 2 + span - qadj, qadj)


def sub_read(keys, qlen, vote_len):
    return forward_qpos(keys, qlen) // vote_len


def bins(keys, shift):
    """the folded diagonal bin of every key (per strand: a bin number means a different bin on the other strand)"""
    _, gp, qadj, _ = fields(keys)
    return (((gp - qadj + (1 << 24)) & 0xffffffff) >> shift) & (BINS - 1)


def tables(keys, qlen, mo):
    """-> (sub-read ids in order, table[n_sub, 2, 1024] of votes, the row of every key)"""
    rev = fields(keys)[0]
    sub = sub_read(keys, qlen, mo.vote_len)
    ids, row = np.unique(sub, return_inverse=True)
    tab = np.zeros((len(ids), 2, BINS), np.int64)
    np.add.at(tab, (row, rev, bins(keys, mo.vote_bin_shift)), 1)
    return ids, tab, row


def thresholds(tab, mo):
    """per sub-read: max(vote_min, ceil(vote_frac_q8 * fullest / 256)); the fullest bin of either strand"""
    vmax = tab.reshape(len(tab), -1).max(axis=1) if len(tab) else np.zeros(0, np.int64)
    return np.maximum(int(mo.vote_min), -((-int(mo.vote_frac_q8) * vmax) // 256)), vmax


def three(tab):
    """votes of every bin plus its two same-strand neighbours, folded"""
    return tab + np.roll(tab, 1, axis=2) + np.roll(tab, -1, axis=2)


def survivors_mask(keys, qlen, mo):
    keys = np.asarray(keys, np.uint64)
    if len(keys) == 0:
        return np.zeros(0, bool)
    _, tab, row = tables(keys, qlen, mo)
    thr, _ = thresholds(tab, mo)
    s3 = three(tab)
    return s3[row, fields(keys)[0], bins(keys, mo.vote_bin_shift)] >= thr[row]


def vote(keys, qlen, mo):
    """the keys that stay, sorted"""
    keys = np.asarray(keys, np.uint64)
    return np.sort(keys[survivors_mask(keys, qlen, mo)])
