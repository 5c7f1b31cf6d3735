"""Edge tables and plain numpy references for the two primitives the engine's stages stand on: the LSD radix sort (radix.hip.h:
radix_sort_passes, reached through Engine.debug_radix_sort) and the tiled exclusive scan (kernels.hip.h: k_qscan_sums / k_qscan_write
behind dev_qscan, reached through Engine.debug_qscan).  tests/test_prim_ref.py shows on a CPU that every case reaches the edge it
names; tests/test_gpu_prims.py holds the kernels to the references, exactly."""
import numpy as np

# ---- the sort -------------------------------------------------------------------------------------------------------------------------
RS_TILE = 2048                    # keys per workgroup of k_rs_hist / k_rs_scatter
RS_ROW = 256                      # threads of k_rs_scan: above 256 tiles a thread owns two entries of a digit's row

# key count -> the tiles it claims.  2,048 k +- 1; 256 tiles against 257; one odd count near 600,000
SORT_N = {1: 1, 63: 1, 64: 1, 65: 1, 255: 1, 256: 1, 257: 1, 2047: 1, 2048: 1, 2049: 2, 4097: 3, 524288: 256, 524289: 257, 599999: 293}
SORT_N_LARGE = 100000             # from here on: fewer patterns and widths per count
# nbits -> the passes it claims (a pass per started byte).  An odd number leaves the result in the temporaries.
SORT_NBITS = {64: {0: 0, 1: 1, 8: 1, 9: 2, 16: 2, 24: 3, 32: 4, 33: 5, 40: 5, 48: 6, 56: 7, 63: 8, 64: 8},
              32: {0: 0, 7: 1, 8: 1, 20: 3, 32: 4}}
SORT_NBITS_LARGE = {64: (8, 16, 40, 64), 32: (8, 20, 32)}
SORT_PATTERNS = ("equal", "ascending", "descending", "two_digits", "digit_cycle", "high_bit", "confined", "garbage")
SORT_PATTERNS_LARGE = ("equal", "two_digits", "high_bit", "garbage")
GARBAGE_KEYS = 5                  # distinct masked keys of the "garbage" pattern: ties in every tile and across tiles


def tiles(n):
    return (n + RS_TILE - 1) // RS_TILE


def passes(nbits):
    return (nbits + 7) // 8


def sort_mask(nbits):
    """what radix_sort_passes sorts by: the low 8 * ceil(nbits / 8) bits (its loop `for (shift = 0; shift < nbits; shift += 8)`)"""
    return (1 << (8 * passes(nbits))) - 1


def digits(keys, p):
    """the digit of every key in pass p"""
    return ((keys.astype(np.uint64) >> np.uint64(8 * p)) & np.uint64(255)).astype(np.int64)


def sort_keys(bits, n, nbits, pattern):
    """the keys of one case (uint64 / uint32), the same at every call"""
    dt = np.uint64 if bits == 64 else np.uint32
    full = (1 << bits) - 1
    rng = np.random.default_rng([bits, n, nbits, SORT_PATTERNS.index(pattern)])
    i = np.arange(n, dtype=np.uint64)
    if pattern == "equal":                      # stability across lanes, waves, the eight rounds of a tile and the tiles; a set top bit
        k = np.full(n, 0x8142C3A4E5F60718 & full, np.uint64)
    elif pattern == "ascending":
        k = i
    elif pattern == "descending":
        k = np.uint64(n - 1) - i
    elif pattern == "two_digits":               # digits 0 and 255 alternate in every pass
        k = (i & np.uint64(1)) * np.uint64(full)
    elif pattern == "digit_cycle":              # key i has digit i % 256 in every pass: one key per digit, repeated
        k = (i & np.uint64(255)) * np.uint64(0x0101010101010101 & full)
    elif pattern == "high_bit":                 # random over the whole key, bit 63 / 31 set in half the keys
        k = rng.integers(0, 1 << (bits - 1), n, dtype=np.uint64) | ((i & np.uint64(1)) << np.uint64(bits - 1))
    elif pattern == "confined":                 # random below 2^nbits
        k = rng.integers(0, 1 << nbits, n, dtype=np.uint64)
    elif pattern == "garbage":                  # a few masked keys, random bits above the rounded width: they ride along, ties in input order
        w = 8 * passes(nbits)
        low = rng.integers(0, min(GARBAGE_KEYS, 1 << w), n, dtype=np.uint64)
        k = low | (rng.integers(0, 1 << (bits - w), n, dtype=np.uint64) << np.uint64(w)) if w < bits else low
    else:
        raise ValueError(pattern)
    return k.astype(dt)


def sort_cases(bits, n):
    """-> [(name, nbits, pattern)] of one key width and count"""
    large = n >= SORT_N_LARGE
    return [("u%d n=%d nbits=%d %s" % (bits, n, nb, pat), nb, pat)
            for nb in (SORT_NBITS_LARGE[bits] if large else SORT_NBITS[bits]) for pat in (SORT_PATTERNS_LARGE if large else SORT_PATTERNS)]


def sort_ref(keys, nbits, vals=None):
    """a stable sort by the masked key, applied to the keys (upper bits intact) and to the values"""
    perm = np.argsort(keys & keys.dtype.type(sort_mask(nbits) & ((1 << (8 * keys.itemsize)) - 1)), kind="stable")
    return keys[perm], None if vals is None else vals[perm]


# ---- the scan -------------------------------------------------------------------------------------------------------------------------
QSCAN_TILE = 4096                 # counts per workgroup
QSCAN_ROW = 256                   # threads of k_qscan_write: above 256 tiles its loop over the tile sums takes a second step

SCAN_N = {0: 1, 1: 1, 15: 1, 16: 1, 17: 1, 255: 1, 256: 1, 257: 1, 4095: 1, 4096: 1, 4097: 2, 8193: 3, 1048576: 256, 1048577: 257}      # (n = 0 still launches one tile)
SCAN_TYPES = ((np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int64))
SCAN_VALUES = ("zeros", "ones", "small", "three_2p30", "above_2p32", "one_at_0", "one_at_4095", "one_at_4096", "one_at_last")
SCAN_CAP = 1000


def scan_tiles(n):
    return max(1, (n + QSCAN_TILE - 1) // QSCAN_TILE)


def scan_counts(n, in_dtype, values):
    """the counts of one case, or None where the case does not exist (an index beyond n, counts above 2^32 in 32 bits)"""
    rng = np.random.default_rng([n, SCAN_VALUES.index(values), np.dtype(in_dtype).itemsize])
    c = np.zeros(n, in_dtype)
    if values == "zeros":
        pass
    elif values == "ones":
        c[:] = 1
    elif values == "small":
        c[:] = rng.integers(0, 10, n)
    elif values == "three_2p30":                # the int32 scan wraps at out[3]; the total in 64 bits is exact
        if n < 3:
            return None
        c[:3] = 1 << 30
    elif values == "above_2p32":
        if np.dtype(in_dtype).itemsize != 8 or n < 1:
            return None
        c[:] = rng.integers(0, 3, n)
        c[rng.integers(0, n, min(n, 7))] = (1 << 32) + 5
        c[n - 1] = (1 << 33) + 1
    else:
        at = {"one_at_0": 0, "one_at_4095": 4095, "one_at_4096": 4096, "one_at_last": n - 1}[values]
        if at < 0 or at >= n:
            return None
        c[at] = 7
    return c


def scan_ref(cnt, out_dtype):
    """-> (out[0 .. n] in out_dtype with wrap-around, the exact total)"""
    full = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))]).astype(np.int64)
    return full.astype(out_dtype), int(full[-1])


def cap_counts(n, in_dtype):
    """counts around SCAN_CAP: cap + 1 (reported) at the first and last index of the first and the last tile and at index 4,096, cap (not
    reported) right beside each, small counts elsewhere -> (counts, the reported indices ascending)"""
    rng = np.random.default_rng([n, 99])
    c = rng.integers(0, 10, n).astype(in_dtype)
    last0 = (scan_tiles(n) - 1) * QSCAN_TILE
    over = sorted({i for i in (0, QSCAN_TILE - 1, QSCAN_TILE, last0, n - 1) if 0 <= i < n})
    for i in over:
        for j in (i - 1, i + 1):
            if 0 <= j < n:
                c[j] = SCAN_CAP
    for i in over:
        c[i] = SCAN_CAP + 1
    return c, np.array(over, np.int32)
