// bam_chunk_plan.h — how telr_bam_load_chunked cuts a BAM file into chunks (behind telr_bam_chunk_plan).  Plain C++: no
// HIP call and no type of the engine's own, so it is pinned on a CPU (tests/test_bam_chunks_ref.py against tests/bam_chunks_ref.py).
//
// Chunks.  A chunk is a run of consecutive whole BGZF members in file order.  It closes before the member whose ISIZE would take the
// chunk's sum of ISIZE above chunk_bytes, and it always holds at least one member: a member that alone exceeds chunk_bytes is a chunk of
// its own.  Members of ISIZE 0 (the EOF marker among them) are members like any other: they join the open chunk whenever that has room
// for 0 bytes, which is always except behind a chunk that is already above chunk_bytes.  No members: no chunks.
#ifndef TELR_BAM_CHUNK_PLAN_H
#define TELR_BAM_CHUNK_PLAN_H
#include <cstdint>
#include "../../include/telr_hip.h"

// first[c] = the first member of chunk c for c < min(*n_chunks, cap); *n_chunks = their number.  TELR_E_ARG: a null pointer, a negative
// count or ISIZE, chunk_bytes below 1.  TELR_E_RANGE: more chunks than cap (the first cap entries are written, *n_chunks is exact).
static inline int bam_chunk_plan(int64_t n_members, const int32_t *isize, int64_t chunk_bytes, int64_t *first, int64_t cap, int64_t *n_chunks)
{
    if (n_members < 0 || chunk_bytes < 1 || cap < 0 || !n_chunks || (n_members > 0 && !isize) || (cap > 0 && !first)) return TELR_E_ARG;
    for (int64_t m = 0; m < n_members; ++m) if (isize[m] < 0) return TELR_E_ARG;
    int64_t n = 0, sum = 0;
    for (int64_t m = 0; m < n_members; ++m) {
        if (m == 0 || sum + isize[m] > chunk_bytes) { if (n < cap) first[n] = m; ++n; sum = 0; }
        sum += isize[m];
    }
    *n_chunks = n;
    return n > cap ? TELR_E_RANGE : TELR_OK;
}
#endif /* TELR_BAM_CHUNK_PLAN_H */
