// Launch interface of the resident-label kernels (resident_hip.hip): the
// projection of a coarse partition onto the finer level and the device form
// of the isolated-vertex scan. Plain device pointers only, so the engine
// struct stays private to lp_hip.hip, which owns the drivers
// (kmp_lp_project, kmp_contract_engine). Rules: include/kaminpar_lp.h.
#pragma once

#include <hip/hip_runtime.h>

#include "lp_common.h"

namespace kmp_resident {

using kmp::i32;
using kmp::u32;
using kmp::u64;

// out[u] = coarse_labels[map[u]] for u < n. coarse_labels holds label_bytes
// (1, 2 or 4) bytes per coarse vertex: the coarse engine's u8 / u16 shadow or
// its u32 label array. Every map[u] indexes that array.
void project(
    const u32 *map, const void *coarse_labels, int label_bytes, u32 n, u32 *out,
    hipStream_t stream
);

// One pass over xadj (n + 1 entries): flags[u] = (degree of u == 0),
// stats[0] = maximum degree, stats[1] = number of flagged vertices. stats is
// cleared here.
void iso_flags(u32 n, const u64 *xadj, uint8_t *flags, u32 *stats, hipStream_t stream);

// Flagged vertex ids in ascending order (rocprim::select is stable);
// *count_out receives their number. temp == nullptr only sizes temp_bytes.
void iso_select(
    void *temp, size_t &temp_bytes, const uint8_t *flags, u32 n, u32 *ids_out, u32 *count_out,
    hipStream_t stream
);

// out[i] = vwgt[ids[i]] (1 where vwgt is null) for i < count.
void iso_weights(const u32 *ids, u32 count, const i32 *vwgt, i32 *out, hipStream_t stream);

} // namespace kmp_resident
