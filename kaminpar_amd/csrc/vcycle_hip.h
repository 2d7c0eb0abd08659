// Launch interface of the V-cycle kernels (vcycle_hip.hip): the restriction
// of a fine partition to the coarse level (the inverse of the projection in
// resident_hip.hip), its consistency count, a small indexed gather and the
// block weights of a partition. Plain device pointers only; the drivers
// (kmp_lp_restrict, kmp_lp_set_communities_resident, kmp_lp_resident_cut) are
// in lp_hip.hip. Rules: include/kaminpar_lp.h. No kernel here keeps a table
// sized by k in LDS, so they run at any k the engine accepts.
#pragma once

#include <hip/hip_runtime.h>

#include "lp_common.h"

namespace kmp_vcycle {

using kmp::i32;
using kmp::u32;
using kmp::u64;

// coarse[map[u]] = comm[u] for u < n; coarse has coarse_n entries and a map[u]
// outside it is skipped (and counted by restrict_mismatches). Writers of one
// slot race; the result is defined iff they all write the same value,
// which restrict_mismatches decides afterwards.
void restrict_labels(
    const u32 *map, const u32 *comm, u32 n, u32 *coarse, u32 coarse_n, hipStream_t stream
);

// *count_out = |{u < n : coarse[map[u]] != comm[u]}| (cleared here).
void restrict_mismatches(
    const u32 *map, const u32 *comm, u32 n, const u32 *coarse, u32 coarse_n,
    unsigned long long *count_out, hipStream_t stream
);

// out[i] = src[ids[i]] for i < count.
void gather(const u32 *ids, u32 count, const u32 *src, u32 *out, hipStream_t stream);

// weights[b] = sum of vwgt[u] (1 where vwgt is null) over labels[u] == b, for
// b < k (cleared here). Every label is below k.
void block_weights(
    const u32 *labels, const i32 *vwgt, u32 n, u32 k, unsigned long long *weights,
    hipStream_t stream
);

} // namespace kmp_vcycle
