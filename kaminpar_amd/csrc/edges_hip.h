// Launch interface of the edge-list ingestion kernels (edges_hip.hip): an
// unsorted, possibly duplicated, possibly one-directional list of pairs
// becomes the canonical device CSR of the undirected simple graph. Plain
// device pointers only; the driver (kmp_lp_create_from_edges) is in
// lp_hip.hip, because the engine struct is private to it. Rule:
// include/kaminpar_lp.h, "engines from edge lists".
#pragma once

#include <hip/hip_runtime.h>

#include "lp_common.h"

namespace kmp_edges {

using kmp::i32;
using kmp::u32;
using kmp::u64;

enum IdKind { kIdsU32 = 0, kIdsI64 = 1, kIdsI32 = 2 };

// Device counters of one build (u64 each; cleared by the driver).
enum Counter {
  kBadIds = 0,     // pairs with an id out of range (or negative, or >= 2^32)
  kBadWeights = 1, // pairs with a weight <= 0
  kSelfLoops = 2,  // valid pairs with src == dst
  kMaxId = 3,      // largest representable id seen (scan_ids)
  kOverflow = 4,   // collapsed arcs whose sum left the i32 range
  kNumCounters = 8
};

// Value of a saturated sum: one past the largest arc weight.
constexpr u32 kSumSaturated = 0x80000000u;

// Bit width of n: the smallest b with n < 2^b. Keys are row * 2^b + col, so
// row n (the "dropped" row of self-loops) fits and sorts behind every real row.
inline u32 key_bits(u32 n) {
  u32 b = 0;
  while (b < 32 && (static_cast<u64>(n) >> b) != 0) {
    ++b;
  }
  return b;
}

// The pass that infers n: counters[kMaxId] = largest id, counters[kBadIds] +=
// pairs with an id that is negative or >= 2^32. Indexes nothing by an id.
void scan_ids(
    const void *src, const void *dst, IdKind kind, u64 num_pairs, u64 *counters,
    hipStream_t stream
);

// keys[2i], keys[2i + 1] = the two arcs of pair i under key_bits(n), or twice
// the dropped key n * 2^b for a self-loop or an invalid pair; vals (null iff
// weights is) the pair's weight twice, 0 on dropped arcs. Counts bad ids (>= n
// included), bad weights and self-loops. Indexes nothing by an id. keys and
// vals are 16-byte aligned; src, dst and weights may have any alignment their
// type allows (16-byte accesses are used where all three allow them).
void pack(
    const void *src, const void *dst, IdKind kind, const i32 *weights, u64 num_pairs, u32 n,
    u64 *keys, i32 *vals, u64 *counters, hipStream_t stream
);

// Radix sort of count keys (with vals, unless vals[0] is null) over the bits
// [0, end_bit). temp == nullptr only sizes temp_bytes. Returns the index (0 or
// 1) of the buffer that holds the result.
int sort(
    void *temp, size_t &temp_bytes, u64 *keys[2], i32 *vals[2], u64 count, u32 end_bit,
    hipStream_t stream
);

// Collapses runs of equal keys: ukeys / uvals receive one entry per run in
// order, *d_count their number. vals == nullptr: keys only. Otherwise the
// value of a run is the maximum, or with sum the sum saturated at
// kSumSaturated (every addition is carried out in 64 bits). temp == nullptr
// only sizes temp_bytes.
void collapse(
    void *temp, size_t &temp_bytes, const u64 *keys, const i32 *vals, u64 count, bool sum,
    u64 *ukeys, i32 *uvals, u32 *d_count, hipStream_t stream
);

// counters[kOverflow] += |{i < *d_count : uvals[i] == kSumSaturated}|; the
// count is read on the device.
void check_sums(const i32 *uvals, const u32 *d_count, u64 *counters, hipStream_t stream);

// adjncy[i] = col of ukeys[i], adjwgt[i] = uvals[i] (unless null) for i < m,
// and xadj (n + 1 entries) = the row offsets: cleared, marked with i + 1 at
// the last arc of every row, then closed by an inclusive maximum scan, which
// carries the offsets across empty rows, row 0 and the tail. Every row of
// ukeys[0 .. m) is below n. temp == nullptr only sizes temp_bytes (the scan's).
void build(
    void *temp, size_t &temp_bytes, const u64 *ukeys, const i32 *uvals, u32 m, u32 n, u64 *xadj,
    u32 *adjncy, i32 *adjwgt, hipStream_t stream
);

} // namespace kmp_edges
