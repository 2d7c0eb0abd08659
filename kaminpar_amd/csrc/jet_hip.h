// Launch interface of the Jet refiner kernels (jet_hip.hip). Plain device
// pointers only, so the engine struct stays private to lp_hip.hip, which owns
// the kmp_lp_jet driver (schedule, rebalancing, best-snapshot bookkeeping).
#pragma once

#include <hip/hip_runtime.h>

#include "lp_common.h"

namespace kmp_jet {

using kmp::i32;
using kmp::i64;
using kmp::u32;
using kmp::u64;

// One 8-byte candidate record per vertex, rewritten by every find pass.
// label is the snapshot block the pass saw; next == label marks "no move".
struct alignas(8) Rec {
  i32 gain;
  uint16_t next;
  uint16_t label;
};

// Device arrays one Jet call works on. Everything is owned by the caller.
struct View {
  u32 n;
  u32 k;
  const u64 *xadj;
  const u32 *adjncy;
  const i32 *adjwgt; // null = unit
  const i32 *vwgt;   // null = unit
  u32 *labels;
  uint16_t *labels16;
  uint8_t *labels8; // written always, gathered from only when k <= 256
  i64 *weights;     // k block weights
  uint8_t *lock;    // n
  Rec *rec;         // n
  u32 *m_list;      // vertices with 16 < deg <= 2048
  u32 *l_list;      // vertices with deg > 2048
  u32 *tier_counts; // [0] = |m_list|, [1] = |l_list|
  unsigned long long *arcs;  // scanned-arc counter
  unsigned long long *moves; // executed-move counter
};

// Degree tiers (degrees never change: once per kmp_lp_jet call). Resets and
// fills tier_counts; list order is unspecified and never affects results.
void build_tiers(const View &v, hipStream_t stream);

// Step 1: writes rec[u] for every vertex. m_count / l_count are the host
// copies of tier_counts.
void find(const View &v, double temp, u32 m_count, u32 l_count, hipStream_t stream);

// Steps 2+3 fused: afterburner over candidates, lock update, in-place commit
// of labels + shadows, block-weight deltas, move counter.
void filter_commit(const View &v, u32 m_count, u32 l_count, hipStream_t stream);

// Step 5: writes TWICE the edge cut of the current labelling to *cut2, over
// the same tiers (the engine's k_edge_cut serializes on hub rows).
void edge_cut2(
    const View &v, u32 m_count, u32 l_count, unsigned long long *cut2, hipStream_t stream
);

} // namespace kmp_jet
