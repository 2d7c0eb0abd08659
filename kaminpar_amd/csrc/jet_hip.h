// Launch interface of the Jet refiner and selection rebalancer kernels
// (jet_hip.hip). Plain device pointers only, so the engine struct stays
// private to lp_hip.hip, which owns the kmp_lp_jet and kmp_lp_rebalance
// drivers (schedule, pass loop, best-snapshot bookkeeping).
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

// ------------------------------------------------- selection rebalancer
// Workspace of kmp_lp_rebalance (rule: include/kaminpar_lp.h). One pass is
//   rebalance_score              candidates of the source blocks, id order
//   rebalance_order(false)       (block, key desc, id) + exclusive weights
//   rebalance_select             shortest prefix covering each overload
//   rebalance_order(true)        (target, key desc, id) + inclusive weights
//   rebalance_apply              admitted moves, committed in place
// and the host only reads *count in between. Everything is owned by the
// caller and allocated once per call; n-sized unless noted.
struct Rebal {
  i64 *over;  // k: W - C, rewritten by the host before every pass
  i64 *room;  // k: C - W
  i64 *cum;   // k: inclusive prefix sum of max(room, 0)
  i64 total_room;  // cum[k - 1]
  u32 best_target; // largest room, smallest id
  u32 pass;
  u64 *key;        // per vertex: block << 53 | (2^53 - 1 - (key + 2^52))
  uint16_t *to;    // per vertex: chosen target
  uint8_t *flag;   // per vertex: candidate (score) / selected (select)
  u32 *ids[2];     // [0] compacted in id order, [1] ordered
  u64 *keys[2];    // sort keys of ids[0] / ids[1]
  u32 *seg;        // segment (block) of ids[1][i]
  i64 *wt;         // vertex weight of ids[1][i]
  i64 *pre;        // segmented prefix weights
  u32 *count;      // 1: length of ids[0]
  void *temp;      // rebalance_temp_bytes(n)
  size_t temp_bytes;
  unsigned long long *arcs;     // scanned arcs (cumulative)
  unsigned long long *selected; // selected moves (cumulative)
  unsigned long long *moves;    // admitted moves (cumulative)
};

size_t rebalance_temp_bytes(u32 n);

// Writes key/to/flag of every candidate and compacts their ids into ids[0]
// (ascending), *count = how many.
void rebalance_score(const View &v, const Rebal &rb, u32 m_count, u32 l_count, hipStream_t stream);

// Orders ids[0][0..count) into ids[1] by (source block | target, key desc, id
// asc) and fills seg, wt and pre: exclusive prefix weights per source block,
// inclusive per target.
void rebalance_order(const View &v, const Rebal &rb, u32 count, bool by_target, hipStream_t stream);

// Marks the ordered candidates whose exclusive prefix is below their block's
// overload and compacts them into ids[0] (ascending), *count = how many.
void rebalance_select(const View &v, const Rebal &rb, u32 count, hipStream_t stream);

// Commits the ordered selected moves whose inclusive prefix fits the room of
// their target: labels, both shadows, block weights, move counter.
void rebalance_apply(const View &v, const Rebal &rb, u32 count, hipStream_t stream);

} // namespace kmp_jet
