// Launch interface of the block subgraph extraction kernels (extract_hip.hip).
// Plain device pointers only, so the engine struct stays private to
// lp_hip.hip, which owns the kmp_lp_extract_subgraphs driver (scratch, the
// rocprim order pass, the packed result handle). Rule: include/kaminpar_lp.h.
#pragma once

#include <hip/hip_runtime.h>

#include "lp_common.h"

namespace kmp_extract {

using kmp::i32;
using kmp::i64;
using kmp::u32;
using kmp::u64;

// Device arrays one extraction works on. Everything is owned by the caller;
// n-sized unless noted.
struct View {
  u32 n;
  u32 k;
  const u64 *xadj;
  const u32 *adjncy;
  const i32 *adjwgt; // null = unit (then sub_adjwgt is null too)
  const i32 *vwgt;   // null = unit (then sub_vwgt is null too)
  const u32 *labels; // the uploaded partition; read by prepare only
  uint16_t *labels16; // shadows written by prepare (a label >= k becomes 0);
  uint8_t *labels8;   // gathered from: u8 when k <= 256, u16 otherwise
  u32 *deg_in;        // internal degree per vertex id (count)
  u32 *m_list;        // vertices with 16 < deg <= 2048
  u32 *l_list;        // vertices with deg > 2048
  u32 *tier_counts;   // [0] = |m_list|, [1] = |l_list|, [2] = labels >= k seen
  u32 *node_cnt;      // k: vertices per block (prepare)
  unsigned long long *arc_cnt; // k: internal arcs per block (count)
  unsigned long long *arcs;    // scanned-arc counter (count + fill)
  // order + fill
  const u32 *nodes;    // vertex ids by (label, id)
  const u32 *node_off; // k + 1
  u32 *pos;            // position of a vertex in nodes
  u32 *mapping;        // pos - node_off[label]
  u64 *sub_xadj;       // n + 1: internal degrees in nodes order, then scanned
  u32 *sub_adj;        // packed outputs
  i32 *sub_adjwgt;
  i32 *sub_vwgt;
};

// Shadows, per-block vertex counts, degree tiers and the bad-label count.
// Resets tier_counts and node_cnt; list order is unspecified and never
// affects results.
void prepare(const View &v, hipStream_t stream);

// Count pass: deg_in of every vertex and arc_cnt of every block (reset here).
// m_count / l_count are the host copies of tier_counts.
void count(const View &v, u32 m_count, u32 l_count, hipStream_t stream);

// After the sort: pos, mapping, sub_vwgt and the unscanned sub_xadj
// (sub_xadj[i] = deg_in[nodes[i]], sub_xadj[n] = 0). keys[i] is the label of
// nodes[i].
void place(const View &v, const u32 *keys, hipStream_t stream);

// Fill pass: every sub-row compacted in adjacency order into sub_adj /
// sub_adjwgt at sub_xadj[pos[u]]. No atomic decides a position.
void fill(const View &v, u32 m_count, u32 l_count, hipStream_t stream);

// out[i] = sub_xadj[first + i] - base for i in [0, count]: one block's xadj.
void rebase_xadj(const u64 *sub_xadj, u64 first, u64 base, u32 count, u64 *out, hipStream_t stream);

void iota(u32 n, u32 *out, hipStream_t stream);

} // namespace kmp_extract
