// Launch interface of the threshold edge sparsification kernels
// (sparsify_hip.hip): a radix select of the threshold weight and a stable
// per-row compaction of a device CSR. Plain device pointers only; the driver
// (kmp_contract_engine_sparsified) is in lp_hip.hip. Rule:
// include/kaminpar_lp.h.
#pragma once

#include <hip/hip_runtime.h>

#include "lp_common.h"

namespace kmp_sparsify {

using kmp::i32;
using kmp::u32;
using kmp::u64;

// Device-side state of the radix select; after select() it holds the result.
struct SelectState {
  u32 prefix; // digits fixed so far; the threshold T after the last pass
  u32 pad;
  u64 rank;   // 1-based rank of T among the weights that match prefix
  u64 larger; // |{w > T}|
  u64 equal;  // |{w == T}|
};

constexpr u32 kSelectPasses = 4; // 8-bit digits of a 32-bit weight
constexpr u32 kSelectBins = 256;

// st->prefix = the rank-th smallest (1-based, 1 <= rank <= c_m) of the c_m
// positive weights w, with st->larger and st->equal. hist: kSelectPasses *
// kSelectBins words of scratch. Nothing is read back between the passes.
void select(const i32 *w, u32 c_m, u64 rank, u32 *hist, SelectState *st, hipStream_t stream);

struct View {
  u32 n;
  const u64 *xadj;   // n + 1
  const u32 *adjncy; // sorted per row
  const i32 *adjwgt;
  // n + 1: count() leaves the kept arcs of every row here and 0 in [n]; the
  // driver scans it exclusively in place, which makes it the new xadj.
  u64 *cnt;
  u32 *out_adj; // fill(): cnt[n] entries after the scan
  i32 *out_wgt;
  u32 *m_list; // n: rows of degree 17 .. 2048 (prepare)
  u32 *l_list; // n: rows of degree > 2048
  u32 *tier_counts; // 2: lengths of m_list, l_list; read on the device
  // nullptr (the default): fill() evaluates the rule again. Otherwise c_m
  // bytes: count() stores a byte per arc and fill() reads it back instead;
  // same output, kept for measuring one form against the other
  uint8_t *flags;
  const SelectState *st;
  u64 target;
  u64 seed;
};

// Builds the degree tier lists.
void prepare(const View &v, hipStream_t stream);
// Kept arcs per row under the rule, with T / larger / equal read from v.st.
void count(const View &v, hipStream_t stream);
// Writes the kept arcs of every row, in row order, at cnt[u] onwards.
void fill(const View &v, hipStream_t stream);

} // namespace kmp_sparsify
