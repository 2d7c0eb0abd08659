// MI355X (gfx950) HIP implementation of the KaMinPar label-propagation hot
// path under the deterministic chunk-synchronous schedule (parity contract:
// oracle/lp_oracle.cpp header). Semantics restated from
//   kaminpar-shm/label_propagation.h (engine: gains :487-505, active set
//   :848-870,1908-1912, try_node_move :817-841)
//   kaminpar-shm/refinement/lp/lp_refiner.cc:151-285 (refiner select)
//   kaminpar-shm/coarsening/clustering/lp_clusterer.cc:181-280 (clusterer
//   select), with the commit fixpoint mirroring
//   kaminpar-dist/refinement/lp/lp_refiner.cc:296-333 (rollback protocol).
//
// Kernel design (CDNA4): irregular integer gather workload; the roofline
// bound is HBM bandwidth (8 B per directed arc: 4 B adjncy + 4 B labels
// gather), not MFMA. The schedule's 64-vertex units keep per-vertex state
// reads coalesced. Phase A uses NO append atomics: every position owns a
// 16-byte proposal slot, written by exactly one kernel (S: deg<=16 with
// 16-lane subgroup shuffle-waterfall gains; M: one wavefront per vertex with
// dense per-cluster LDS gains for k<=2048; L: one workgroup per high-degree
// vertex), then rocprim::select compacts valid slots in position order
// (stable), so the commit's stable 32-bit radix sort by target cluster
// yields the deterministic (to, rank) admission order.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string.h>
#include <atomic>
#include <set>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include <rocprim/rocprim.hpp>

#include <rccl/rccl.h>

#include "../../include/kaminpar_lp.h"
#include "edges_hip.h"
#include "extract_hip.h"
#include "jet_hip.h"
#include "lp_common.h"
#include "resident_hip.h"
#include "sparsify_hip.h"
#include "vcycle_hip.h"

using kmp::i32;
using kmp::i64;
using kmp::u32;
using kmp::u64;
using kmp::BlockPerm;
using kmp::iter_seed_of;
using kmp::tie_hash;

// Check the sticky error right after a kernel launch (configuration errors
// surface there, not at the launch statement).
#define LAUNCH_CHECK()                                                                             \
  do {                                                                                             \
    hipError_t lerr_ = hipGetLastError();                                                          \
    if (lerr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: launch error %s at %s:%d\n", hipGetErrorString(lerr_),       \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

#define HIP_CHECK(cmd)                                                                             \
  do {                                                                                             \
    hipError_t err_ = (cmd);                                                                       \
    if (err_ != hipSuccess) {                                                                      \
      fprintf(stderr, "kaminpar_amd: HIP error %s at %s:%d\n", hipGetErrorString(err_), __FILE__,  \
              __LINE__);                                                                           \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

namespace {

// kmp_lp_label_traffic_bytes: every host<->device copy of a partition, a
// clustering or a mapping (and kmp_contract_engine's coarse xadj / vwgt
// downloads) passes its byte count through here, and nothing else does.
std::atomic<u64> g_label_traffic{0};

inline size_t label_traffic(size_t bytes) {
  g_label_traffic.fetch_add(bytes, std::memory_order_relaxed);
  return bytes;
}

constexpr u32 kSmallDeg = 16;    // S path: <= 16 neighbours, 16 lanes/vertex
constexpr u32 kMidDeg = 2048;    // M path: one wavefront per vertex
constexpr u32 kMaxDenseK = 2048; // dense per-cluster LDS gains limit (refine)
constexpr u32 kWave = 64;
constexpr u32 kInvalid = 0xFFFFFFFFu;

struct Prop { // 16-byte proposal record (ABI: uint32x4)
  u32 u;
  u32 to;   // kInvalid marks an empty slot (pre-compaction)
  u32 rank; // position - chunk_base (admission order within the chunk)
  u32 w;    // node weight bits (i32 >= 0)
};

struct PropValid {
  __host__ __device__ bool operator()(const Prop &p) const { return p.to != kInvalid; }
};

// ------------------------------------------------- select helpers (device)
struct BestState {
  i32 gain;
  u64 h;
  u32 c;
  bool have;
};

__device__ inline bool key_better(i32 g, u64 h, u32 c, const BestState &b) {
  if (!b.have) {
    return true;
  }
  if (g != b.gain) {
    return g > b.gain;
  }
  if (h != b.h) {
    return h > b.h;
  }
  return c < b.c;
}

// Gain accumulation uses REPLICATED per-cluster LDS counters: lane l adds
// into replica l % R, so same-address LDS atomic serialization (the dominant
// cost with a single counter per cluster) is cut by ~R. The replicas are
// merged once per vertex. R is chosen so k * R stays within the LDS budget.
__host__ __device__ inline u32 gain_replicas(u32 k) {
  if (k <= 64) {
    return 8;
  }
  if (k <= 256) {
    return 4;
  }
  return 1;
}

// Weight-acceptance predicate (refiner variant, lp_refiner.cc:185-230).
// excl_cur implements BALANCE mode (the overload balancer's forcing rule,
// refinement/balancer/overload_balancer.cc in spirit): a vertex whose block
// exceeds its cap loses "stay" as a candidate, so it proposes its best
// admissible target even at negative gain; everything else (commit
// admission, caps, determinism) is the normal refiner machinery.
__device__ inline bool accept_refine(
    u32 c, u32 cur, i32 u_w, i64 cw, i64 maxw, i64 cur_w, i64 cur_maxw,
    bool balance = false
) {
  if (c == cur) {
    return !(balance && cur_w > cur_maxw);
  }
  if (balance) {
    // room-only in balance mode: the relative-overload clause would let the
    // deterministic select livelock on an already-full favourite target
    return cw + u_w <= maxw;
  }
  return (cw + u_w <= maxw) || ((cw - maxw) < (cur_w - cur_maxw));
}

// Underload-balancer acceptance (underload_balancer.cc is_movable_to): only
// underloaded targets with room; the current block is never a candidate.
__device__ inline bool accept_underload(u32 c, u32 cur, i32 u_w, i64 cw, i64 maxw_c, i64 minw_c) {
  return c != cur && cw < minw_c && cw + u_w <= maxw_c;
}

// Weight-acceptance predicate (clusterer variant, lp_clusterer.cc:199-204).
__device__ inline bool accept_cluster(u32 c, u32 cur, i32 u_w, i64 cw, i64 maxw_uniform) {
  return (cw + u_w <= maxw_uniform) || (c == cur);
}

__device__ inline u32 hash_u32(u32 c) {
  return static_cast<u32>(kmp::splitmix64(c));
}

// ------------------------------------------------------------ S path
// Covers EVERY position of the slice: 4 * kSGroup positions per wave, each
// 16-lane subgroup walking kSGroup positions with the loads staged across
// them (all xadj/active/labels[u] loads, then all adjncy loads, then all
// label gathers), so a lane keeps kSGroup independent chains in flight
// instead of one. Owns the slot for: tail positions (u >= n), inactive or
// degree-filtered vertices (invalid slot), and active deg <= 16 vertices
// (computed result). Leaves deg in (16, inf) active slots for the M/L kernels.
constexpr u32 kSGroup = 4;               // positions per 16-lane subgroup
constexpr u32 kSWavePos = 4 * kSGroup;   // positions per wave

template <typename LT>
__global__ void k_phase_s(
    u32 pos_lo,
    u32 pos_hi,
    u32 chunk_base,
    u32 n,
    u64 iter_seed,
    u32 mode, // 0 = refine, 1 = overload balance, 2 = underload balance
    u32 fallback,
    u32 max_degree,
    u32 s_clear, // v2 path: S owns the chunk's active-flag clearing
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ vwgt,
    const i32 *__restrict__ adjwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const i64 *__restrict__ minw, // per-block minimums (mode 2 only)
    const LT *__restrict__ labels_s, // u8 shadow for k <= 256, else u16
    uint8_t *__restrict__ active,
    const uint8_t *__restrict__ unit_active,
    Prop *__restrict__ slots
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;  // subgroup 0..3
  const u32 slot = lane & 15; // lane within subgroup
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u64 p0 = static_cast<u64>(pos_lo) + static_cast<u64>(wave_id) * kSWavePos;
  if (p0 >= pos_hi) {
    return;
  }
  const u32 pbase = static_cast<u32>(p0) + sub * kSGroup;

  const BlockPerm perm(n, iter_seed);

  // per-position state: 0 = not ours (past pos_hi, inactive unit, or an
  // active deg > 16 vertex owned by M/L), 1 = write an invalid slot,
  // 2 = compute
  u32 st[kSGroup];
  u32 uu[kSGroup];
  u64 row[kSGroup];
  u32 deg[kSGroup];
  u32 cur[kSGroup];
  i32 uw[kSGroup];

  // stage 0: a subgroup's kSGroup consecutive positions span at most two
  // 64-vertex units (one whenever pos_lo is subgroup-aligned). One byte per
  // unit decides whether anything in it is active (inactive units are
  // skipped downstream); a wave with no active unit exits here.
  const u32 p_last = pos_hi - 1;
  const u32 p_a = pbase < p_last ? pbase : p_last;
  const u32 p_b = (p_last - p_a) < (kSGroup - 1) ? p_last : p_a + (kSGroup - 1);
  const u32 unit_a = p_a / kmp::kUnit;
  const u32 unit_b = p_b / kmp::kUnit;
  const u32 vb_a = perm.fp(unit_a);
  u32 vb_b = vb_a;
  if (unit_b != unit_a) {
    vb_b = perm.fp(unit_b);
  }
  const bool on_a = unit_active[vb_a] != 0;
  const bool on_b = unit_active[vb_b] != 0;
  if (!__any(on_a || on_b)) {
    return;
  }

  // stage 1: per-vertex loads of all kSGroup positions, issued
  // unconditionally on clamped (always valid) indices so that nothing
  // separates them; the validity flags pick what is used
  const u32 n_last = n - 1;
#pragma unroll
  for (u32 g = 0; g < kSGroup; ++g) {
    const u32 p = pbase + g;
    const bool in_range = pbase <= p_last && g <= p_last - pbase;
    const u32 pc = in_range ? p : p_last;
    const bool in_a = (pc / kmp::kUnit) == unit_a;
    const u32 vb = in_a ? vb_a : vb_b;
    const bool unit_on = in_a ? on_a : on_b;
    const u32 u = vb * kmp::kUnit + (pc % kmp::kUnit);
    const u32 uc = u < n ? u : n_last;
    const u64 r0 = xadj[uc];
    const u64 r1 = xadj[uc + 1];
    const uint8_t a = active[uc];
    cur[g] = labels[uc];
    uw[g] = vwgt ? vwgt[uc] : 1;
    uu[g] = u;
    row[g] = r0;
    deg[g] = static_cast<u32>(r1 - r0);
    st[g] = !(in_range && unit_on) ? 0u : (u < n && a) ? 2u : 1u;
  }

  // classify; v2: clear the processed flag inline (replaces
  // k_clear_active's pass; exactly the legacy condition:
  // deg <= max_degree && active). M/L work lists are built by k_build_lists
  // (one reservation atomic per wave-row; appending from here serialized
  // millions of waves on a single counter -- measured 2x at scale 26).
#pragma unroll
  for (u32 g = 0; g < kSGroup; ++g) {
    if (st[g] == 2) {
      if (deg[g] > max_degree) {
        st[g] = 1;
      } else {
        if (s_clear && slot == 0) {
          active[uu[g]] = 0;
        }
        if (deg[g] > kSmallDeg) {
          st[g] = 0; // M/L kernels own (and always write) these slots
        }
      }
    }
  }

  // stage 2: candidate loads, lane handles one edge of each position
  // (non-temporal: the adjncy stream is read once per sweep and must not
  // evict the label shadow from L2/MALL, the gather working set)
  u32 v[kSGroup];
  i32 w[kSGroup];
#pragma unroll
  for (u32 g = 0; g < kSGroup; ++g) {
    v[g] = kInvalid;
    w[g] = 0;
    if (st[g] == 2 && slot < deg[g]) {
      v[g] = __builtin_nontemporal_load(&adjncy[row[g] + slot]);
      w[g] = adjwgt ? adjwgt[row[g] + slot] : 1;
    }
  }
  // stage 3: label gathers (narrow shadow: u8 for k <= 256 -- 64 MB at
  // scale 26, MALL-resident -- u16 up to k <= 2048)
  u32 c[kSGroup];
#pragma unroll
  for (u32 g = 0; g < kSGroup; ++g) {
    c[g] = kInvalid;
    if (v[g] != kInvalid) {
      c[g] = labels_s[v[g]];
    }
  }

  // stage 4: dedupe, select and slot write per position
  const u32 base = sub * 16;
#pragma unroll
  for (u32 g = 0; g < kSGroup; ++g) {
    if (st[g] == 0) {
      continue;
    }
    const u32 p = pbase + g;
    const u32 sidx = p - pos_lo;
    if (st[g] == 1) {
      // always-write contract: every position of an ACTIVE unit gets a fresh
      // slot each chunk (proposal or invalid), so the memset-free v2 commit
      // can read raw slots gated only by unit_active
      if (slot == 0) {
        slots[sidx] = Prop{0u, kInvalid, 0u, 0u};
      }
      continue;
    }
    const u32 u = uu[g];
    const u32 cg = c[g];
    const i32 wg = w[g];

    // dedupe within subgroup: sum weights of equal clusters; lowest slot owns
    i32 gain = wg;
    bool owner = (slot < deg[g]);
    for (u32 j = 0; j < 16; ++j) {
      const u32 cj = __shfl(cg, base + j, kWave);
      const i32 wj = __shfl(wg, base + j, kWave);
      if (j != slot && cg != kInvalid && cj == cg) {
        gain += wj;
        if (j < slot) {
          owner = false;
        }
      }
    }

    const u32 cu = cur[g];
    const i32 u_w = uw[g];
    const i64 cur_w = weights[cu];
    const i64 cur_maxw = maxw[cu];
    const bool excl_cur = mode == 1;
    bool vgate = true;
    if (mode == 2) {
      const i64 mnw = minw[cu];
      vgate = cur_w >= mnw && cur_w - u_w >= mnw; // is_movable_from
    }

    BestState best{0, 0, 0, false};
    if (owner && cg != kInvalid && vgate) {
      const i64 cw = weights[cg];
      const i64 mw = maxw[cg];
      const bool ok = (mode == 2)
                          ? accept_underload(cg, cu, u_w, cw, mw, minw[cg])
                          : accept_refine(cg, cu, u_w, cw, mw, cur_w, cur_maxw, excl_cur);
      if (ok) {
        best = BestState{gain, tie_hash(iter_seed, u, cg), cg, true};
      }
    }

    // subgroup argmax over 16 lanes
    for (int off = 8; off > 0; off >>= 1) {
      const i32 og = __shfl_down(best.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
      const u32 oc = __shfl_down(best.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
      if ((slot + off) < 16 && ohave && key_better(og, oh, oc, best)) {
        best = BestState{og, oh, oc, true};
      }
    }

    if (slot == 0) {
      BestState fin = best;
      if (!fin.have && mode == 1 && cur_w > cur_maxw && fallback != kInvalid &&
          fallback != cu) {
        // balance fallback: no admissible adjacent target (e.g. everything in
        // one block) -- propose the lightest block with room at gain 0
        fin = BestState{0, tie_hash(iter_seed, u, fallback), fallback, true};
      }
      if (fin.have && fin.c != cu) {
        slots[sidx] = Prop{u, fin.c, p - chunk_base, static_cast<u32>(u_w)};
      } else {
        slots[sidx] = Prop{0u, kInvalid, 0u, 0u};
      }
    }
  }
}

// ------------------------------------------------------------ M path
// One wavefront per position (dead waves for non-M positions retire in a
// few cycles; list building would need a serializing append counter).
// Handles active vertices with kSmallDeg < deg <= kMidDeg: dense per-wave
// LDS gains (k <= kMaxDenseK), ballot-waterfall accumulation. Active
// deg > kMidDeg vertices were appended to the L list by k_phase_s.
// blockDim.x = 256 (4 waves); dynamic LDS = 4 * k * sizeof(i32).
constexpr u32 kMUnroll = 4; // adjncy loads / gathers in flight per lane (M, L)

template <bool kUnitWeights, typename LT>
__global__ void k_phase_m(
    u32 pos_lo,
    u32 chunk_base,
    u32 k,
    u64 iter_seed,
    u32 mode,
    u32 fallback,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const LT *__restrict__ labels_s,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const i64 *__restrict__ minw,
    const u64 *__restrict__ m_list,
    const u32 *__restrict__ m_count,
    Prop *__restrict__ slots
) {
  extern __shared__ i32 lds[];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wave_in_wg = threadIdx.x >> 6;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  const u32 R = gain_replicas(k);
  i32 *gains = lds + wave_in_wg * k * R; // R replicas of k counters

  // Software pipeline over the wave's list entries, so no load is consumed
  // right after it is issued: the list record is read two entries ahead,
  // the xadj pair one entry ahead (at the top of the current entry), and the
  // first kMUnroll-deep adjncy batch of the next entry after the current
  // entry's edge loop, i.e. under the current selection and reduction.
  // Look-ahead indices are clamped to the last list entry and look-ahead
  // edges to the row's last edge (listed rows have deg > kSmallDeg), so the
  // prefetches are unconditional loads of valid addresses; past the end they
  // re-read the last entry and are never used.
  const u32 count = *m_count;
  if (wave_id >= count) {
    return;
  }
  const u32 last = count - 1;
  u64 rec_n = m_list[wave_id]; // record of the next entry
  u64 rec_nn;                  // record two entries ahead
  {
    const u64 i2 = static_cast<u64>(wave_id) + num_waves;
    rec_nn = m_list[i2 < last ? i2 : last];
  }
  u64 row_n;   // row of the next entry
  u32 deg_n;
  u32 vpre[kMUnroll]; // first adjncy batch of the next entry
  {
    const u32 u0 = static_cast<u32>(rec_n);
    row_n = xadj[u0];
    deg_n = static_cast<u32>(xadj[u0 + 1] - row_n);
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      const u32 e = lane + j * kWave;
      vpre[j] = __builtin_nontemporal_load(&adjncy[row_n + (e < deg_n ? e : deg_n - 1)]);
    }
  }

  for (u32 vid = wave_id; vid < count; vid += num_waves) {
  const u64 rec = rec_n;
  const u32 p = static_cast<u32>(rec >> 32);
  const u32 u = static_cast<u32>(rec);
  const u64 row = row_n;
  const u32 deg = deg_n;
  u32 vcur[kMUnroll];
#pragma unroll
  for (u32 j = 0; j < kMUnroll; ++j) {
    vcur[j] = vpre[j];
  }

  for (u32 c = lane; c < k * R; c += kWave) {
    gains[c] = 0;
  }
  __threadfence_block(); // LDS ordering; gains slice is private to this wave

  // next entry: xadj pair now (its record arrived an entry ago), and the
  // record after it
  rec_n = rec_nn;
  const u32 un = static_cast<u32>(rec_n);
  row_n = xadj[un];
  const u64 row_n1 = xadj[un + 1];
  {
    const u64 i2 = static_cast<u64>(vid) + 2ull * num_waves;
    rec_nn = m_list[i2 < last ? i2 : last];
  }
  // per-vertex state of the current entry, issued ahead of the edge loop
  const u32 cur = labels[u];
  const i32 u_w = vwgt ? vwgt[u] : 1;

  const u32 rep_off = (lane % R) * k;
  // first batch: adjncy values were prefetched under the previous entry
  // (lanes past the row hold its last edge again and add nothing)
  {
    i32 wv[kMUnroll];
    u32 cv[kMUnroll];
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      const u32 e = lane + j * kWave;
      wv[j] = kUnitWeights ? 1 : adjwgt[row + (e < deg ? e : deg - 1)];
    }
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      cv[j] = labels_s[vcur[j]];
    }
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      if (lane + j * kWave < deg) {
        atomicAdd(&gains[rep_off + cv[j]], wv[j]);
      }
    }
  }
  // full batches: kMUnroll adjncy loads, then the gathers, then the atomics
  u32 eb = kMUnroll * kWave;
  for (; eb + kMUnroll * kWave <= deg; eb += kMUnroll * kWave) {
    u32 vv[kMUnroll];
    i32 wv[kMUnroll];
    u32 cv[kMUnroll];
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      const u32 e = eb + lane + j * kWave;
      vv[j] = __builtin_nontemporal_load(&adjncy[row + e]);
      wv[j] = kUnitWeights ? 1 : adjwgt[row + e];
    }
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      cv[j] = labels_s[vv[j]];
    }
#pragma unroll
    for (u32 j = 0; j < kMUnroll; ++j) {
      atomicAdd(&gains[rep_off + cv[j]], wv[j]);
    }
  }
  // remainder
  for (u32 e = eb + lane; e < deg; e += kWave) {
    const u32 v = __builtin_nontemporal_load(&adjncy[row + e]);
    const i32 w = kUnitWeights ? 1 : adjwgt[row + e];
    atomicAdd(&gains[rep_off + labels_s[v]], w);
  }
  // next entry's first adjncy batch, in flight during the selection below
  deg_n = static_cast<u32>(row_n1 - row_n);
#pragma unroll
  for (u32 j = 0; j < kMUnroll; ++j) {
    const u32 e = lane + j * kWave;
    vpre[j] = __builtin_nontemporal_load(&adjncy[row_n + (e < deg_n ? e : deg_n - 1)]);
  }
  __threadfence_block();

  const i64 cur_w = weights[cur];
  const i64 cur_maxw = maxw[cur];
  const bool excl_cur = mode == 1;
  bool vgate = true;
  if (mode == 2) {
    const i64 mnw = minw[cur];
    vgate = cur_w >= mnw && cur_w - u_w >= mnw;
  }

  BestState best{0, 0, 0, false};
  for (u32 c = lane; vgate && c < k; c += kWave) {
    i32 g = gains[c];
    for (u32 r = 1; r < R; ++r) {
      g += gains[r * k + c];
    }
    if (g <= 0) {
      continue;
    }
    const i64 cw = weights[c];
    const i64 mw = maxw[c];
    const bool ok = (mode == 2)
                        ? accept_underload(c, cur, u_w, cw, mw, minw[c])
                        : accept_refine(c, cur, u_w, cw, mw, cur_w, cur_maxw, excl_cur);
    if (!ok) {
      continue;
    }
    const u64 h = tie_hash(iter_seed, u, c);
    if (key_better(g, h, c, best)) {
      best = BestState{g, h, c, true};
    }
  }

  for (int off = 32; off > 0; off >>= 1) {
    const i32 og = __shfl_down(best.gain, off, kWave);
    const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
    const u32 oc = __shfl_down(best.c, off, kWave);
    const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
    if (ohave && key_better(og, oh, oc, best)) {
      best = BestState{og, oh, oc, true};
    }
  }

  if (lane == 0) {
    BestState fin = best;
    if (!fin.have && mode == 1 && cur_w > cur_maxw && fallback != kInvalid &&
        fallback != cur) {
      fin = BestState{0, tie_hash(iter_seed, u, fallback), fallback, true};
    }
    if (fin.have && fin.c != cur) {
      slots[p - pos_lo] = Prop{u, fin.c, p - chunk_base, static_cast<u32>(u_w)};
    } else {
      slots[p - pos_lo] = Prop{0u, kInvalid, 0u, 0u};
    }
  }
  __threadfence_block(); // gains reuse across grid-stride iterations
  }
}

// ------------------------------------------------------------ L path
// High-degree vertices are processed slice-parallel: rows are cut into
// kLSlice-edge slices, each handled by one workgroup accumulating into a
// per-vertex global gains row (via a per-WG replicated LDS histogram), then
// a selection kernel reduces each row. This keeps mega-hubs (100K+ edges)
// from serializing on a single workgroup.
constexpr u32 kLSlice = 8192;

// Refine-path slice length. A chunk's L work at the 8192-edge slice is a few
// hundred slices on a 2048-workgroup grid; 1024-edge slices (one unrolled
// trip of a 256-thread workgroup) cover the grid. Each slice pays k * R LDS
// clears and up to k global atomics, so the short slice stops paying as k
// grows: at k = 256 (R-MAT scale 28) it measured no gain, 489.2 / 486.7 ms
// per step against 487.2 / 483.7 with the long slice (alternating runs,
// profiles/round3/bench_rmat28_k256_lslice.json), so k > 64 keeps the long
// slice. Where between 64 and 256 the two cross was not measured. The
// clustering L kernels keep kLSlice.
constexpr u32 kLSliceSmall = 1024;
inline u32 refine_l_slice(u32 k) {
  return k <= 64 ? kLSliceSmall : kLSlice;
}

// L prep (refine): write per-vertex slice counts in parallel into a
// zeroed l_cap+1 array; the exclusive prefix runs as a rocprim scan on the
// host side (entries beyond the live count are zero, so l_off[count] holds
// the total).
__global__ void k_l_sizes(
    const u64 *__restrict__ l_list,
    const u32 *__restrict__ l_count,
    const u64 *__restrict__ xadj,
    u32 l_cap,
    u32 slice,
    u32 *__restrict__ sizes
) {
  const u32 count = *l_count < l_cap ? *l_count : l_cap;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    const u32 u = static_cast<u32>(l_list[i]);
    const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
    sizes[i] = (deg + slice - 1) / slice;
  }
}

// Accumulate one slice per workgroup into the vertex's global gains row.
template <bool kUnitWeights, typename LT>
__global__ void k_phase_l_acc(
    u32 k,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const LT *__restrict__ labels_s,
    const u64 *__restrict__ l_list,
    const u32 *__restrict__ l_count,
    u32 l_cap,
    u32 slice, // edges per slice (as used by the prep kernel for l_off)
    const u32 *__restrict__ l_off,
    i32 *__restrict__ l_gains // l_cap x k
) {
  extern __shared__ i32 lds[];
  const u32 R = gain_replicas(k);
  i32 *hist = lds;

  const u32 count = *l_count < l_cap ? *l_count : l_cap;
  const u32 total = l_off[count];
  for (u32 s = blockIdx.x; s < total; s += gridDim.x) {
    // binary search the vertex owning slice s
    u32 lo = 0, hi = count - 1;
    while (lo < hi) {
      const u32 mid = (lo + hi + 1) >> 1;
      if (l_off[mid] <= s) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    const u32 vid = lo;
    const u32 u = static_cast<u32>(l_list[vid]);
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    const u32 e_lo = (s - l_off[vid]) * slice;
    const u32 e_hi = e_lo + slice < deg ? e_lo + slice : deg;

    for (u32 c = threadIdx.x; c < k * R; c += blockDim.x) {
      hist[c] = 0;
    }
    __syncthreads();
    const u32 rep_off = (threadIdx.x % R) * k;
    // full batches: kMUnroll adjncy loads, then the gathers, then the atomics
    u32 eb = e_lo;
    for (; eb + kMUnroll * blockDim.x <= e_hi; eb += kMUnroll * blockDim.x) {
      u32 vv[kMUnroll];
      i32 wv[kMUnroll];
      u32 cv[kMUnroll];
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        const u32 e = eb + threadIdx.x + j * blockDim.x;
        vv[j] = __builtin_nontemporal_load(&adjncy[row + e]);
        wv[j] = kUnitWeights ? 1 : adjwgt[row + e];
      }
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        cv[j] = labels_s[vv[j]];
      }
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        atomicAdd(&hist[rep_off + cv[j]], wv[j]);
      }
    }
    // remainder
    for (u32 e = eb + threadIdx.x; e < e_hi; e += blockDim.x) {
      const u32 v = __builtin_nontemporal_load(&adjncy[row + e]);
      const i32 w = kUnitWeights ? 1 : adjwgt[row + e];
      atomicAdd(&hist[rep_off + labels_s[v]], w);
    }
    __syncthreads();
    i32 *grow = l_gains + static_cast<size_t>(vid) * k;
    for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
      i32 g = hist[c];
      for (u32 r = 1; r < R; ++r) {
        g += hist[r * k + c];
      }
      if (g) {
        atomicAdd(&grow[c], g);
      }
    }
    __syncthreads();
  }
}

// Select per L vertex (one workgroup each, grid-stride), write the slot,
// and reset the gains row for the next chunk.
__global__ void k_phase_l_sel(
    u32 mode,
    u32 fallback,
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    u32 k,
    const u64 *__restrict__ xadj,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const i64 *__restrict__ minw,
    const u64 *__restrict__ l_list,
    const u32 *__restrict__ l_count,
    u32 l_cap,
    i32 *__restrict__ l_gains,
    Prop *__restrict__ slots
) {
  __shared__ i64 red[16];
  const u32 count = *l_count < l_cap ? *l_count : l_cap;
  for (u32 vid = blockIdx.x; vid < count; vid += gridDim.x) {
    const u64 rec = l_list[vid];
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;
    const i64 cur_w = weights[cur];
    const i64 cur_maxw = maxw[cur];
    const bool excl_cur = mode == 1;
    bool vgate = true;
    if (mode == 2) {
      const i64 mnw = minw[cur];
      vgate = cur_w >= mnw && cur_w - u_w >= mnw;
    }
    i32 *grow = l_gains + static_cast<size_t>(vid) * k;

    BestState best{0, 0, 0, false};
    for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
      const i32 g = grow[c];
      grow[c] = 0; // reset for the next chunk
      if (g <= 0 || !vgate) {
        continue;
      }
      const i64 cw = weights[c];
      const i64 mw = maxw[c];
      const bool ok = (mode == 2)
                          ? accept_underload(c, cur, u_w, cw, mw, minw[c])
                          : accept_refine(c, cur, u_w, cw, mw, cur_w, cur_maxw, excl_cur);
      if (!ok) {
        continue;
      }
      const u64 h = tie_hash(iter_seed, u, c);
      if (key_better(g, h, c, best)) {
        best = BestState{g, h, c, true};
      }
    }
    const u32 lane = threadIdx.x & (kWave - 1);
    for (int off = 32; off > 0; off >>= 1) {
      const i32 og = __shfl_down(best.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
      const u32 oc = __shfl_down(best.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
      if (ohave && key_better(og, oh, oc, best)) {
        best = BestState{og, oh, oc, true};
      }
    }
    const u32 wave_in_wg = threadIdx.x >> 6;
    if (lane == 0) {
      red[wave_in_wg * 2] = (static_cast<i64>(best.gain) << 1) | (best.have ? 1 : 0);
      red[wave_in_wg * 2 + 1] = static_cast<i64>(best.h);
      reinterpret_cast<u32 *>(red + 8)[wave_in_wg] = best.c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      BestState total{0, 0, 0, false};
      const u32 waves = blockDim.x >> 6;
      for (u32 wv = 0; wv < waves; ++wv) {
        const i64 packed = red[wv * 2];
        if (packed & 1) {
          const i32 g = static_cast<i32>(packed >> 1);
          const u64 h = static_cast<u64>(red[wv * 2 + 1]);
          const u32 c = reinterpret_cast<u32 *>(red + 8)[wv];
          if (key_better(g, h, c, total)) {
            total = BestState{g, h, c, true};
          }
        }
      }
      if (!total.have && mode == 1 && cur_w > cur_maxw &&
          fallback != kInvalid && fallback != cur) {
        total = BestState{0, tie_hash(iter_seed, u, fallback), fallback, true};
      }
      if (total.have && total.c != cur) {
        slots[p - pos_lo] = Prop{u, total.c, p - chunk_base, static_cast<u32>(u_w)};
      } else {
        slots[p - pos_lo] = Prop{0u, kInvalid, 0u, 0u};
      }
    }
    __syncthreads();
  }
}

// Fallback for L entries beyond l_cap (pathological): one workgroup per
// vertex, whole row, replicated LDS histogram.
template <bool kUnitWeights, typename LT>
__global__ void k_phase_l_direct(
    u32 mode,
    u32 fallback,
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    u32 k,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ vwgt,
    const i32 *__restrict__ adjwgt,
    const u32 *__restrict__ labels,
    const LT *__restrict__ labels_s,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const i64 *__restrict__ minw,
    const u64 *__restrict__ l_list,
    const u32 *__restrict__ l_count,
    u32 l_cap,
    Prop *__restrict__ slots
) {
  extern __shared__ i32 lds[];
  const u32 R = gain_replicas(k);
  i32 *gains = lds;
  i64 *red = reinterpret_cast<i64 *>(lds + ((k * R + 1) & ~1u));

  const u32 count = *l_count;
  for (u32 vid = l_cap + blockIdx.x; vid < count; vid += gridDim.x) {
    for (u32 c = threadIdx.x; c < k * R; c += blockDim.x) {
      gains[c] = 0;
    }
    __syncthreads();

    const u64 rec = l_list[vid];
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);

    const u32 rep_off = (threadIdx.x % R) * k;
    for (u32 e = threadIdx.x; e < deg; e += blockDim.x) {
      const u32 v = adjncy[row + e];
      const i32 w = kUnitWeights ? 1 : adjwgt[row + e];
      atomicAdd(&gains[rep_off + labels_s[v]], w);
    }
    __syncthreads();

    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;
    const i64 cur_w = weights[cur];
    const i64 cur_maxw = maxw[cur];
    const bool excl_cur = mode == 1;
    bool vgate = true;
    if (mode == 2) {
      const i64 mnw = minw[cur];
      vgate = cur_w >= mnw && cur_w - u_w >= mnw;
    }

    BestState best{0, 0, 0, false};
    for (u32 c = threadIdx.x; vgate && c < k; c += blockDim.x) {
      i32 g = gains[c];
      for (u32 r = 1; r < R; ++r) {
        g += gains[r * k + c];
      }
      if (g <= 0) {
        continue;
      }
      const i64 cw = weights[c];
      const i64 mw = maxw[c];
      const bool ok = (mode == 2)
                          ? accept_underload(c, cur, u_w, cw, mw, minw[c])
                          : accept_refine(c, cur, u_w, cw, mw, cur_w, cur_maxw, excl_cur);
      if (!ok) {
        continue;
      }
      const u64 h = tie_hash(iter_seed, u, c);
      if (key_better(g, h, c, best)) {
        best = BestState{g, h, c, true};
      }
    }
    const u32 lane = threadIdx.x & (kWave - 1);
    for (int off = 32; off > 0; off >>= 1) {
      const i32 og = __shfl_down(best.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
      const u32 oc = __shfl_down(best.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
      if (ohave && key_better(og, oh, oc, best)) {
        best = BestState{og, oh, oc, true};
      }
    }
    const u32 wave_in_wg = threadIdx.x >> 6;
    if (lane == 0) {
      red[wave_in_wg * 2] = (static_cast<i64>(best.gain) << 1) | (best.have ? 1 : 0);
      red[wave_in_wg * 2 + 1] = static_cast<i64>(best.h);
      reinterpret_cast<u32 *>(red + 8)[wave_in_wg] = best.c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      BestState total{0, 0, 0, false};
      const u32 waves = blockDim.x >> 6;
      for (u32 wv = 0; wv < waves; ++wv) {
        const i64 packed = red[wv * 2];
        if (packed & 1) {
          const i32 g = static_cast<i32>(packed >> 1);
          const u64 h = static_cast<u64>(red[wv * 2 + 1]);
          const u32 c = reinterpret_cast<u32 *>(red + 8)[wv];
          if (key_better(g, h, c, total)) {
            total = BestState{g, h, c, true};
          }
        }
      }
      if (!total.have && mode == 1 && cur_w > cur_maxw &&
          fallback != kInvalid && fallback != cur) {
        total = BestState{0, tie_hash(iter_seed, u, fallback), fallback, true};
      }
      if (total.have && total.c != cur) {
        slots[p - pos_lo] = Prop{u, total.c, p - chunk_base, static_cast<u32>(u_w)};
      } else {
        slots[p - pos_lo] = Prop{0u, kInvalid, 0u, 0u};
      }
    }
    __syncthreads();
  }
}

// ==================== clustering (clusters = vertices) ====================
// LP clusterer instantiation (lp_clusterer.cc:23-28): ClusterID space = n,
// clusters start as singletons, uniform weight cap, favored-cluster tracking
// for two-hop merging. Gain maps are hash-based (cluster ids are unbounded):
// deg <= 16 register waterfall, deg <= 512 per-wave LDS hash, larger rows
// slice-parallel into a pooled global hash.

constexpr u32 kClusterMidDeg = 512; // per-wave LDS-hash path bound
constexpr u32 kHashSlots = 1024;    // per-wave LDS hash (8 KB per wave)
constexpr u32 kClusterM2Deg = 1536; // per-WG LDS-hash path bound (load <= 0.375)
constexpr u32 kM2HashSlots = 4096;  // per-WG LDS hash (32 KB per WG)

// S path for clustering: identical structure to k_phase_s, clusterer accept
// + favored-cluster argmax over all candidates.
__global__ void k_phase_s_c(
    u32 pos_lo,
    u32 pos_hi,
    u32 chunk_base,
    u32 n,
    u64 iter_seed,
    u32 max_degree,
    i64 maxw_uniform,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ vwgt,
    const i32 *__restrict__ adjwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const u32 *__restrict__ comm, // null = unrestricted (clusterer.h:35)
    const uint8_t *__restrict__ active,
    const uint8_t *__restrict__ unit_active,
    u32 *__restrict__ favored,
    Prop *__restrict__ slots
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 p = pos_lo + wave_id * 4 + sub;
  if (p >= pos_hi) {
    return;
  }

  const BlockPerm perm(n, iter_seed);
  // all 4 positions of this wave share one 64-vertex unit (slots pre-invalid)
  const u32 vb = perm.fp(p / kmp::kUnit);
  if (!unit_active[vb]) {
    return;
  }
  const u32 u = vb * kmp::kUnit + (p % kmp::kUnit);
  const u32 sidx = p - pos_lo;

  bool skip = false;
  u64 row = 0;
  u32 deg = 0;
  if (u >= n) {
    skip = true;
  } else {
    row = xadj[u];
    deg = static_cast<u32>(xadj[u + 1] - row);
    if (!active[u] || deg > max_degree) {
      skip = true;
    }
  }

  // M/L work lists are built by k_build_lists
  if (skip || deg > kSmallDeg) {
    return; // M/L own larger degrees
  }

  u32 c = kInvalid;
  i32 w = 0;
  if (slot < deg) {
    const u32 v = adjncy[row + slot];
    c = labels[v];
    w = adjwgt ? adjwgt[row + slot] : 1;
  }

  i32 gain = w;
  bool owner = (slot < deg);
  const u32 base = sub * 16;
  for (u32 j = 0; j < 16; ++j) {
    const u32 cj = __shfl(c, base + j, kWave);
    const i32 wj = __shfl(w, base + j, kWave);
    if (j != slot && c != kInvalid && cj == c) {
      gain += wj;
      if (j < slot) {
        owner = false;
      }
    }
  }

  const u32 cur = labels[u];
  const i32 u_w = vwgt ? vwgt[u] : 1;
  const i64 cur_w = weights[cur];

  BestState best{0, 0, 0, false};
  BestState fav{0, 0, 0, false};
  if (owner && c != kInvalid &&
      (comm == nullptr || comm[c] == comm[cur])) { // lp_clusterer.cc:193-194
    const u64 h = tie_hash(iter_seed, u, c);
    fav = BestState{gain, h, c, true};
    if (accept_cluster(c, cur, u_w, weights[c], maxw_uniform)) {
      best = BestState{gain, h, c, true};
    }
  }

  for (int off = 8; off > 0; off >>= 1) {
    {
      const i32 og = __shfl_down(best.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
      const u32 oc = __shfl_down(best.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
      if ((slot + off) < 16 && ohave && key_better(og, oh, oc, best)) {
        best = BestState{og, oh, oc, true};
      }
    }
    {
      const i32 og = __shfl_down(fav.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(fav.h), off, kWave);
      const u32 oc = __shfl_down(fav.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(fav.have), off, kWave);
      if ((slot + off) < 16 && ohave && key_better(og, oh, oc, fav)) {
        fav = BestState{og, oh, oc, true};
      }
    }
  }

  if (slot == 0) {
    // favored cluster for two-hop (label_propagation.h:517-535): stored only
    // while the vertex still sits in a light singleton cluster
    const bool store_favored = (u_w == cur_w) && (cur_w <= maxw_uniform / 2);
    if (store_favored) {
      favored[u] = fav.have ? fav.c : cur;
    }
    if (best.have && best.c != cur) {
      slots[sidx] = Prop{u, best.c, p - chunk_base, static_cast<u32>(u_w)};
    }
  }
}

// M path for clustering: one wave per position, per-wave LDS hash
// (kHashSlots key/value pairs), deg in (kSmallDeg, kClusterMidDeg].
template <bool kUnitWeights>
__global__ void k_phase_m_c(
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    i64 maxw_uniform,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const u32 *__restrict__ comm,
    const u64 *__restrict__ m_list,
    const u32 *__restrict__ m_count,
    u32 *__restrict__ favored,
    Prop *__restrict__ slots
) {
  extern __shared__ u32 ldsu[];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wave_in_wg = threadIdx.x >> 6;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  u32 *hkeys = ldsu + wave_in_wg * 2 * kHashSlots;
  i32 *hvals = reinterpret_cast<i32 *>(hkeys + kHashSlots);

  const u32 count = *m_count;
  for (u32 vid = wave_id; vid < count; vid += num_waves) {
  const u64 rec = m_list[vid];
  const u32 p = static_cast<u32>(rec >> 32);
  const u32 u = static_cast<u32>(rec);
  const u64 row = xadj[u];
  const u32 deg = static_cast<u32>(xadj[u + 1] - row);

  for (u32 s = lane; s < kHashSlots; s += kWave) {
    hkeys[s] = kInvalid;
    hvals[s] = 0;
  }
  __threadfence_block();

  for (u32 e = lane; e < deg; e += kWave) {
    const u32 v = adjncy[row + e];
    const u32 c = labels[v];
    const i32 w = kUnitWeights ? 1 : adjwgt[row + e];
    u32 s = hash_u32(c) & (kHashSlots - 1);
    while (true) {
      const u32 kcur = hkeys[s];
      if (kcur == c) {
        atomicAdd(&hvals[s], w);
        break;
      }
      if (kcur == kInvalid) {
        const u32 old = atomicCAS(&hkeys[s], kInvalid, c);
        if (old == kInvalid || old == c) {
          atomicAdd(&hvals[s], w);
          break;
        }
      }
      s = (s + 1) & (kHashSlots - 1);
    }
  }
  __threadfence_block();

  const u32 cur = labels[u];
  const i32 u_w = vwgt ? vwgt[u] : 1;
  const i64 cur_w = weights[cur];

  BestState best{0, 0, 0, false};
  BestState fav{0, 0, 0, false};
  for (u32 s = lane; s < kHashSlots; s += kWave) {
    const u32 c = hkeys[s];
    if (c == kInvalid) {
      continue;
    }
    const i32 g = hvals[s];
    if (g <= 0 || (comm != nullptr && comm[c] != comm[cur])) {
      continue;
    }
    const u64 h = tie_hash(iter_seed, u, c);
    if (key_better(g, h, c, fav)) {
      fav = BestState{g, h, c, true};
    }
    if (accept_cluster(c, cur, u_w, weights[c], maxw_uniform) && key_better(g, h, c, best)) {
      best = BestState{g, h, c, true};
    }
  }

  for (int off = 32; off > 0; off >>= 1) {
    {
      const i32 og = __shfl_down(best.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
      const u32 oc = __shfl_down(best.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
      if (ohave && key_better(og, oh, oc, best)) {
        best = BestState{og, oh, oc, true};
      }
    }
    {
      const i32 og = __shfl_down(fav.gain, off, kWave);
      const u64 oh = __shfl_down(static_cast<unsigned long long>(fav.h), off, kWave);
      const u32 oc = __shfl_down(fav.c, off, kWave);
      const int ohave = __shfl_down(static_cast<int>(fav.have), off, kWave);
      if (ohave && key_better(og, oh, oc, fav)) {
        fav = BestState{og, oh, oc, true};
      }
    }
  }

  if (lane == 0) {
    const bool store_favored = (u_w == cur_w) && (cur_w <= maxw_uniform / 2);
    if (store_favored) {
      favored[u] = fav.have ? fav.c : cur;
    }
    if (best.have && best.c != cur) {
      slots[p - pos_lo] = Prop{u, best.c, p - chunk_base, static_cast<u32>(u_w)};
    }
  }
  __threadfence_block(); // hash reuse across grid-stride iterations
  }
}

// M2 path for clustering: one 256-thread workgroup per vertex with a
// 4096-slot LDS hash -- absorbs the dense coarse-level rows
// (kClusterMidDeg < deg <= kClusterM2Deg) that otherwise take the pooled
// GLOBAL hash path (measured dominant in the multilevel pipeline).
template <bool kUnitWeights>
__global__ void k_phase_m2_c(
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    i64 maxw_uniform,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const u32 *__restrict__ comm,
    const u64 *__restrict__ m2_list,
    const u32 *__restrict__ m2_count,
    u32 *__restrict__ favored,
    Prop *__restrict__ slots
) {
  __shared__ u32 hkeys[kM2HashSlots];
  __shared__ i32 hvals[kM2HashSlots];
  __shared__ i64 red[24];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 count = *m2_count;
  for (u32 vid = blockIdx.x; vid < count; vid += gridDim.x) {
    const u64 rec = m2_list[vid];
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);

    for (u32 s = threadIdx.x; s < kM2HashSlots; s += blockDim.x) {
      hkeys[s] = kInvalid;
      hvals[s] = 0;
    }
    __syncthreads();
    for (u32 e = threadIdx.x; e < deg; e += blockDim.x) {
      const u32 v = adjncy[row + e];
      const u32 c = labels[v];
      const i32 w = kUnitWeights ? 1 : adjwgt[row + e];
      u32 s = hash_u32(c) & (kM2HashSlots - 1);
      while (true) {
        const u32 kcur = hkeys[s];
        if (kcur == c) {
          atomicAdd(&hvals[s], w);
          break;
        }
        if (kcur == kInvalid) {
          const u32 old = atomicCAS(&hkeys[s], kInvalid, c);
          if (old == kInvalid || old == c) {
            atomicAdd(&hvals[s], w);
            break;
          }
        }
        s = (s + 1) & (kM2HashSlots - 1);
      }
    }
    __syncthreads();

    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;
    const i64 cur_w = weights[cur];

    BestState best{0, 0, 0, false};
    BestState fav{0, 0, 0, false};
    for (u32 s = threadIdx.x; s < kM2HashSlots; s += blockDim.x) {
      const u32 c = hkeys[s];
      if (c == kInvalid) {
        continue;
      }
      const i32 g = hvals[s];
      if (g <= 0 || (comm != nullptr && comm[c] != comm[cur])) {
        continue;
      }
      const u64 h = tie_hash(iter_seed, u, c);
      if (key_better(g, h, c, fav)) {
        fav = BestState{g, h, c, true};
      }
      if (accept_cluster(c, cur, u_w, weights[c], maxw_uniform) && key_better(g, h, c, best)) {
        best = BestState{g, h, c, true};
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      {
        const i32 og = __shfl_down(best.gain, off, kWave);
        const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
        const u32 oc = __shfl_down(best.c, off, kWave);
        const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
        if (ohave && key_better(og, oh, oc, best)) {
          best = BestState{og, oh, oc, true};
        }
      }
      {
        const i32 og = __shfl_down(fav.gain, off, kWave);
        const u64 oh = __shfl_down(static_cast<unsigned long long>(fav.h), off, kWave);
        const u32 oc = __shfl_down(fav.c, off, kWave);
        const int ohave = __shfl_down(static_cast<int>(fav.have), off, kWave);
        if (ohave && key_better(og, oh, oc, fav)) {
          fav = BestState{og, oh, oc, true};
        }
      }
    }
    const u32 wave_in_wg = threadIdx.x >> 6;
    if (lane == 0) {
      red[wave_in_wg * 3] = (static_cast<i64>(best.gain) << 2) | (best.have ? 1 : 0) |
                            (fav.have ? 2 : 0);
      red[wave_in_wg * 3 + 1] = static_cast<i64>(best.h);
      red[wave_in_wg * 3 + 2] = static_cast<i64>(fav.h);
      reinterpret_cast<u32 *>(red + 12)[wave_in_wg * 2] = best.c;
      reinterpret_cast<u32 *>(red + 12)[wave_in_wg * 2 + 1] = fav.c;
      reinterpret_cast<i32 *>(red + 16)[wave_in_wg] = fav.gain;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      BestState tb{0, 0, 0, false};
      BestState tf{0, 0, 0, false};
      const u32 waves = blockDim.x >> 6;
      for (u32 wv = 0; wv < waves; ++wv) {
        const i64 packed = red[wv * 3];
        const i32 bg = static_cast<i32>(packed >> 2);
        if (packed & 1) {
          const u64 h = static_cast<u64>(red[wv * 3 + 1]);
          const u32 c = reinterpret_cast<u32 *>(red + 12)[wv * 2];
          if (key_better(bg, h, c, tb)) {
            tb = BestState{bg, h, c, true};
          }
        }
        if (packed & 2) {
          const i32 fg = reinterpret_cast<i32 *>(red + 16)[wv];
          const u64 h = static_cast<u64>(red[wv * 3 + 2]);
          const u32 c = reinterpret_cast<u32 *>(red + 12)[wv * 2 + 1];
          if (key_better(fg, h, c, tf)) {
            tf = BestState{fg, h, c, true};
          }
        }
      }
      const bool store_favored = (u_w == cur_w) && (cur_w <= maxw_uniform / 2);
      if (store_favored) {
        favored[u] = tf.have ? tf.c : cur;
      }
      if (tb.have && tb.c != cur) {
        slots[p - pos_lo] = Prop{u, tb.c, p - chunk_base, static_cast<u32>(u_w)};
      }
    }
    __syncthreads();
  }
}

// L prep for clustering: per-vertex slice prefix AND pooled-hash region
// prefix (region size = next power of two >= 2*deg). Writes the total
// region demand to *hacc_out: when it exceeds the pool, the host processes
// the L list in pool-sized batches (k_phase_l_sel_c clears each region
// after reading it, so the pool can be reused within a chunk).
__global__ void k_l_prep_c(
    const u64 *__restrict__ l_list,
    const u32 *__restrict__ l_count,
    const u64 *__restrict__ xadj,
    u32 l_cap,
    u32 *__restrict__ l_off,  // slice prefix
    u64 *__restrict__ l_hoff, // hash-region prefix
    u32 *__restrict__ l_hbits, // log2(region size)
    u32 *__restrict__ l_ccnt, // per-vertex claimed-slot counts (zeroed here)
    unsigned long long *__restrict__ hacc_out
) {
  __shared__ u64 red[17];
  const u32 count = *l_count < l_cap ? *l_count : l_cap;
  const u32 tid = threadIdx.x;
  const u32 lane = tid & (kWave - 1);
  u32 scarry = 0;
  u64 hcarry = 0;
  for (u32 base = 0; base < count; base += blockDim.x) {
    const u32 i = base + tid;
    u32 sc = 0;
    u64 hs = 0;
    if (i < count) {
      const u32 u = static_cast<u32>(l_list[i]);
      const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
      sc = (deg + kLSlice - 1) / kLSlice;
      u32 bits = 11; // >= 2048 slots
      while ((1u << bits) < 2 * deg) {
        ++bits;
      }
      l_hbits[i] = bits;
      l_ccnt[i] = 0;
      hs = 1ull << bits;
    }
    // joint block exclusive scan: region sizes in the high 32 bits, slice
    // counts in the low 32 (tile sums stay well under 2^32 each)
    u64 inc = (hs << 32) | sc;
    for (int off = 1; off < 64; off <<= 1) {
      const u64 o = __shfl_up(static_cast<unsigned long long>(inc), off, kWave);
      if (lane >= static_cast<u32>(off)) {
        inc += o;
      }
    }
    __syncthreads();
    if (lane == 63) {
      red[tid >> 6] = inc;
    }
    __syncthreads();
    u64 wbase = 0;
    for (u32 w = 0; w < (tid >> 6); ++w) {
      wbase += red[w];
    }
    const u64 ex = wbase + inc - ((hs << 32) | sc);
    if (i < count) {
      l_off[i] = scarry + static_cast<u32>(ex & 0xFFFFFFFFu);
      l_hoff[i] = hcarry + (ex >> 32);
    }
    u64 tsum = 0;
    for (u32 w = 0; w < blockDim.x / kWave; ++w) {
      tsum += red[w];
    }
    scarry += static_cast<u32>(tsum & 0xFFFFFFFFu);
    hcarry += tsum >> 32;
    __syncthreads();
  }
  if (tid == 0) {
    l_off[count] = scarry;
    l_hoff[count] = hcarry;
    *hacc_out = hcarry;
  }
}

// Slice-parallel accumulation into the pooled per-vertex global hash.
// Processes L vertices [vid_lo, vid_hi) with pool offsets rebased to
// l_hoff[vid_lo] (batched when a chunk's total region demand exceeds the
// pool; k_phase_l_sel_c clears each region so batches can reuse the pool).
template <bool kUnitWeights>
__global__ void k_phase_l_acc_c(
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const u32 *__restrict__ labels,
    const u64 *__restrict__ l_list,
    u32 vid_lo,
    u32 vid_hi,
    const u32 *__restrict__ l_off,
    const u64 *__restrict__ l_hoff,
    const u32 *__restrict__ l_hbits,
    u32 *__restrict__ pool_keys,
    i32 *__restrict__ pool_vals,
    u32 *__restrict__ l_clist, // claimed-slot lists (region/2 per vertex)
    u32 *__restrict__ l_ccnt   // per-vertex claimed counts
) {
  const u32 count = vid_hi;
  if (count <= vid_lo) {
    return;
  }
  const u64 hbase = l_hoff[vid_lo];
  const u32 s_lo = l_off[vid_lo];
  const u32 total = l_off[count];
  for (u32 s = s_lo + blockIdx.x; s < total; s += gridDim.x) {
    u32 lo = vid_lo, hi = count - 1;
    while (lo < hi) {
      const u32 mid = (lo + hi + 1) >> 1;
      if (l_off[mid] <= s) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    const u32 vid = lo;
    const u32 u = static_cast<u32>(l_list[vid]);
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    const u32 e_lo = (s - l_off[vid]) * kLSlice;
    const u32 e_hi = e_lo + kLSlice < deg ? e_lo + kLSlice : deg;
    const u64 roff = l_hoff[vid] - hbase;
    u32 *hk = pool_keys + roff;
    i32 *hv = pool_vals + roff;
    u32 *cl = l_clist + (roff >> 1); // region sizes are even powers of two
    const u32 mask = (1u << l_hbits[vid]) - 1;

    for (u32 e = e_lo + threadIdx.x; e < e_hi; e += blockDim.x) {
      const u32 v = adjncy[row + e];
      const u32 c = labels[v];
      const i32 w = kUnitWeights ? 1 : adjwgt[row + e];
      u32 slot = hash_u32(c) & mask;
      while (true) {
        const u32 kcur = hk[slot];
        if (kcur == c) {
          atomicAdd(&hv[slot], w);
          break;
        }
        if (kcur == kInvalid) {
          const u32 old = atomicCAS(&hk[slot], kInvalid, c);
          if (old == kInvalid || old == c) {
            if (old == kInvalid) {
              // record the claimed slot so selection/clearing is
              // O(distinct) instead of O(region)
              cl[atomicAdd(&l_ccnt[vid], 1u)] = slot;
            }
            atomicAdd(&hv[slot], w);
            break;
          }
        }
        slot = (slot + 1) & mask;
      }
    }
  }
}

// Selection per clustering L vertex: scan its hash region, clear it for the
// next chunk, write slot + favored.
__global__ void k_phase_l_sel_c(
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    u32 n,
    i64 maxw_uniform,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const u64 *__restrict__ l_list,
    u32 vid_lo,
    u32 vid_hi,
    const u64 *__restrict__ l_hoff,
    const u32 *__restrict__ l_hbits,
    u32 *__restrict__ pool_keys,
    i32 *__restrict__ pool_vals,
    const u32 *__restrict__ l_clist,
    const u32 *__restrict__ l_ccnt,
    const u32 *__restrict__ comm,
    u32 *__restrict__ favored,
    Prop *__restrict__ slots
) {
  __shared__ i64 red[24];
  const u64 hbase = vid_hi > vid_lo ? l_hoff[vid_lo] : 0;
  for (u32 vid = vid_lo + blockIdx.x; vid < vid_hi; vid += gridDim.x) {
    const u64 rec = l_list[vid];
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;
    const i64 cur_w = weights[cur];
    const u64 roff = l_hoff[vid] - hbase;
    u32 *hk = pool_keys + roff;
    i32 *hv = pool_vals + roff;
    const u32 *cl = l_clist + (roff >> 1);
    const u32 claimed = l_ccnt[vid];

    BestState best{0, 0, 0, false};
    BestState fav{0, 0, 0, false};
    for (u32 j = threadIdx.x; j < claimed; j += blockDim.x) {
      const u32 s = cl[j];
      const u32 c = hk[s];
      const i32 g = hv[s];
      hk[s] = kInvalid; // clear for the next chunk
      hv[s] = 0;
      if (g <= 0 || (comm != nullptr && comm[c] != comm[cur])) {
        continue;
      }
      const u64 h = tie_hash(iter_seed, u, c);
      if (key_better(g, h, c, fav)) {
        fav = BestState{g, h, c, true};
      }
      if (accept_cluster(c, cur, u_w, weights[c], maxw_uniform) && key_better(g, h, c, best)) {
        best = BestState{g, h, c, true};
      }
    }
    const u32 lane = threadIdx.x & (kWave - 1);
    for (int off = 32; off > 0; off >>= 1) {
      {
        const i32 og = __shfl_down(best.gain, off, kWave);
        const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
        const u32 oc = __shfl_down(best.c, off, kWave);
        const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
        if (ohave && key_better(og, oh, oc, best)) {
          best = BestState{og, oh, oc, true};
        }
      }
      {
        const i32 og = __shfl_down(fav.gain, off, kWave);
        const u64 oh = __shfl_down(static_cast<unsigned long long>(fav.h), off, kWave);
        const u32 oc = __shfl_down(fav.c, off, kWave);
        const int ohave = __shfl_down(static_cast<int>(fav.have), off, kWave);
        if (ohave && key_better(og, oh, oc, fav)) {
          fav = BestState{og, oh, oc, true};
        }
      }
    }
    const u32 wave_in_wg = threadIdx.x >> 6;
    if (lane == 0) {
      red[wave_in_wg * 3] = (static_cast<i64>(best.gain) << 2) | (best.have ? 1 : 0) |
                            (fav.have ? 2 : 0);
      red[wave_in_wg * 3 + 1] = static_cast<i64>(best.h);
      red[wave_in_wg * 3 + 2] = static_cast<i64>(fav.h);
      reinterpret_cast<u32 *>(red + 12)[wave_in_wg * 2] = best.c;
      reinterpret_cast<u32 *>(red + 12)[wave_in_wg * 2 + 1] = fav.c;
      reinterpret_cast<i32 *>(red + 16)[wave_in_wg] = fav.gain;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      BestState tb{0, 0, 0, false};
      BestState tf{0, 0, 0, false};
      const u32 waves = blockDim.x >> 6;
      for (u32 wv = 0; wv < waves; ++wv) {
        const i64 packed = red[wv * 3];
        const i32 bg = static_cast<i32>(packed >> 2);
        if (packed & 1) {
          const u64 h = static_cast<u64>(red[wv * 3 + 1]);
          const u32 c = reinterpret_cast<u32 *>(red + 12)[wv * 2];
          if (key_better(bg, h, c, tb)) {
            tb = BestState{bg, h, c, true};
          }
        }
        if (packed & 2) {
          const i32 fg = reinterpret_cast<i32 *>(red + 16)[wv];
          const u64 h = static_cast<u64>(red[wv * 3 + 2]);
          const u32 c = reinterpret_cast<u32 *>(red + 12)[wv * 2 + 1];
          if (key_better(fg, h, c, tf)) {
            tf = BestState{fg, h, c, true};
          }
        }
      }
      const bool store_favored = (u_w == cur_w) && (cur_w <= maxw_uniform / 2);
      if (store_favored) {
        favored[u] = tf.have ? tf.c : cur;
      }
      if (tb.have && tb.c != cur) {
        slots[p - pos_lo] = Prop{u, tb.c, p - chunk_base, static_cast<u32>(u_w)};
      }
    }
    __syncthreads();
  }
}

// ============ refine / balance phase A for k > kMaxDenseK ============
// The dense gain tables of k_phase_m / k_phase_l_* grow with k; above
// kMaxDenseK the refiner takes the clusterer's containers instead, which are
// sized by degree (a vertex has at most deg distinct adjacent blocks): the
// per-wave 1024-slot LDS hash (kSmallDeg < deg <= kClusterMidDeg), the
// per-workgroup 4096-slot LDS hash (<= kClusterM2Deg) and the pooled global
// hash (k_l_prep_c + k_phase_l_acc_c, reused as they are). Selection restates
// k_phase_m's: skip g <= 0, accept_refine, key (gain, tie_hash, c), mode-1
// fallback. All sums are integer and the key is a total order, so the result
// does not depend on slot order or on the order of the atomics. Modes 0 and
// 1 only (underload stays on the dense path). LT is the gather type: the u16
// shadow for k <= 65536, the u32 labels themselves beyond.

__device__ inline void lds_hash_add(u32 *hkeys, i32 *hvals, u32 mask, u32 c, i32 w) {
  u32 s = hash_u32(c) & mask;
  while (true) {
    const u32 kcur = hkeys[s];
    if (kcur == c) {
      atomicAdd(&hvals[s], w);
      break;
    }
    if (kcur == kInvalid) {
      const u32 old = atomicCAS(&hkeys[s], kInvalid, c);
      if (old == kInvalid || old == c) {
        atomicAdd(&hvals[s], w);
        break;
      }
    }
    s = (s + 1) & mask;
  }
}

// One candidate of the refiner's select; cw / mw are weights[c] / maxw[c].
__device__ inline void refine_consider(
    BestState &best, u32 c, i32 g, i64 cw, i64 mw, u32 cur, i32 u_w, i64 cur_w, i64 cur_maxw,
    bool excl_cur, u64 iter_seed, u32 u
) {
  if (g <= 0 || !accept_refine(c, cur, u_w, cw, mw, cur_w, cur_maxw, excl_cur)) {
    return;
  }
  const u64 h = tie_hash(iter_seed, u, c);
  if (key_better(g, h, c, best)) {
    best = BestState{g, h, c, true};
  }
}

__device__ inline BestState wave_reduce_best(BestState best) {
  for (int off = 32; off > 0; off >>= 1) {
    const i32 og = __shfl_down(best.gain, off, kWave);
    const u64 oh = __shfl_down(static_cast<unsigned long long>(best.h), off, kWave);
    const u32 oc = __shfl_down(best.c, off, kWave);
    const int ohave = __shfl_down(static_cast<int>(best.have), off, kWave);
    if (ohave && key_better(og, oh, oc, best)) {
      best = BestState{og, oh, oc, true};
    }
  }
  return best; // lane 0 holds the wave's best
}

// Workgroup argmax (up to 4 waves) through red[12]; thread 0 gets the result.
// The caller synchronizes before red is used again.
__device__ inline BestState wg_reduce_best(BestState best, i64 *red) {
  best = wave_reduce_best(best);
  const u32 wave_in_wg = threadIdx.x >> 6;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[wave_in_wg * 2] = (static_cast<i64>(best.gain) << 1) | (best.have ? 1 : 0);
    red[wave_in_wg * 2 + 1] = static_cast<i64>(best.h);
    reinterpret_cast<u32 *>(red + 8)[wave_in_wg] = best.c;
  }
  __syncthreads();
  BestState tb{0, 0, 0, false};
  if (threadIdx.x == 0) {
    const u32 waves = blockDim.x >> 6;
    for (u32 wv = 0; wv < waves; ++wv) {
      const i64 packed = red[wv * 2];
      if (packed & 1) {
        const i32 g = static_cast<i32>(packed >> 1);
        const u64 h = static_cast<u64>(red[wv * 2 + 1]);
        const u32 c = reinterpret_cast<u32 *>(red + 8)[wv];
        if (key_better(g, h, c, tb)) {
          tb = BestState{g, h, c, true};
        }
      }
    }
  }
  return tb;
}

// The slot of a listed vertex: its proposal, the mode-1 fallback, or invalid.
__device__ inline void write_refine_slot(
    Prop *__restrict__ slots, u32 sidx, u32 rank, BestState fin, u32 mode, u32 fallback,
    u64 iter_seed, u32 u, u32 cur, i32 u_w, i64 cur_w, i64 cur_maxw
) {
  if (!fin.have && mode == 1 && cur_w > cur_maxw && fallback != kInvalid && fallback != cur) {
    fin = BestState{0, tie_hash(iter_seed, u, fallback), fallback, true};
  }
  if (fin.have && fin.c != cur) {
    slots[sidx] = Prop{u, fin.c, rank, static_cast<u32>(u_w)};
  } else {
    slots[sidx] = Prop{0u, kInvalid, 0u, 0u};
  }
}

constexpr u32 kHSelBatch = 4; // hash slots examined together in the selection

// M tier: one wavefront per listed vertex, per-wave kHashSlots LDS hash.
// blockDim.x = 256; dynamic LDS = 4 * 2 * kHashSlots * 4 bytes. The table is
// cleared once; afterwards the selection empties every slot it reads.
template <bool kUnitWeights, typename LT>
__global__ void __launch_bounds__(256) k_phase_m_h(
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    u32 mode,
    u32 fallback,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const LT *__restrict__ labels_s,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const u64 *__restrict__ m_list,
    const u32 *__restrict__ m_count,
    Prop *__restrict__ slots
) {
  extern __shared__ u32 ldsu[];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wave_in_wg = threadIdx.x >> 6;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  u32 *hkeys = ldsu + wave_in_wg * 2 * kHashSlots;
  i32 *hvals = reinterpret_cast<i32 *>(hkeys + kHashSlots);

  const u32 count = *m_count;
  if (wave_id >= count) {
    return;
  }
  for (u32 s = lane; s < kHashSlots; s += kWave) {
    hkeys[s] = kInvalid;
    hvals[s] = 0;
  }
  __threadfence_block(); // LDS ordering; the table is private to this wave

  const u32 last = count - 1;
  u64 rec_n = m_list[wave_id]; // record of the next entry, read an entry ahead
  for (u32 vid = wave_id; vid < count; vid += num_waves) {
    const u64 rec = rec_n;
    {
      const u64 i1 = static_cast<u64>(vid) + num_waves;
      rec_n = m_list[i1 < last ? i1 : last];
    }
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    // per-vertex state, issued ahead of the edge loop
    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;

    // kMUnroll adjncy loads, then the gathers, then the LDS atomics; lanes
    // past the row re-read its last edge (listed rows have deg > kSmallDeg)
    // and add nothing
    for (u32 eb = 0; eb < deg; eb += kMUnroll * kWave) {
      u32 vv[kMUnroll];
      i32 wv[kMUnroll];
      u32 cv[kMUnroll];
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        const u32 e = eb + lane + j * kWave;
        const u32 ec = e < deg ? e : deg - 1;
        vv[j] = __builtin_nontemporal_load(&adjncy[row + ec]);
        wv[j] = kUnitWeights ? 1 : adjwgt[row + ec];
      }
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        cv[j] = labels_s[vv[j]];
      }
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        if (eb + lane + j * kWave < deg) {
          lds_hash_add(hkeys, hvals, kHashSlots - 1, cv[j], wv[j]);
        }
      }
    }
    __threadfence_block();

    const i64 cur_w = weights[cur];
    const i64 cur_maxw = maxw[cur];
    const bool excl_cur = mode == 1;

    BestState best{0, 0, 0, false};
    for (u32 sb = 0; sb < kHashSlots; sb += kHSelBatch * kWave) {
      u32 cc[kHSelBatch];
      i32 gg[kHSelBatch];
      i64 cw[kHSelBatch];
      i64 mw[kHSelBatch];
#pragma unroll
      for (u32 j = 0; j < kHSelBatch; ++j) {
        const u32 s = sb + j * kWave + lane;
        cc[j] = hkeys[s];
        gg[j] = hvals[s];
        if (cc[j] != kInvalid) {
          hkeys[s] = kInvalid; // empty for the next vertex
          hvals[s] = 0;
        }
      }
#pragma unroll
      for (u32 j = 0; j < kHSelBatch; ++j) {
        const bool live = cc[j] != kInvalid && gg[j] > 0;
        cw[j] = live ? weights[cc[j]] : 0;
        mw[j] = live ? maxw[cc[j]] : 0;
      }
#pragma unroll
      for (u32 j = 0; j < kHSelBatch; ++j) {
        if (cc[j] != kInvalid) {
          refine_consider(best, cc[j], gg[j], cw[j], mw[j], cur, u_w, cur_w, cur_maxw, excl_cur,
                          iter_seed, u);
        }
      }
    }
    best = wave_reduce_best(best);
    if (lane == 0) {
      write_refine_slot(slots, p - pos_lo, p - chunk_base, best, mode, fallback, iter_seed, u, cur,
                        u_w, cur_w, cur_maxw);
    }
    __threadfence_block(); // table reuse across grid-stride iterations
  }
}

// M2 tier: one 256-thread workgroup per listed vertex, kM2HashSlots LDS hash
// (kClusterMidDeg < deg <= kClusterM2Deg, load <= 0.375).
template <bool kUnitWeights, typename LT>
__global__ void __launch_bounds__(256) k_phase_m2_h(
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    u32 mode,
    u32 fallback,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const LT *__restrict__ labels_s,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const u64 *__restrict__ m2_list,
    const u32 *__restrict__ m2_count,
    Prop *__restrict__ slots
) {
  __shared__ u32 hkeys[kM2HashSlots];
  __shared__ i32 hvals[kM2HashSlots];
  __shared__ i64 red[12];
  const u32 count = *m2_count;
  if (blockIdx.x >= count) {
    return;
  }
  for (u32 s = threadIdx.x; s < kM2HashSlots; s += blockDim.x) {
    hkeys[s] = kInvalid;
    hvals[s] = 0;
  }
  __syncthreads();
  for (u32 vid = blockIdx.x; vid < count; vid += gridDim.x) {
    const u64 rec = m2_list[vid];
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;

    for (u32 eb = 0; eb < deg; eb += kMUnroll * blockDim.x) {
      u32 vv[kMUnroll];
      i32 wv[kMUnroll];
      u32 cv[kMUnroll];
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        const u32 e = eb + threadIdx.x + j * blockDim.x;
        const u32 ec = e < deg ? e : deg - 1;
        vv[j] = __builtin_nontemporal_load(&adjncy[row + ec]);
        wv[j] = kUnitWeights ? 1 : adjwgt[row + ec];
      }
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        cv[j] = labels_s[vv[j]];
      }
#pragma unroll
      for (u32 j = 0; j < kMUnroll; ++j) {
        if (eb + threadIdx.x + j * blockDim.x < deg) {
          lds_hash_add(hkeys, hvals, kM2HashSlots - 1, cv[j], wv[j]);
        }
      }
    }
    __syncthreads();

    const i64 cur_w = weights[cur];
    const i64 cur_maxw = maxw[cur];
    const bool excl_cur = mode == 1;

    BestState best{0, 0, 0, false};
    for (u32 sb = 0; sb < kM2HashSlots; sb += kHSelBatch * blockDim.x) {
      u32 cc[kHSelBatch];
      i32 gg[kHSelBatch];
      i64 cw[kHSelBatch];
      i64 mw[kHSelBatch];
#pragma unroll
      for (u32 j = 0; j < kHSelBatch; ++j) {
        const u32 s = sb + j * blockDim.x + threadIdx.x;
        cc[j] = hkeys[s];
        gg[j] = hvals[s];
        if (cc[j] != kInvalid) {
          hkeys[s] = kInvalid; // empty for the next vertex
          hvals[s] = 0;
        }
      }
#pragma unroll
      for (u32 j = 0; j < kHSelBatch; ++j) {
        const bool live = cc[j] != kInvalid && gg[j] > 0;
        cw[j] = live ? weights[cc[j]] : 0;
        mw[j] = live ? maxw[cc[j]] : 0;
      }
#pragma unroll
      for (u32 j = 0; j < kHSelBatch; ++j) {
        if (cc[j] != kInvalid) {
          refine_consider(best, cc[j], gg[j], cw[j], mw[j], cur, u_w, cur_w, cur_maxw, excl_cur,
                          iter_seed, u);
        }
      }
    }
    const BestState tb = wg_reduce_best(best, red);
    if (threadIdx.x == 0) {
      write_refine_slot(slots, p - pos_lo, p - chunk_base, tb, mode, fallback, iter_seed, u, cur,
                        u_w, cur_w, cur_maxw);
    }
    __syncthreads(); // red and the emptied table, before the next vertex
  }
}

// L tier selection: the refiner's rule over each region's claimed-slot list
// (filled by k_phase_l_acc_c); clears the region after reading it, so that
// batches and later chunks can reuse the pool.
__global__ void __launch_bounds__(256) k_phase_l_sel_h(
    u32 pos_lo,
    u32 chunk_base,
    u64 iter_seed,
    u32 mode,
    u32 fallback,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const u64 *__restrict__ l_list,
    u32 vid_lo,
    u32 vid_hi,
    const u64 *__restrict__ l_hoff,
    u32 *__restrict__ pool_keys,
    i32 *__restrict__ pool_vals,
    const u32 *__restrict__ l_clist,
    const u32 *__restrict__ l_ccnt,
    Prop *__restrict__ slots
) {
  __shared__ i64 red[12];
  const u64 hbase = vid_hi > vid_lo ? l_hoff[vid_lo] : 0;
  for (u32 vid = vid_lo + blockIdx.x; vid < vid_hi; vid += gridDim.x) {
    const u64 rec = l_list[vid];
    const u32 p = static_cast<u32>(rec >> 32);
    const u32 u = static_cast<u32>(rec);
    const u32 cur = labels[u];
    const i32 u_w = vwgt ? vwgt[u] : 1;
    const i64 cur_w = weights[cur];
    const i64 cur_maxw = maxw[cur];
    const bool excl_cur = mode == 1;
    const u64 roff = l_hoff[vid] - hbase;
    u32 *hk = pool_keys + roff;
    i32 *hv = pool_vals + roff;
    const u32 *cl = l_clist + (roff >> 1);
    const u32 claimed = l_ccnt[vid];

    BestState best{0, 0, 0, false};
    for (u32 j = threadIdx.x; j < claimed; j += blockDim.x) {
      const u32 s = cl[j];
      const u32 c = hk[s];
      const i32 g = hv[s];
      hk[s] = kInvalid; // clear for the next batch / chunk
      hv[s] = 0;
      if (g > 0) {
        refine_consider(best, c, g, weights[c], maxw[c], cur, u_w, cur_w, cur_maxw, excl_cur,
                        iter_seed, u);
      }
    }
    const BestState tb = wg_reduce_best(best, red);
    if (threadIdx.x == 0) {
      write_refine_slot(slots, p - pos_lo, p - chunk_base, tb, mode, fallback, iter_seed, u, cur,
                        u_w, cur_w, cur_maxw);
    }
    __syncthreads();
  }
}

// Block weights by global integer atomics (k > kMaxDenseK, where
// k_init_weights' k-sized LDS table does not fit). A wave whose vertices all
// sit in one block (the balancer's everything-in-block-0 start) adds once.
__global__ void k_init_weights_direct(
    u32 n,
    const u32 *__restrict__ labels,
    const i32 *__restrict__ vwgt,
    unsigned long long *__restrict__ weights
) {
  const u32 stride = gridDim.x * blockDim.x;
  const u32 lane = threadIdx.x & (kWave - 1);
  // whole waves iterate together (the bound is rounded up to the wave)
  const u32 n_up = (n + kWave - 1) & ~(kWave - 1);
  for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < n_up; u += stride) {
    const bool valid = u < n;
    const u32 l = valid ? labels[u] : kInvalid;
    unsigned long long w = valid ? static_cast<unsigned long long>(vwgt ? vwgt[u] : 1) : 0ull;
    const u32 l0 = __shfl(l, 0, kWave); // lane 0 is valid whenever any lane is
    if (__all(!valid || l == l0)) {
      for (int off = 32; off > 0; off >>= 1) {
        w += __shfl_down(w, off, kWave);
      }
      if (lane == 0 && w) {
        atomicAdd(&weights[l0], w);
      }
    } else if (valid) {
      atomicAdd(&weights[l], w);
    }
  }
}

// -------- big-k commit variants (cluster space = n) --------

// Reset dep entries touched by this chunk's proposals (idempotent).
__global__ void k_dep_reset_touched(
    const Prop *__restrict__ props,
    u32 count,
    const u32 *__restrict__ labels,
    unsigned long long *__restrict__ dep
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    dep[labels[props[i].u]] = 0;
  }
}

// Departures via direct global atomics (sources spread over many clusters).
__global__ void k_dep_direct(
    const u32 *__restrict__ order,
    const Prop *__restrict__ props,
    const u32 *__restrict__ sto,
    u32 count,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ prefix_len,
    const u32 *__restrict__ labels,
    unsigned long long *__restrict__ dep
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 to = sto[i];
  if (i - seg_begin[to] < prefix_len[to]) {
    const Prop pr = props[order[i]];
    atomicAdd(&dep[labels[pr.u]], static_cast<unsigned long long>(pr.w));
  }
}

// Head-driven cutoff: one thread per SEGMENT HEAD in the sorted proposals
// (avoids an O(num_clusters) sweep per fixpoint round).
__global__ void k_cutoff_heads(
    const u32 *__restrict__ sto,
    u32 count,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ seg_end,
    u32 *__restrict__ prefix_len,
    const i64 *__restrict__ pw,
    const i64 *__restrict__ weights,
    i64 maxw_uniform,
    const unsigned long long *__restrict__ dep,
    int *__restrict__ changed
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 c = sto[i];
  const u32 b = seg_begin[c];
  if (i != b) {
    return; // not the segment head
  }
  const i64 capacity = maxw_uniform - weights[c] + static_cast<i64>(dep[c]);
  const u32 old_len = prefix_len[c];
  u32 lo = 0, hi = old_len;
  while (lo < hi) {
    const u32 mid = (lo + hi + 1) >> 1;
    if (pw[b + mid - 1] <= capacity) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  if (lo < old_len) {
    prefix_len[c] = lo;
    atomicExch(changed, 1);
  }
}

__global__ void k_seg_len_heads(
    const u32 *__restrict__ sto,
    u32 count,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ seg_end,
    u32 *__restrict__ prefix_len
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 c = sto[i];
  if (i == seg_begin[c]) {
    prefix_len[c] = seg_end[c] - seg_begin[c];
  }
}

// Weight updates for big-k: arrivals head-driven, departures via a
// once-per-cluster atomic exchange of the final dep value.
__global__ void k_weights_update_big(
    const u32 *__restrict__ order,
    const Prop *__restrict__ props,
    const u32 *__restrict__ sto,
    u32 count,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ prefix_len,
    const i64 *__restrict__ pw,
    const u32 *__restrict__ labels,
    unsigned long long *__restrict__ dep,
    i64 *__restrict__ weights
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 to = sto[i];
  const u32 b = seg_begin[to];
  if (i == b && prefix_len[to] > 0) {
    atomicAdd(reinterpret_cast<unsigned long long *>(&weights[to]),
              static_cast<unsigned long long>(pw[b + prefix_len[to] - 1]));
  }
  // departures: first toucher per source cluster applies the whole dep
  const u32 from = labels[props[order[i]].u];
  const unsigned long long d = atomicExch(&dep[from], 0ull);
  if (d) {
    atomicAdd(reinterpret_cast<unsigned long long *>(&weights[from]),
              static_cast<unsigned long long>(-static_cast<i64>(d)));
  }
}

// Count clusters emptied by this chunk (distinct sources with final weight
// zero); eflag entries are reset by k_emptied_reset.
__global__ void k_emptied_count(
    const u32 *__restrict__ order,
    const Prop *__restrict__ props,
    const u32 *__restrict__ sto,
    u32 count,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ prefix_len,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    uint8_t *__restrict__ eflag,
    unsigned long long *__restrict__ emptied
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 to = sto[i];
  if (i - seg_begin[to] >= prefix_len[to]) {
    return;
  }
  const u32 from = labels[props[order[i]].u];
  if (weights[from] == 0) {
    // no 8-bit atomicExch: use 32-bit CAS on the aligned word
    u32 *word = reinterpret_cast<u32 *>(reinterpret_cast<uintptr_t>(&eflag[from]) & ~3ull);
    const u32 shift = (from & 3u) * 8;
    const u32 bit = 1u << shift;
    const u32 old = atomicOr(word, bit);
    if ((old & bit) == 0) {
      atomicAdd(emptied, 1ull);
    }
  }
}

__global__ void k_emptied_reset(
    const u32 *__restrict__ order,
    const Prop *__restrict__ props,
    u32 count,
    const u32 *__restrict__ labels,
    uint8_t *__restrict__ eflag
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    eflag[labels[props[i].u]] = 0;
  }
}

// -------- post passes (clusterer) --------

__global__ void k_iota(u32 n, u32 *__restrict__ a) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    a[i] = i;
  }
}

__global__ void k_init_cluster_weights(
    u32 n, const i32 *__restrict__ vwgt, i64 *__restrict__ weights
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    weights[i] = vwgt ? vwgt[i] : 1;
  }
}

// Two-hop candidate collection (label_propagation.h:939-975 threadwise
// considered-set): deg > 0, still in its own singleton cluster at its
// initial weight, light. Slot-write + stable select keeps ascending-u order.
__global__ void k_twohop_cand(
    u32 n,
    i64 maxw_uniform,
    const u64 *__restrict__ xadj,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ labels,
    const i64 *__restrict__ weights,
    const u32 *__restrict__ favored,
    u64 *__restrict__ cand_slots // (favored << 32) | u, or ~0 invalid
) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) {
    return;
  }
  u64 out = ~0ull;
  const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
  if (deg > 0 && labels[u] == u) {
    const i64 w = weights[u];
    const i64 vw = vwgt ? vwgt[u] : 1;
    if (w == vw && w <= maxw_uniform / 2) {
      out = (static_cast<u64>(favored[u]) << 32) | u;
    }
  }
  cand_slots[u] = out;
}

struct CandValid {
  __host__ __device__ bool operator()(const u64 &v) const { return v != ~0ull; }
};

// Pair consecutive candidates with equal favored cluster: even rank joins
// the preceding candidate's (singleton) cluster. rank = 1-based rank within
// the favored segment (scan_by_key output). Always fits: both weights
// <= max/2 (label_propagation.h:977-1002 match semantics).
__global__ void k_twohop_pair(
    const u64 *__restrict__ cand_sorted,
    const u32 *__restrict__ rank, // 1-based within favored segment
    u32 count,
    u32 *__restrict__ labels,
    i64 *__restrict__ weights,
    unsigned long long *__restrict__ merged
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u64 local = 0;
  if (i < count && (rank[i] & 1u) == 0) {
    const u32 u = static_cast<u32>(cand_sorted[i]);
    const u32 rep = static_cast<u32>(cand_sorted[i - 1]);
    labels[u] = rep;
    // no atomics needed: each candidate appears in exactly one pair
    weights[rep] += weights[u];
    weights[u] = 0;
    local = 1;
  }
  for (int off = 32; off > 0; off >>= 1) {
    local += __shfl_down(static_cast<unsigned long long>(local), off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && local) {
    atomicAdd(merged, static_cast<unsigned long long>(local));
  }
}

__global__ void k_extract_fav(const u64 *__restrict__ cand, u32 count, u32 *__restrict__ fav) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    fav[i] = static_cast<u32>(cand[i] >> 32);
  }
}

__global__ void k_ones(u32 count, u32 *__restrict__ a) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    a[i] = 1;
  }
}

// Apply host-computed isolated-node matches: pairs (u -> rep).
__global__ void k_apply_pairs(
    const u64 *__restrict__ pairs, // (rep << 32) | u
    u32 count,
    u32 *__restrict__ labels,
    i64 *__restrict__ weights
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    const u32 u = static_cast<u32>(pairs[i]);
    const u32 rep = static_cast<u32>(pairs[i] >> 32);
    labels[u] = rep;
    weights[rep] += weights[u];
    weights[u] = 0;
  }
}

// Count non-empty clusters.
__global__ void k_count_nonempty(
    u32 n, const i64 *__restrict__ weights, unsigned long long *__restrict__ out
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u64 local = (i < n && weights[i] != 0) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) {
    local += __shfl_down(static_cast<unsigned long long>(local), off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && local) {
    atomicAdd(out, static_cast<unsigned long long>(local));
  }
}

// -------------------------------------------------------------- commit
__global__ void k_make_keys(
    const Prop *__restrict__ props, u32 count, u32 *__restrict__ keys, u32 *__restrict__ vals
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    keys[i] = props[i].to;
    vals[i] = i;
  }
}

__global__ void k_extract_w(
    const u32 *__restrict__ order, const Prop *__restrict__ props, u32 count, i64 *__restrict__ sw
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    sw[i] = static_cast<i64>(static_cast<i32>(props[order[i]].w));
  }
}

__global__ void k_seg_bounds(
    const u32 *__restrict__ sto, u32 count, u32 *__restrict__ seg_begin, u32 *__restrict__ seg_end
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 to = sto[i];
  if (i == 0 || sto[i - 1] != to) {
    seg_begin[to] = i;
  }
  if (i == count - 1 || sto[i + 1] != to) {
    seg_end[to] = i + 1;
  }
}

// Per-WG LDS histogram of departures (one global atomic per cluster per WG;
// a per-proposal global atomic on k addresses serializes badly). Dynamic
// LDS: k x u64. Grid-stride so the WG count stays bounded.
__global__ void k_dep(
    const u32 *__restrict__ order,
    const Prop *__restrict__ props,
    const u32 *__restrict__ sto,
    u32 count,
    u32 k,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ prefix_len,
    const u32 *__restrict__ labels,
    unsigned long long *__restrict__ dep
) {
  extern __shared__ unsigned long long hist[];
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    hist[c] = 0;
  }
  __syncthreads();
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const u32 to = sto[i];
    if (i - seg_begin[to] < prefix_len[to]) {
      const Prop pr = props[order[i]];
      atomicAdd(&hist[labels[pr.u]], static_cast<unsigned long long>(pr.w));
    }
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    if (hist[c]) {
      atomicAdd(&dep[c], hist[c]);
    }
  }
}

__global__ void k_cutoff(
    u32 k_or_n,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ seg_end,
    u32 *__restrict__ prefix_len,
    const i64 *__restrict__ pw, // within-segment inclusive prefix weights
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    const unsigned long long *__restrict__ dep,
    int *__restrict__ changed
) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k_or_n) {
    return;
  }
  const u32 b = seg_begin[c], e = seg_end[c];
  if (e <= b) {
    return;
  }
  const i64 capacity = maxw[c] - weights[c] + static_cast<i64>(dep[c]);
  const u32 old_len = prefix_len[c];
  u32 lo = 0, hi = old_len;
  while (lo < hi) {
    const u32 mid = (lo + hi + 1) >> 1;
    if (pw[b + mid - 1] <= capacity) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  if (lo < old_len) {
    prefix_len[c] = lo;
    atomicExch(changed, 1);
  }
}

__global__ void k_weights_update(
    u32 k_or_n,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ seg_end,
    const u32 *__restrict__ prefix_len,
    const i64 *__restrict__ pw,
    const unsigned long long *__restrict__ dep,
    i64 *__restrict__ weights
) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k_or_n) {
    return;
  }
  i64 arr = 0;
  const u32 b = seg_begin[c], e = seg_end[c];
  if (e > b && prefix_len[c] > 0) {
    arr = pw[b + prefix_len[c] - 1];
  }
  const i64 delta = arr - static_cast<i64>(dep[c]);
  if (delta != 0) {
    weights[c] += delta;
  }
}

__global__ void k_apply(
    const u32 *__restrict__ order,
    const Prop *__restrict__ props,
    const u32 *__restrict__ sto,
    u32 count,
    const u32 *__restrict__ seg_begin,
    const u32 *__restrict__ prefix_len,
    u32 *__restrict__ labels,
    uint16_t *__restrict__ labels16, // refine shadow; null for clustering
    uint8_t *__restrict__ labels8,   // u8 shadow; null unless k <= 256
    u32 *__restrict__ admitted_flags, // per sorted index
    unsigned long long *__restrict__ moves
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u64 local = 0;
  if (i < count) {
    const u32 to = sto[i];
    const bool admitted = (i - seg_begin[to]) < prefix_len[to];
    admitted_flags[i] = admitted ? 1u : 0u;
    if (admitted) {
      const u32 u = props[order[i]].u;
      labels[u] = to;
      if (labels16 != nullptr) {
        labels16[u] = static_cast<uint16_t>(to);
      }
      if (labels8 != nullptr) {
        labels8[u] = static_cast<uint8_t>(to);
      }
      local = 1;
    }
  }
  // wave-aggregated move count
  for (int off = 32; off > 0; off >>= 1) {
    local += __shfl_down(static_cast<unsigned long long>(local), off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && local) {
    atomicAdd(moves, static_cast<unsigned long long>(local));
  }
}

// Clear active flags for processed vertices of the WHOLE chunk (identical on
// every rank) and count scanned arcs (WG-aggregated).
__global__ void k_clear_active(
    u32 chunk_lo,
    u32 chunk_hi,
    u32 n,
    u64 iter_seed,
    u32 max_degree,
    const u64 *__restrict__ xadj,
    uint8_t *__restrict__ active,
    uint8_t *__restrict__ unit_active,
    unsigned long long *__restrict__ arcs
) {
  __shared__ unsigned long long wg_sum[4];
  const u32 tid = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 p = chunk_lo + tid;
  const BlockPerm perm(n, iter_seed);
  const u32 lane0 = threadIdx.x & (kWave - 1);

  // one wave covers exactly one 64-vertex unit (chunks are 64-aligned):
  // skip fully-inactive units, clear the unit bit after processing (the
  // activation kernel re-sets it for units that received movers)
  u32 vb = 0;
  bool unit_on = false;
  if (p < chunk_hi) {
    vb = perm.fp(p / kmp::kUnit);
    unit_on = unit_active[vb] != 0;
  }

  u64 my_deg = 0;
  if (p < chunk_hi && unit_on) {
    const u32 u = vb * kmp::kUnit + (p % kmp::kUnit);
    if (u < n) {
      const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
      if (deg <= max_degree && active[u]) {
        my_deg = deg;
        active[u] = 0;
      }
    }
    if (lane0 == 0) {
      unit_active[vb] = 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    my_deg += __shfl_down(static_cast<unsigned long long>(my_deg), off, kWave);
  }
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wave_in_wg = threadIdx.x >> 6;
  if (lane == 0) {
    wg_sum[wave_in_wg] = my_deg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = wg_sum[0] + wg_sum[1] + wg_sum[2] + wg_sum[3];
    if (total) {
      atomicAdd(arcs, total);
    }
  }
}

__global__ void k_activate(
    const u32 *__restrict__ order,
    const u32 *__restrict__ admitted_flags,
    const Prop *__restrict__ props,
    u32 count,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    uint8_t *__restrict__ active,
    uint8_t *__restrict__ unit_active
) {
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 lane = threadIdx.x & (kWave - 1);
  if (wave_id >= count || !admitted_flags[wave_id]) {
    return;
  }
  const u32 u = props[order ? order[wave_id] : wave_id].u;
  const u64 row = xadj[u];
  const u32 deg = static_cast<u32>(xadj[u + 1] - row);
  for (u32 e = lane; e < deg; e += kWave) {
    const u32 v = adjncy[row + e];
    active[v] = 1;
    unit_active[v >> 6] = 1;
  }
}

// Reset the touched per-cluster segment entries (reads the UNSORTED props'
// target fields directly; zeroing per cluster is idempotent).
__global__ void k_reset_segs(
    const Prop *__restrict__ props,
    u32 count,
    u32 *__restrict__ seg_begin,
    u32 *__restrict__ seg_end,
    u32 *__restrict__ prefix_len
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) {
    return;
  }
  const u32 to = props[i].to;
  seg_begin[to] = 0;
  seg_end[to] = 0;
  prefix_len[to] = 0;
}

__global__ void k_dep_reset_all(u32 k_or_n, unsigned long long *__restrict__ dep) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < k_or_n) {
    dep[c] = 0;
  }
}

// Grid-stride with a per-workgroup LDS histogram (one global atomic per
// cluster per WG instead of one per vertex -- same-address global atomics
// serialize at ~11ns).
__global__ void k_sync_labels16(
    u32 n, const u32 *__restrict__ labels, uint16_t *__restrict__ labels16,
    uint8_t *__restrict__ labels8
) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n) {
    const u32 l = labels[u];
    labels16[u] = static_cast<uint16_t>(l);
    labels8[u] = static_cast<uint8_t>(l); // meaningful only for k <= 256
  }
}

__global__ void k_init_weights(
    u32 n,
    u32 k,
    const u32 *__restrict__ labels,
    const i32 *__restrict__ vwgt,
    unsigned long long *__restrict__ weights
) {
  extern __shared__ unsigned long long hist[];
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    hist[c] = 0;
  }
  __syncthreads();
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < n; u += stride) {
    atomicAdd(&hist[labels[u]], static_cast<unsigned long long>(vwgt ? vwgt[u] : 1));
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    if (hist[c]) {
      atomicAdd(&weights[c], hist[c]);
    }
  }
}

// Grid-stride, 16-lane subgroups (4 vertices per wave) so low-degree rows
// keep lanes busy; per-wave partial sums, one atomic per wave.
__global__ void k_edge_cut(
    u32 n,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const u32 *__restrict__ labels,
    unsigned long long *__restrict__ cut
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  u64 local = 0;
  for (u32 base = wave_id * 4; base < n; base += num_waves * 4) {
    const u32 u = base + sub;
    if (u >= n) {
      continue;
    }
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    const u32 lu = labels[u];
    for (u32 e = slot; e < deg; e += 16) {
      if (labels[adjncy[row + e]] != lu) {
        local += adjwgt ? adjwgt[row + e] : 1;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    local += __shfl_down(static_cast<unsigned long long>(local), off, kWave);
  }
  if (lane == 0 && local) {
    atomicAdd(cut, static_cast<unsigned long long>(local));
  }
}

// ==================== commit v2 (refine, k <= 256) ====================
// The round-1 commit issued ~30 launches + 3 rocprim calls + 2-3 host syncs
// per chunk (~85 ms/step control floor). v2 replaces it
// with 4 fixed-shape launches and ZERO host syncs: a stable counting sort
// by target block (k <= 256 distinct keys -- radix sort is overkill), then
// ONE kernel holding the whole admission fixpoint + weight update + label
// apply + active-set maintenance, using a hand-rolled resident-grid barrier
// (all blocks co-resident; hipLaunchCooperativeKernel semantics without the
// API so the launch stays graph-capturable). Admission semantics unchanged:
// per target, proposals are admitted in rank-prefix order under the
// greatest-fixpoint rollback of kaminpar-dist lp_refiner.cc:296-333.

// Refine L-path prep: per-vertex slice counts + exclusive prefix in one
// single-workgroup kernel (replaces k_l_sizes + a rocprim scan over l_cap).
__global__ void k_l_prep_r(
    const u64 *__restrict__ l_list,
    const u32 *__restrict__ l_count,
    const u64 *__restrict__ xadj,
    u32 l_cap,
    u32 slice,
    u32 *__restrict__ l_off
) {
  __shared__ u32 red[17];
  const u32 count = *l_count < l_cap ? *l_count : l_cap;
  const u32 tid = threadIdx.x;
  u32 carry = 0;
  for (u32 base = 0; base < count; base += blockDim.x) {
    const u32 i = base + tid;
    u32 v = 0;
    if (i < count) {
      const u32 u = static_cast<u32>(l_list[i]);
      const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
      v = (deg + slice - 1) / slice;
    }
    u32 inc = v;
    for (int off = 1; off < 64; off <<= 1) {
      const u32 o = __shfl_up(inc, off, kWave);
      if ((tid & 63) >= static_cast<u32>(off)) {
        inc += o;
      }
    }
    __syncthreads();
    if ((tid & 63) == 63) {
      red[tid >> 6] = inc;
    }
    __syncthreads();
    u32 wbase = 0;
    for (u32 w = 0; w < (tid >> 6); ++w) {
      wbase += red[w];
    }
    if (i < count) {
      l_off[i] = carry + wbase + inc - v; // exclusive
    }
    u32 tsum = 0;
    for (u32 w = 0; w < blockDim.x / kWave; ++w) {
      tsum += red[w];
    }
    carry += tsum;
    __syncthreads();
  }
  if (tid == 0) {
    l_off[count] = carry;
  }
}

// Build the M and L work lists for a chunk straight from xadj/active under
// the permutation (no S-kernel involvement): each wave owns a run of
// 64-position tiles; pass 1 counts its M/L entries, ONE reservation atomic
// per wave per list, pass 2 writes the records. List order is wave-row
// order -- irrelevant for determinism since the M/L kernels write
// per-position slots.
__global__ void k_build_lists(
    u32 pos_lo,
    u32 pos_hi, // may be an unaligned sub-range (sharded path)
    u32 n,
    u64 iter_seed,
    u32 rows,
    u32 tpw,
    u32 mid_lo, // kSmallDeg
    u32 mid_hi, // kMidDeg (refine) / kClusterMidDeg (cluster)
    u32 m2_hi,  // kClusterM2Deg (cluster; == mid_hi disables the M2 tier)
    u32 max_degree,
    const u64 *__restrict__ xadj,
    const uint8_t *__restrict__ active,
    const uint8_t *__restrict__ unit_active,
    u64 *__restrict__ m_list,
    u32 *__restrict__ m_count,
    u64 *__restrict__ m2_list,
    u32 *__restrict__ m2_count,
    u64 *__restrict__ l_list,
    u32 *__restrict__ l_count,
    unsigned long long *__restrict__ arcs // null: no tally (legacy path)
) {
  __shared__ unsigned long long arc_red[4];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 ta0 = pos_lo >> 6;                 // absolute unit-tile range
  const u32 T = ((pos_hi + 63) >> 6) - ta0;
  unsigned long long my_arcs = 0;
  const kmp::FeistelPerm fp(kmp::num_units(n), iter_seed);
  const u32 t0 = row * tpw;
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  u32 m_cnt = 0, m2_cnt = 0, l_cnt = 0;
  for (u32 pass = 0; pass < 2; ++pass) {
    u32 m_base = 0, m2_base = 0, l_base = 0;
    if (pass == 1) {
      // flush the arcs tally (one WG-aggregated atomic)
      if (arcs != nullptr) {
        for (int off = 32; off > 0; off >>= 1) {
          my_arcs += __shfl_down(my_arcs, off, kWave);
        }
        __syncthreads();
        if (lane == 0) {
          arc_red[threadIdx.x >> 6] = my_arcs;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          const unsigned long long t2 =
              arc_red[0] + arc_red[1] + arc_red[2] + arc_red[3];
          if (t2) {
            atomicAdd(arcs, t2);
          }
        }
        my_arcs = 0;
      }
      // reserve (lane 0; contention = one atomic per wave-row per list)
      if (lane == 0) {
        if (m_cnt) {
          m_base = atomicAdd(m_count, m_cnt);
        }
        if (m2_cnt) {
          m2_base = atomicAdd(m2_count, m2_cnt);
        }
        if (l_cnt) {
          l_base = atomicAdd(l_count, l_cnt);
        }
      }
      m_base = __shfl(m_base, 0, kWave);
      m2_base = __shfl(m2_base, 0, kWave);
      l_base = __shfl(l_base, 0, kWave);
      if (m_cnt == 0 && m2_cnt == 0 && l_cnt == 0) {
        return;
      }
    }
    for (u32 t = t0; t < t1; ++t) {
      u32 vb = 0;
      if (lane == 0) {
        vb = fp(ta0 + t);
      }
      vb = __shfl(vb, 0, kWave);
      if (!unit_active[vb]) {
        continue;
      }
      const u32 p = ((ta0 + t) << 6) + lane;
      const u32 u = vb * kmp::kUnit + lane;
      bool is_m = false, is_m2 = false, is_l = false;
      if (p >= pos_lo && p < pos_hi && u < n && active[u]) {
        const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
        if (deg <= max_degree) {
          is_m = deg > mid_lo && deg <= mid_hi;
          is_m2 = deg > mid_hi && deg <= m2_hi;
          is_l = deg > m2_hi;
          if (pass == 0 && arcs != nullptr) {
            my_arcs += deg; // arcs-scanned tally (was k_clear_active's job)
          }
        }
      }
      const unsigned long long mm = __ballot(is_m);
      const unsigned long long mm2 = __ballot(is_m2);
      const unsigned long long ll = __ballot(is_l);
      if (pass == 0) {
        m_cnt += __popcll(mm);
        m2_cnt += __popcll(mm2);
        l_cnt += __popcll(ll);
      } else {
        if (is_m) {
          m_list[m_base + __popcll(mm & ((1ull << lane) - 1))] =
              (static_cast<u64>(p) << 32) | u;
        }
        if (is_m2) {
          m2_list[m2_base + __popcll(mm2 & ((1ull << lane) - 1))] =
              (static_cast<u64>(p) << 32) | u;
        }
        if (is_l) {
          l_list[l_base + __popcll(ll & ((1ull << lane) - 1))] =
              (static_cast<u64>(p) << 32) | u;
        }
        m_base += __popcll(mm);
        m2_base += __popcll(mm2);
        l_base += __popcll(ll);
      }
    }
  }
}

// Resident-grid exclusive scan of the k x rows histogram (entries up to
// 262144; a single-workgroup scan is latency-bound at that size) + segment
// offsets, with one grid barrier (coop_bar).
__global__ void k_scan_coop(
    u32 k,
    u32 rows,
    u32 nblk,
    const u32 *__restrict__ histT,
    u32 *__restrict__ offT,
    u32 *__restrict__ seg_off, // k+1
    i64 *__restrict__ blocksums,
    u32 *__restrict__ bar
);

// The commit train's k-sized accumulators (d_dep) are kept in kDepRep
// replicas, workgroup b adding into replica b % kDepRep: ~1000 workgroups
// finishing together onto k = 16 addresses made the same-address atomics the
// tail of the histogram and scatter kernels. Layout: dep[h][r][c], half h = 0
// (departures under full admission) or 1 (see k_scatter_v2).
constexpr u32 kDepRep = 16;

__device__ inline unsigned long long *dep_slot(
    unsigned long long *__restrict__ dep, u32 k, u32 half, u32 c
) {
  return dep + (static_cast<size_t>(half) * kDepRep + blockIdx.x % kDepRep) * k + c;
}

__device__ inline unsigned long long dep_sum(
    const unsigned long long *__restrict__ dep, u32 k, u32 half, u32 c
) {
  unsigned long long s = 0;
#pragma unroll
  for (u32 r = 0; r < kDepRep; ++r) {
    s += dep[(static_cast<size_t>(half) * kDepRep + r) * k + c];
  }
  return s;
}

// The block of the vertex that slot `lane` of unit vb's tile belongs to. The
// v2 train keeps slots in position order and position p holds vertex
// fp(p / 64) * 64 + p % 64, so a valid slot's pr.u is vb * 64 + lane: the
// label can be loaded beside the slot instead of after it. Callers compare
// pr.u and gather again if it ever differs.
__device__ inline u32 unit_label(const uint16_t *__restrict__ labels16, u32 vb, u32 lane, u32 n) {
  const u32 u = vb * kmp::kUnit + lane;
  return u < n ? labels16[u] : 0u;
}

// Per-wave-row histogram of proposal targets over the raw slot array.
// Each wave owns a contiguous run of 64-position tiles (= permutation
// units); fully-inactive units are skipped without reading their (stale)
// slots -- the phase-A kernels freshly write every slot of an ACTIVE unit.
// kUnitW (unit node weights): also counts the proposals by SOURCE block
// (labels16 gather, coalesced within the unit) into dep_full, the
// departures under full admission. With the segment lengths they fix round
// 1 of the admission fixpoint before the scatter runs (round1_cutoff).
// dep_full is zero on entry: k_fixpoint_v2 clears it after reading it.
template <bool kUnitW>
__global__ void k_hist_v2(
    u32 span,
    u32 pos_lo,
    u32 n,
    u64 iter_seed,
    u32 k,
    u32 rows,
    u32 tpw,
    const Prop *__restrict__ slots,
    const uint8_t *__restrict__ unit_active,
    const uint16_t *__restrict__ labels16,
    u32 *__restrict__ histT, // k x rows, column-major by target
    unsigned long long *__restrict__ dep_full // d_dep, half 0 (kUnitW only)
) {
  // dynamic LDS: per-wave cnt (k u32 each); kUnitW: then per-wave source
  // counts (k u32 each)
  extern __shared__ u32 cnt_lds[];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  const u32 waves_per_wg = blockDim.x >> 6;
  u32 *cnt = cnt_lds + wv * k;
  u32 *out = cnt_lds + (waves_per_wg + wv) * k;
  for (u32 c = lane; c < k; c += kWave) {
    cnt[c] = 0;
    if (kUnitW) {
      out[c] = 0;
    }
  }
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 T = span >> 6;
  const kmp::FeistelPerm fp(kmp::num_units(n), iter_seed);
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  for (u32 t = row * tpw; t < t1; ++t) {
    u32 vb = 0;
    if (lane == 0) {
      vb = fp(pos_lo / kmp::kUnit + t);
    }
    vb = __shfl(vb, 0, kWave);
    if (!unit_active[vb]) {
      continue;
    }
    const Prop pr = slots[(t << 6) + lane];
    u32 src = 0;
    if (kUnitW) {
      src = unit_label(labels16, vb, lane, n);
    }
    if (pr.to != kInvalid) {
      atomicAdd(&cnt[pr.to], 1u);
      if (kUnitW) {
        if (pr.u != vb * kmp::kUnit + lane) {
          src = labels16[pr.u];
        }
        atomicAdd(&out[src], 1u);
      }
    }
  }
  for (u32 c = lane; c < k; c += kWave) {
    histT[c * rows + row] = cnt[c];
  }
  if (kUnitW) {
    __syncthreads();
    for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
      u32 s = 0;
      for (u32 w = 0; w < waves_per_wg; ++w) {
        s += cnt_lds[(waves_per_wg + w) * k + c];
      }
      if (s) {
        atomicAdd(dep_slot(dep_full, k, 0, c), static_cast<unsigned long long>(s));
      }
    }
  }
}

// Round 1 of the admission fixpoint for unit node weights, per target c:
// every arrival weighs 1, so the admitted weight of a prefix is its length
// and the round's capacity needs only the departures under full admission.
// Exactly the first trip of the loop in k_fixpoint_v2.
__device__ inline u32 round1_cutoff(i64 maxw, i64 weight, unsigned long long dep_full, u32 len) {
  const i64 cap = maxw - weight + static_cast<i64>(dep_full);
  return cap <= 0 ? 0u : (cap >= static_cast<i64>(len) ? len : static_cast<u32>(cap));
}

// Stable scatter into target-sorted order. Each wave replays its tile run
// in position order; within a 64-slot tile, stable per-target ranks come
// from a 64-step shuffle waterfall (no LDS read-after-write ordering
// assumptions: the leader's base is broadcast by shuffle). Also freezes the
// source block of every proposal (labels16 gather, coalesced within the
// unit) so the fixpoint never gathers labels again.
//
// kUnitW (unit node weights) applies round 1 of the admission fixpoint on
// the way: an entry whose rank in its target segment is at or past the
// round-1 cutoff can never be admitted (admission only shrinks), so it is
// neither written nor counted, and dep half 1 receives the departures AFTER
// round 1 (half 0 holds k_hist_v2's full-admission departures). The
// admitted prefix of every segment is written exactly as before. s_w is not
// written: nothing reads it for unit weights.
template <bool kUnitW>
__global__ void k_scatter_v2(
    u32 span,
    u32 pos_lo,
    u32 n,
    u64 iter_seed,
    u32 k,
    u32 rows,
    u32 tpw,
    const Prop *__restrict__ slots,
    const uint8_t *__restrict__ unit_active,
    const u32 *__restrict__ offT,
    const uint16_t *__restrict__ labels16,
    const u32 *__restrict__ seg_off,  // k+1 (kUnitW)
    const i64 *__restrict__ weights,  // k (kUnitW)
    const i64 *__restrict__ maxw,     // k (kUnitW)
    u32 *__restrict__ s_u,
    u32 *__restrict__ s_w,
    uint16_t *__restrict__ s_to,
    uint16_t *__restrict__ s_b,
    // d_dep (kDepRep replicas per half). Weighted: half 0 departures, half 1
    // arrivals under full admission; kUnitW: half 0 read (k_hist_v2), half 1
    // departures after round 1
    unsigned long long *__restrict__ dep
) {
  // dynamic LDS: per-wave cnt (k u32 each); then, weighted: one per-WG pair
  // of u64 hists, full-admission departure weights by source block and
  // incoming weights by target (the fixpoint kernel starts from these
  // totals); kUnitW: the segment starts and round-1 cutoffs (k u32 each) and
  // per-wave departure counts (k u32 each).
  extern __shared__ u32 cnt_lds[];
  const u32 waves_per_wg = blockDim.x >> 6;
  unsigned long long *h_out =
      reinterpret_cast<unsigned long long *>(cnt_lds + waves_per_wg * k);
  unsigned long long *h_in = h_out + k;
  u32 *soff = cnt_lds + waves_per_wg * k;
  u32 *nl1 = soff + k;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  u32 *cnt = cnt_lds + wv * k;
  u32 *out1 = nl1 + k + wv * k;
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  for (u32 c = lane; c < k; c += kWave) {
    cnt[c] = offT[c * rows + row];
    if (kUnitW) {
      out1[c] = 0;
    }
  }
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    if (kUnitW) {
      const u32 b = seg_off[c];
      soff[c] = b;
      nl1[c] = round1_cutoff(maxw[c], weights[c], dep_sum(dep, k, 0, c), seg_off[c + 1] - b);
    } else {
      h_out[c] = 0;
      h_in[c] = 0;
    }
  }
  __syncthreads();
  const u32 T = span >> 6;
  const kmp::FeistelPerm fp(kmp::num_units(n), iter_seed);
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  for (u32 t = row * tpw; t < t1; ++t) {
    u32 vb = 0;
    if (lane == 0) {
      vb = fp(pos_lo / kmp::kUnit + t);
    }
    vb = __shfl(vb, 0, kWave);
    if (!unit_active[vb]) {
      continue;
    }
    const Prop pr = slots[(t << 6) + lane];
    u32 lab = unit_label(labels16, vb, lane, n);
    const u32 c = pr.to;
    const bool valid = c != kInvalid;
    if (valid && pr.u != vb * kmp::kUnit + lane) {
      lab = labels16[pr.u];
    }
    u32 rank = 0, total = 0, leader = 0;
    bool seen = false;
    for (u32 j = 0; j < kWave; ++j) {
      const u32 cj = __shfl(c, j, kWave);
      if (valid && cj == c) {
        ++total;
        if (j < lane) {
          ++rank;
        }
        if (!seen) {
          leader = j;
          seen = true;
        }
      }
    }
    u32 base0 = 0;
    if (valid && rank == 0) {
      base0 = cnt[c];
      cnt[c] = base0 + total;
    }
    const u32 base = __shfl(base0, leader, kWave);
    if (kUnitW) {
      const u32 dst = base + rank;
      if (valid && dst - soff[c] < nl1[c]) {
        const uint16_t src = static_cast<uint16_t>(lab);
        s_u[dst] = pr.u;
        s_to[dst] = static_cast<uint16_t>(c);
        s_b[dst] = src;
        atomicAdd(&out1[src], 1u);
      }
    } else if (valid) {
      const u32 dst = base + rank;
      const uint16_t src = static_cast<uint16_t>(lab);
      s_u[dst] = pr.u;
      s_w[dst] = pr.w;
      s_to[dst] = static_cast<uint16_t>(c);
      s_b[dst] = src;
      atomicAdd(&h_out[src], static_cast<unsigned long long>(pr.w));
      atomicAdd(&h_in[c], static_cast<unsigned long long>(pr.w));
    }
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    if (kUnitW) {
      u32 s = 0;
      for (u32 w = 0; w < waves_per_wg; ++w) {
        s += nl1[k + w * k + c];
      }
      if (s) {
        atomicAdd(dep_slot(dep, k, 1, c), static_cast<unsigned long long>(s));
      }
    } else {
      if (h_out[c]) {
        atomicAdd(dep_slot(dep, k, 0, c), h_out[c]);
      }
      if (h_in[c]) {
        atomicAdd(dep_slot(dep, k, 1, c), h_in[c]);
      }
    }
  }
}

// ==================== degree-bucket rearrangement (on-GPU) ====================
// The reference's default NodeOrdering::DEGREE_BUCKETS preprocessing
// (graphutils/permutator.cc:36-110): stable counting sort of vertices into
// 33 log2-degree buckets (deg-0 last) + CSR re-gather with neighbour
// relabeling. Device-resident so the drop-in path needs no host pass
// (bit-identical to the host kmp_rearrange_degree_buckets).
constexpr u32 kDbBuckets = 33;

__device__ inline u32 db_bucket_of(u32 deg) {
  return deg == 0 ? kDbBuckets - 1 : (31 - __clz(deg) + 1);
}

__global__ void k_db_hist(
    u32 n,
    u32 rows,
    u32 tpw,
    const u64 *__restrict__ xadj,
    u32 *__restrict__ histT // kDbBuckets x rows
) {
  __shared__ u32 cnt_lds[4 * kDbBuckets];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  u32 *cnt = cnt_lds + wv * kDbBuckets;
  for (u32 b = lane; b < kDbBuckets; b += kWave) {
    cnt[b] = 0;
  }
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 T = (n + 63) >> 6;
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  for (u32 t = row * tpw; t < t1; ++t) {
    const u32 u = (t << 6) + lane;
    if (u < n) {
      atomicAdd(&cnt[db_bucket_of(static_cast<u32>(xadj[u + 1] - xadj[u]))], 1u);
    }
  }
  for (u32 b = lane; b < kDbBuckets; b += kWave) {
    histT[b * rows + row] = cnt[b];
  }
}

__global__ void k_db_scatter(
    u32 n,
    u32 rows,
    u32 tpw,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ offT,
    u32 *__restrict__ perm, // perm[u_old] = u_new
    u32 *__restrict__ inv   // inv[u_new] = u_old
) {
  __shared__ u32 cnt_lds[4 * kDbBuckets];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  u32 *cnt = cnt_lds + wv * kDbBuckets;
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  for (u32 b = lane; b < kDbBuckets; b += kWave) {
    cnt[b] = offT[b * rows + row];
  }
  const u32 T = (n + 63) >> 6;
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  for (u32 t = row * tpw; t < t1; ++t) {
    const u32 u = (t << 6) + lane;
    const bool valid = u < n;
    const u32 b = valid ? db_bucket_of(static_cast<u32>(xadj[u + 1] - xadj[u]))
                        : 0xFFFFFFFFu;
    u32 rank = 0, total = 0, leader = 0;
    bool seen = false;
    for (u32 j = 0; j < kWave; ++j) {
      const u32 bj = __shfl(b, j, kWave);
      if (valid && bj == b) {
        ++total;
        if (j < lane) {
          ++rank;
        }
        if (!seen) {
          leader = j;
          seen = true;
        }
      }
    }
    u32 base0 = 0;
    if (valid && rank == 0) {
      base0 = cnt[b];
      cnt[b] = base0 + total;
    }
    const u32 base = __shfl(base0, leader, kWave);
    if (valid) {
      const u32 pos = base + rank;
      perm[u] = pos;
      inv[pos] = u;
    }
  }
}

__global__ void k_db_degrees(
    u32 n,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ inv,
    u64 *__restrict__ new_deg // n+1 entries ([0] = 0 written by host memset)
) {
  const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) {
    const u32 u = inv[v];
    new_deg[v + 1] = xadj[u + 1] - xadj[u];
  }
}

// 16-lane subgroups, 4 vertices/wave: copy each new row from its old
// position, relabeling neighbours through perm.
__global__ void k_db_gather(
    u32 n,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const i32 *__restrict__ vwgt,
    const u32 *__restrict__ perm,
    const u32 *__restrict__ inv,
    const u64 *__restrict__ new_xadj,
    u32 *__restrict__ new_adjncy,
    i32 *__restrict__ new_adjwgt,
    i32 *__restrict__ new_vwgt
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  for (u32 base = wave_id * 4; base < n; base += num_waves * 4) {
    const u32 v = base + sub;
    if (v >= n) {
      continue;
    }
    const u32 u = inv[v];
    const u64 src = xadj[u];
    const u64 dst = new_xadj[v];
    const u32 deg = static_cast<u32>(xadj[u + 1] - src);
    for (u32 i = slot; i < deg; i += 16) {
      new_adjncy[dst + i] = perm[adjncy[src + i]];
      if (adjwgt != nullptr) {
        new_adjwgt[dst + i] = adjwgt[src + i];
      }
    }
    if (slot == 0 && vwgt != nullptr) {
      new_vwgt[v] = vwgt[u];
    }
  }
}

// ==================== sharded commit (multi-GPU) ====================
// Rank-sharded deterministic admission over the ALL-GATHERED proposal list
// (dense Prop records in global rank order): each rank sorts and fixpoints
// only its own target range [c_lo, c_hi); the k-sized de-admission delta is
// allreduced per round (exactly the block-weight reconciliation of
// kaminpar-dist/refinement/lp/lp_refiner.cc:296-333) and the final
// per-target rank-cutoffs are exchanged so every rank applies the identical
// admitted set. Bit-identical to the single-GPU commit: the per-round
// global departure sums match the monolithic fixpoint's rounds.

// Histogram over the dense proposal list, filtered to the rank's targets.
__global__ void k_hist_props(
    const u32 *__restrict__ count_dev,
    u32 k,
    u32 rows,
    u32 tpw,
    u32 c_lo,
    u32 c_hi,
    const Prop *__restrict__ props,
    u32 *__restrict__ histT
) {
  extern __shared__ u32 cnt_lds[];
  const u32 count = *count_dev;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  u32 *cnt = cnt_lds + wv * k;
  for (u32 c = lane; c < k; c += kWave) {
    cnt[c] = 0;
  }
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 T = (count + 63) >> 6;
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  for (u32 t = row * tpw; t < t1; ++t) {
    const u32 i = (t << 6) + lane;
    if (i < count) {
      const u32 to = props[i].to;
      if (to >= c_lo && to < c_hi) {
        atomicAdd(&cnt[to], 1u);
      }
    }
  }
  for (u32 c = lane; c < k; c += kWave) {
    histT[c * rows + row] = cnt[c];
  }
}

// Stable scatter of the rank's targets + full-admission dep/arr totals:
// dep contributions (by SOURCE block, over the rank's own-target proposals)
// go to the caller's allreduce buffer; arrival totals stay local.
__global__ void k_scatter_props(
    const u32 *__restrict__ count_dev,
    u32 k,
    u32 rows,
    u32 tpw,
    u32 c_lo,
    u32 c_hi,
    const Prop *__restrict__ props,
    const u32 *__restrict__ offT,
    const u32 *__restrict__ labels,
    u32 *__restrict__ s_u,
    u32 *__restrict__ s_w,
    u32 *__restrict__ s_r,
    uint16_t *__restrict__ s_to,
    uint16_t *__restrict__ s_b,
    long long *__restrict__ dep_out,          // k+1 (caller buffer, zeroed)
    unsigned long long *__restrict__ arr_loc  // e->d_dep + k
) {
  extern __shared__ u32 cnt_lds[];
  const u32 waves_per_wg = blockDim.x >> 6;
  unsigned long long *h_out =
      reinterpret_cast<unsigned long long *>(cnt_lds + waves_per_wg * k);
  unsigned long long *h_in = h_out + k;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  u32 *cnt = cnt_lds + wv * k;
  const u32 row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  for (u32 c = lane; c < k; c += kWave) {
    cnt[c] = offT[c * rows + row];
  }
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    h_out[c] = 0;
    h_in[c] = 0;
  }
  __syncthreads();
  const u32 count = *count_dev;
  const u32 T = (count + 63) >> 6;
  const u32 t1 = (row + 1) * tpw < T ? (row + 1) * tpw : T;
  for (u32 t = row * tpw; t < t1; ++t) {
    const u32 i = (t << 6) + lane;
    Prop pr{0u, kInvalid, 0u, 0u};
    if (i < count) {
      pr = props[i];
    }
    const u32 c = pr.to;
    const bool valid = c != kInvalid && c >= c_lo && c < c_hi;
    u32 rank = 0, total = 0, leader = 0;
    bool seen = false;
    for (u32 j = 0; j < kWave; ++j) {
      const u32 cj = __shfl(c, j, kWave);
      const int vj = __shfl(static_cast<int>(valid), j, kWave);
      if (valid && vj && cj == c) {
        ++total;
        if (j < lane) {
          ++rank;
        }
        if (!seen) {
          leader = j;
          seen = true;
        }
      }
    }
    u32 base0 = 0;
    if (valid && rank == 0) {
      base0 = cnt[c];
      cnt[c] = base0 + total;
    }
    const u32 base = __shfl(base0, leader, kWave);
    if (valid) {
      const u32 dst = base + rank;
      const uint16_t srcb = static_cast<uint16_t>(labels[pr.u]);
      s_u[dst] = pr.u;
      s_w[dst] = pr.w;
      s_r[dst] = pr.rank;
      s_to[dst] = static_cast<uint16_t>(c);
      s_b[dst] = srcb;
      atomicAdd(&h_out[srcb], static_cast<unsigned long long>(pr.w));
      atomicAdd(&h_in[c], static_cast<unsigned long long>(pr.w));
    }
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    if (h_out[c]) {
      atomicAdd(reinterpret_cast<unsigned long long *>(&dep_out[c]), h_out[c]);
    }
    if (h_in[c]) {
      atomicAdd(&arr_loc[c], h_in[c]);
    }
  }
}

// Copy the device proposal count into the send buffer's trailing row so a
// single fixed-size allgather moves payload + counts with no host sync.
__global__ void k_set_u32(u32 *__restrict__ dst, u32 v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *dst = v;
  }
}

__global__ void k_pack_count(const u32 *__restrict__ count_dev, Prop *__restrict__ trailing) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    trailing->u = *count_dev;
  }
}

// Dense-pack the gathered per-rank segments (cap+1 rows each, trailing row
// carries the rank's count) into e->d_props, in rank order (= global rank
// order since rank position slices ascend); writes the total count.
__global__ void k_compact_gathered(
    u32 world,
    u32 cap,
    const Prop *__restrict__ recv, // world * (cap+1) rows
    Prop *__restrict__ dense,
    u32 *__restrict__ total_out
) {
  __shared__ u32 cnt_s[8], off_s[9];
  const u32 tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (threadIdx.x < world) {
    cnt_s[threadIdx.x] = recv[(static_cast<size_t>(threadIdx.x) * (cap + 1) + cap)].u;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 acc = 0;
    for (u32 r = 0; r < world; ++r) {
      off_s[r] = acc;
      acc += cnt_s[r];
    }
    off_s[world] = acc;
    if (blockIdx.x == 0) {
      *total_out = acc;
    }
  }
  __syncthreads();
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 r = 0; r < world; ++r) {
    const u32 n_r = cnt_s[r];
    const Prop *src_r = recv + static_cast<size_t>(r) * (cap + 1);
    Prop *dst_r = dense + off_s[r];
    for (u32 i = tid; i < n_r; i += stride) {
      dst_r[i] = src_r[i];
    }
  }
}

__global__ void k_vec_sub_i64(u32 n, long long *__restrict__ a, const long long *__restrict__ b) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    a[i] -= b[i];
  }
}

// Activation over the dense proposal list with a device count (wave per
// admitted entry; the C++ dist driver's analogue of k_activate).
__global__ void k_activate_props_dev(
    const u32 *__restrict__ count_dev,
    const u32 *__restrict__ admitted_flags,
    const Prop *__restrict__ props,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    uint8_t *__restrict__ active,
    uint8_t *__restrict__ unit_active
) {
  const u32 count = *count_dev;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 waves = (gridDim.x * blockDim.x) >> 6;
  const u32 lane = threadIdx.x & (kWave - 1);
  for (u32 i = wave_id; i < count; i += waves) {
    if (!admitted_flags[i]) {
      continue;
    }
    const u32 u = props[i].u;
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    for (u32 e2 = lane; e2 < deg; e2 += kWave) {
      const u32 v = adjncy[row + e2];
      active[v] = 1;
      unit_active[v >> 6] = 1;
    }
  }
}

// Segmented prefix weights for the rank's targets (weighted graphs only;
// wave per segment, tile scans).
__global__ void k_shard_pw(
    u32 k,
    u32 c_lo,
    u32 c_hi,
    const u32 *__restrict__ seg_off,
    const u32 *__restrict__ prefix_len,
    const u32 *__restrict__ s_w,
    i64 *__restrict__ pw
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 waves = (gridDim.x * blockDim.x) >> 6;
  for (u32 c = c_lo + wv; c < c_hi; c += waves) {
    const u32 b = seg_off[c];
    const u32 len = prefix_len[c];
    i64 carry = 0;
    for (u32 base = 0; base < len; base += kWave) {
      const u32 i = base + lane;
      i64 v = (i < len) ? static_cast<i64>(s_w[b + i]) : 0;
      i64 inc = v;
      for (int off = 1; off < 64; off <<= 1) {
        const i64 o = __shfl_up(inc, off, kWave);
        if (lane >= static_cast<u32>(off)) {
          inc += o;
        }
      }
      if (i < len) {
        pw[b + i] = carry + inc;
      }
      carry += __shfl(inc, kWave - 1, kWave);
    }
  }
}

// One synchronous fixpoint round over the rank's targets: capacities frozen
// from the GLOBAL departure vector, de-admissions accumulated into the
// caller's delta buffer ([k] = changed flag). plen/arr persist in
// d_prefix_len / d_dep[k..2k).
__global__ void k_shard_round(
    u32 k,
    u32 c_lo,
    u32 c_hi,
    u32 has_vwgt,
    const u32 *__restrict__ seg_off,
    u32 *__restrict__ prefix_len,
    unsigned long long *__restrict__ arr_loc, // d_dep + k (live)
    const long long *__restrict__ dep_global, // k (allreduced)
    const u32 *__restrict__ s_w,
    const uint16_t *__restrict__ s_b,
    const i64 *__restrict__ pw, // segmented prefix weights (weighted only)
    const i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    long long *__restrict__ delta_out // k+1 (caller buffer, zeroed here)
) {
  __shared__ unsigned long long ddelta[256];
  __shared__ u32 rlo_s[256], rhi_s[256];
  __shared__ int chg;
  const u32 tid = threadIdx.x;
  if (tid < k) {
    ddelta[tid] = 0;
  }
  if (tid == 0) {
    chg = 0;
  }
  __syncthreads();
  if (tid < k) {
    const u32 c = tid;
    u32 nlo = 0, nhi = 0;
    if (c >= c_lo && c < c_hi && prefix_len[c] > 0) {
      const i64 cap = maxw[c] - weights[c] + static_cast<i64>(dep_global[c]);
      const long long a = static_cast<long long>(arr_loc[c]);
      if (a > cap) {
        const u32 old = prefix_len[c];
        const u32 b = seg_off[c];
        u32 nl;
        if (!has_vwgt) {
          nl = cap <= 0 ? 0u : (cap >= static_cast<i64>(old) ? old : static_cast<u32>(cap));
          arr_loc[c] = nl;
        } else {
          u32 lo2 = 0, hi2 = old;
          while (lo2 < hi2) {
            const u32 mid = (lo2 + hi2 + 1) >> 1;
            if (pw[b + mid - 1] <= cap) {
              lo2 = mid;
            } else {
              hi2 = mid - 1;
            }
          }
          nl = lo2;
          arr_loc[c] = nl ? static_cast<unsigned long long>(pw[b + nl - 1]) : 0ull;
        }
        if (nl < old) {
          prefix_len[c] = nl;
          nlo = b + nl;
          nhi = b + old;
          chg = 1;
        }
      }
    }
    rlo_s[c] = nlo;
    rhi_s[c] = nhi;
  }
  __syncthreads();
  for (u32 c = 0; c < k; ++c) {
    const u32 lo2 = rlo_s[c], hi2 = rhi_s[c];
    for (u32 i = lo2 + tid; i < hi2; i += blockDim.x) {
      atomicAdd(&ddelta[s_b[i]], has_vwgt ? static_cast<unsigned long long>(s_w[i]) : 1ull);
    }
  }
  __syncthreads();
  if (tid < k) {
    delta_out[tid] = static_cast<long long>(ddelta[tid]);
  }
  if (tid == 0) {
    delta_out[k] = chg;
  }
}

// Export the rank's final per-target cutoff ranks + admitted arrival
// weights into caller buffers (zero elsewhere; an allreduce-sum doubles as
// the allgather).
__global__ void k_shard_finish_meta(
    u32 k,
    u32 c_lo,
    u32 c_hi,
    const u32 *__restrict__ seg_off,
    const u32 *__restrict__ prefix_len,
    const unsigned long long *__restrict__ arr_loc,
    const u32 *__restrict__ s_r,
    unsigned long long *__restrict__ cutoff_out, // k i64 (zeroed by caller)
    long long *__restrict__ arr_out              // k i64 (zeroed by caller)
) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < c_lo || c >= c_hi) {
    return;
  }
  const u32 len = prefix_len[c];
  const u32 seg_len = seg_off[c + 1] - seg_off[c];
  // cutoff = rank of the first NON-admitted proposal (all ranks below it
  // are admitted: the sorted order is rank order within the target); i64
  // cells so a plain allreduce-sum doubles as the allgather
  cutoff_out[c] = (len >= seg_len) ? ~0ull : s_r[seg_off[c] + len];
  arr_out[c] = static_cast<long long>(arr_loc[c]);
}

// Apply the globally-agreed admission on the full proposal list + update
// all block weights; every rank executes this identically.
__global__ void k_shard_apply(
    const u32 *__restrict__ count_dev,
    u32 k,
    const Prop *__restrict__ props,
    const unsigned long long *__restrict__ cutoff_all, // k (allreduced)
    const long long *__restrict__ arr_all,   // k (allreduced)
    const long long *__restrict__ dep_global, // k (final)
    i64 *__restrict__ weights,
    u32 *__restrict__ labels,
    uint16_t *__restrict__ labels16,
    uint8_t *__restrict__ labels8, // null unless k <= 256
    u32 *__restrict__ admitted_flags,
    unsigned long long *__restrict__ moves
) {
  const u32 count = *count_dev;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) {
    const i64 delta = static_cast<i64>(arr_all[i]) - static_cast<i64>(dep_global[i]);
    if (delta) {
      weights[i] += delta;
    }
  }
  unsigned long long local = 0;
  if (i < count) {
    const Prop pr = props[i];
    const bool adm = pr.rank < cutoff_all[pr.to];
    admitted_flags[i] = adm ? 1u : 0u;
    if (adm) {
      labels[pr.u] = pr.to;
      labels16[pr.u] = static_cast<uint16_t>(pr.to);
      if (labels8 != nullptr) {
        labels8[pr.u] = static_cast<uint8_t>(pr.to);
      }
      local = 1;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    local += __shfl_down(static_cast<unsigned long long>(local), off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && local) {
    atomicAdd(moves, local);
  }
}

// Resident-grid barrier: flat arrival counter + generation release, relaxed
// agent-scope atomics bracketed by __threadfence (measured the fastest
// variant on gfx950: ~3 us at 64 blocks vs ~20 us for acq_rel two-level --
// tools/bar_bench.hip). Requires every block co-resident (grid sized from
// occupancy, capped small since the commit stages are latency- not
// bandwidth-bound).
__device__ inline void coop_bar(u32 *bar, u32 nblk) {
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 *root = bar + 8;
    u32 *gen = bar + 9;
    __threadfence(); // publish this block's writes before arrival
    const u32 g = __hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_fetch_add(root, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
        nblk - 1) {
      __hip_atomic_store(root, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(gen, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      // deadman: if residency was ever violated this spin would hang the
      // device -- trap instead so the failure is a visible abort
      u32 spins = 0;
      while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > 400000000u) {
          __builtin_trap();
        }
      }
    }
    __threadfence(); // see every other block's published writes
  }
  __syncthreads();
}

// One grid barrier: every workgroup scans its range [lo, hi) and keeps the
// local exclusive values in registers (kScanPer per thread; a range of
// 4096 entries at 64 workgroups and the largest table), publishes its total,
// and after the barrier every wave sums the totals of the workgroups before
// its own with one reduction, so offT is written once. A range too long for
// the registers (fewer resident workgroups) parks the local values in offT
// and adds the carry in a second pass. Segment starts are written by the
// workgroup that owns entry c * rows. Launch with 256 threads.
constexpr u32 kScanPer = 16;

__global__ void k_scan_coop(
    u32 k,
    u32 rows,
    u32 nblk,
    const u32 *__restrict__ histT,
    u32 *__restrict__ offT,
    u32 *__restrict__ seg_off,
    i64 *__restrict__ blocksums,
    u32 *__restrict__ bar
) {
  constexpr u32 kWaves = 4; // kScanPer * kWaves wave totals = one wave scan
  static_assert(kScanPer * kWaves == kWave, "wave totals are scanned by one wave");
  __shared__ u32 red[kScanPer * kWaves + 1];
  const u32 tid = threadIdx.x;
  const u32 lane = tid & (kWave - 1);
  const u32 wv = tid >> 6;
  const u32 entries = k * rows;
  const u32 rlen = (entries + nblk - 1) / nblk;
  const u32 lo = blockIdx.x * rlen < entries ? blockIdx.x * rlen : entries;
  const u32 hi = lo + rlen < entries ? lo + rlen : entries;
  const u32 tile = kScanPer * kWaves * kWave;
  const bool in_regs = rlen <= tile;

  u32 loc[kScanPer];
  u32 carry = 0;
  for (u32 t0 = lo; t0 < hi; t0 += tile) {
    u32 v[kScanPer];
#pragma unroll
    for (u32 j = 0; j < kScanPer; ++j) {
      const u32 i = t0 + j * (kWaves * kWave) + tid;
      v[j] = i < hi ? histT[i] : 0;
    }
#pragma unroll
    for (u32 j = 0; j < kScanPer; ++j) {
      u32 inc = v[j];
      for (int off = 1; off < 64; off <<= 1) {
        const u32 o = __shfl_up(inc, off, kWave);
        if (lane >= static_cast<u32>(off)) {
          inc += o;
        }
      }
      loc[j] = inc - v[j]; // exclusive within the wave
      if (lane == kWave - 1) {
        red[j * kWaves + wv] = inc;
      }
    }
    __syncthreads();
    if (wv == 0) {
      // exclusive scan of the 64 wave totals, in entry order
      const u32 x = red[lane];
      u32 inc = x;
      for (int off = 1; off < 64; off <<= 1) {
        const u32 o = __shfl_up(inc, off, kWave);
        if (lane >= static_cast<u32>(off)) {
          inc += o;
        }
      }
      red[lane] = inc - x;
      if (lane == kWave - 1) {
        red[kScanPer * kWaves] = inc;
      }
    }
    __syncthreads();
#pragma unroll
    for (u32 j = 0; j < kScanPer; ++j) {
      loc[j] += carry + red[j * kWaves + wv];
      if (!in_regs) {
        const u32 i = t0 + j * (kWaves * kWave) + tid;
        if (i < hi) {
          offT[i] = loc[j];
        }
      }
    }
    carry += red[kScanPer * kWaves];
    __syncthreads();
  }
  if (tid == 0) {
    blocksums[blockIdx.x] = static_cast<i64>(carry);
  }
  coop_bar(bar, nblk);
  // totals before this workgroup, and the grand total
  u32 before = 0, all = 0;
  for (u32 b = lane; b < nblk; b += kWave) {
    const u32 s = static_cast<u32>(
        __hip_atomic_load(&blocksums[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
    );
    all += s;
    before += b < blockIdx.x ? s : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    before += __shfl_xor(before, off, kWave);
    all += __shfl_xor(all, off, kWave);
  }
  if (in_regs) {
#pragma unroll
    for (u32 j = 0; j < kScanPer; ++j) {
      const u32 i = lo + j * (kWaves * kWave) + tid;
      if (i < hi) {
        offT[i] = loc[j] + before;
      }
    }
  } else if (before) {
    for (u32 i = lo + tid; i < hi; i += blockDim.x) {
      offT[i] += before;
    }
  }
  __syncthreads();
  for (u32 c = (lo + rows - 1) / rows + tid; c < k && c * rows < hi; c += blockDim.x) {
    seg_off[c] = offT[c * rows];
  }
  if (blockIdx.x == 0 && tid == 0) {
    seg_off[k] = all;
  }
}

// The admission fixpoint in ONE single-workgroup launch (no grid
// barriers, trivially stream-ordered). Walks each target's rank-cutoff
// BACKWARD per round under capacities frozen at round start -- exactly the
// synchronous rollback rounds of kaminpar-dist lp_refiner.cc:296-333, with
// O(de-admitted) work per round instead of a full rescan. Bit-identical to
// the legacy commit (same per-round cutoffs, greatest fixpoint).
//
// kVw (node weights): starts from the full-admission state the scatter
// kernel accumulated (dep half 0 = departures by source block, half 1 =
// incoming weight by target; see dep_slot). Unit weights: round 1 ran on the
// full grid (k_hist_v2 + k_scatter_v2), so the walk starts from the round-1
// cutoffs with half 1 = departures after round 1, and its first trip is round 2;
// if round 1 truncated nothing that trip finds every target within its
// capacity and exits. Thread c keeps target c's state in registers; weights
// and maxw do not change until the epilogue. Both halves of dep are read
// once and cleared for the next chunk.
template <bool kVw>
__global__ void k_fixpoint_v2(
    u32 k,
    const u32 *__restrict__ seg_off,
    u32 *__restrict__ prefix_len,
    unsigned long long *__restrict__ dep,
    const u32 *__restrict__ s_w,
    const uint16_t *__restrict__ s_b,
    i64 *__restrict__ weights,
    const i64 *__restrict__ maxw,
    unsigned long long *__restrict__ moves,
    i64 *__restrict__ pw // scratch: segmented prefix weights (weighted only)
) {
  // unit weights: a round de-admits fewer than 2^32 entries
  using Delta = typename std::conditional<kVw, unsigned long long, u32>::type;
  __shared__ Delta ddelta[256];          // this round's de-admissions
  __shared__ u32 rlo_s[256], rhi_s[256]; // this round's de-admitted ranges
  __shared__ unsigned long long red[4];
  __shared__ int chg;
  const u32 tid = threadIdx.x;
  i64 w = 0, mx = 0;
  i64 ddep = 0; // current departures
  i64 arr = 0;  // admitted incoming weight
  u32 plen = 0, soff = 0;
  if (tid < k) {
    w = weights[tid];
    mx = maxw[tid];
    soff = seg_off[tid];
    const u32 len = seg_off[tid + 1] - soff;
    const unsigned long long d0 = dep_sum(dep, k, 0, tid), d1 = dep_sum(dep, k, 1, tid);
#pragma unroll
    for (u32 r = 0; r < 2 * kDepRep; ++r) {
      dep[static_cast<size_t>(r) * k + tid] = 0;
    }
    if (kVw) {
      ddep = static_cast<i64>(d0);
      arr = static_cast<i64>(d1);
      plen = len;
    } else {
      plen = round1_cutoff(mx, w, d0, len);
      arr = static_cast<i64>(plen);
      ddep = static_cast<i64>(d1);
    }
    ddelta[tid] = 0;
    rlo_s[tid] = 0;
    rhi_s[tid] = 0;
  }
  if (kVw) {
    // build segmented prefix weights once (wave per target, tile scans) so
    // per-round cutoffs are binary searches instead of serial walks
    const u32 lane = tid & (kWave - 1);
    const u32 wv = tid >> 6;
    for (u32 c = wv; c < k; c += blockDim.x / kWave) {
      const u32 b = seg_off[c];
      const u32 len = seg_off[c + 1] - b;
      i64 carry = 0;
      for (u32 base = 0; base < len; base += kWave) {
        const u32 i = base + lane;
        i64 v = (i < len) ? static_cast<i64>(s_w[b + i]) : 0;
        i64 inc = v;
        for (int off = 1; off < 64; off <<= 1) {
          const i64 o = __shfl_up(inc, off, kWave);
          if (lane >= static_cast<u32>(off)) {
            inc += o;
          }
        }
        if (i < len) {
          pw[b + i] = carry + inc;
        }
        carry += __shfl(inc, kWave - 1, kWave);
      }
    }
  }
  __syncthreads();
  for (;;) {
    if (tid == 0) {
      chg = 0;
    }
    // capacity frozen at round start (synchronous rounds)
    const i64 cap = mx - w + ddep;
    __syncthreads();
    if (tid < k && plen > 0 && arr > cap) {
      const u32 old = plen;
      u32 nl;
      if (!kVw) {
        // unit weights: admitted weight of a prefix IS its length
        nl = cap <= 0 ? 0u : (cap >= static_cast<i64>(old) ? old : static_cast<u32>(cap));
        arr = static_cast<i64>(nl);
      } else {
        // weighted: binary search the segmented prefix weights
        u32 lo2 = 0, hi2 = old;
        while (lo2 < hi2) {
          const u32 mid = (lo2 + hi2 + 1) >> 1;
          if (pw[soff + mid - 1] <= cap) {
            lo2 = mid;
          } else {
            hi2 = mid - 1;
          }
        }
        nl = lo2;
        arr = nl ? pw[soff + nl - 1] : 0;
      }
      plen = nl;
      rlo_s[tid] = soff + nl;
      rhi_s[tid] = soff + old;
      chg = 1; // benign same-value race
    }
    __syncthreads();
    if (!chg) {
      break;
    }
    // block-parallel de-admission deltas (coalesced; O(total de-admitted))
    for (u32 c = 0; c < k; ++c) {
      const u32 lo2 = rlo_s[c], hi2 = rhi_s[c];
      for (u32 i = lo2 + tid; i < hi2; i += blockDim.x) {
        atomicAdd(&ddelta[s_b[i]], kVw ? static_cast<Delta>(s_w[i]) : static_cast<Delta>(1));
      }
    }
    __syncthreads();
    if (tid < k) {
      if (ddelta[tid]) {
        ddep -= static_cast<i64>(ddelta[tid]);
        ddelta[tid] = 0;
      }
      rlo_s[tid] = 0;
      rhi_s[tid] = 0;
    }
    __syncthreads();
  }

  // weights + writeback + move count
  unsigned long long mv = 0;
  if (tid < k) {
    const i64 delta = arr - ddep;
    if (delta) {
      weights[tid] = w + delta;
    }
    prefix_len[tid] = plen;
    mv = plen;
  }
  for (int off = 32; off > 0; off >>= 1) {
    mv += __shfl_down(mv, off, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    red[tid >> 6] = mv;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (u32 w2 = 0; w2 < blockDim.x / kWave; ++w2) {
      t += red[w2];
    }
    if (t) {
      atomicAdd(moves, t);
    }
  }
}

// Single-workgroup variant of the histogram scan for small chunks (entries
// <= a few thousand; the resident-grid version's barriers dominate there).
// kInit: also the fixpoint init of the sharded commit (prefix_len = segment
// lengths, dep and changed cleared). The v2 train takes offsets only: its
// consumers derive the lengths from seg_off and k_fixpoint_v2 clears dep.
template <bool kInit>
__global__ void k_scan_small(
    u32 k,
    u32 rows,
    const u32 *__restrict__ histT,
    u32 *__restrict__ offT,
    u32 *__restrict__ seg_off,
    u32 *__restrict__ prefix_len,
    unsigned long long *__restrict__ dep,
    int *__restrict__ changed2
) {
  __shared__ u32 red[5];
  const u32 entries = k * rows;
  const u32 tid = threadIdx.x;
  const u32 lane = tid & (kWave - 1);
  u32 carry = 0;
  for (u32 base = 0; base < entries; base += blockDim.x) {
    const u32 i = base + tid;
    u32 v = i < entries ? histT[i] : 0;
    u32 inc = v;
    for (int off = 1; off < 64; off <<= 1) {
      const u32 o = __shfl_up(inc, off, kWave);
      if (lane >= static_cast<u32>(off)) {
        inc += o;
      }
    }
    __syncthreads();
    if (lane == 63) {
      red[tid >> 6] = inc;
    }
    __syncthreads();
    u32 wbase = 0;
    for (u32 w = 0; w < (tid >> 6); ++w) {
      wbase += red[w];
    }
    if (i < entries) {
      offT[i] = carry + wbase + inc - v; // exclusive
    }
    u32 tsum = 0;
    for (u32 w = 0; w < blockDim.x / kWave; ++w) {
      tsum += red[w];
    }
    carry += tsum;
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  for (u32 c = tid; c < k; c += blockDim.x) {
    const u32 b = offT[c * rows];
    seg_off[c] = b;
    if (kInit) {
      const u32 e2 = (c + 1 < k) ? offT[(c + 1) * rows] : carry;
      prefix_len[c] = e2 - b;
      dep[c] = 0;
      dep[k + c] = 0;
    }
  }
  if (tid == 0) {
    seg_off[k] = carry;
    if (kInit) {
      changed2[0] = 0;
      changed2[1] = 0;
    }
  }
}

// Serial rank-order admission for underload-balancer mode: both per-block
// minima (source side) and maxima (target side) are re-checked against live
// weights per move, in deterministic rank order -- the batch analogue of
// underload_balancer.cc's locked per-move checks. Proposal counts in this
// mode are small (only vertices adjacent to underloaded blocks propose).
__global__ void k_commit_underload(
    const Prop *__restrict__ props,
    const u32 *__restrict__ count_dev,
    const i64 *__restrict__ maxw,
    const i64 *__restrict__ minw,
    i64 *__restrict__ weights,
    u32 *__restrict__ labels,
    uint16_t *__restrict__ labels16,
    uint8_t *__restrict__ labels8, // null unless k <= 256
    u32 *__restrict__ admitted_flags,
    unsigned long long *__restrict__ moves
) {
  if (threadIdx.x != 0 || blockIdx.x != 0) {
    return;
  }
  const u32 count = *count_dev;
  unsigned long long mv = 0;
  for (u32 i = 0; i < count; ++i) {
    const Prop pr = props[i];
    const u32 from = labels[pr.u];
    const i64 w = static_cast<i64>(static_cast<i32>(pr.w));
    const i64 mn_from = minw[from];
    const i64 mn_to = minw[pr.to];
    const bool ok = weights[from] >= mn_from && weights[from] - w >= mn_from &&
                    weights[pr.to] < mn_to && weights[pr.to] + w <= maxw[pr.to];
    admitted_flags[i] = ok ? 1u : 0u;
    if (ok) {
      weights[from] -= w;
      weights[pr.to] += w;
      labels[pr.u] = pr.to;
      labels16[pr.u] = static_cast<uint16_t>(pr.to);
      if (labels8 != nullptr) {
        labels8[pr.u] = static_cast<uint8_t>(pr.to);
      }
      ++mv;
    }
  }
  if (mv) {
    atomicAdd(moves, mv);
  }
}

// Apply admitted labels + clear the chunk's unit-active bits (full grid;
// the per-vertex flags were cleared inline by k_phase_s, and activation --
// which re-marks receiving units -- runs in the NEXT kernel, so stream
// order preserves the clear-then-activate semantics).
__global__ void k_apply_v2(
    u32 k,
    u32 pos_lo,
    u32 pos_hi,
    u32 n,
    u64 iter_seed,
    const u32 *__restrict__ seg_off,
    const u32 *__restrict__ prefix_len,
    const u32 *__restrict__ s_u,
    const uint16_t *__restrict__ s_to,
    u32 *__restrict__ labels,
    uint16_t *__restrict__ labels16,
    uint8_t *__restrict__ labels8, // null unless k <= 256
    uint8_t *__restrict__ unit_active,
    u32 *__restrict__ list_counts // M, L, M2 list lengths of this chunk
) {
  // the chunk's phase-A kernels, the last readers of the list counters, are
  // done: leave the counters zero for the next chunk's k_build_lists
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    list_counts[threadIdx.x] = 0;
  }
  const u32 count = seg_off[k];
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    // the scatter leaves entries past a segment's round-1 cutoff unwritten:
    // a stale target c' < k there fails the rank test (i lies outside c' or
    // past its cutoff), a value that is no block at all is caught here
    const u32 c = s_to[i];
    if (c < k && i - seg_off[c] < prefix_len[c]) {
      const u32 u = s_u[i];
      labels[u] = c;
      labels16[u] = static_cast<uint16_t>(c);
      if (labels8 != nullptr) {
        labels8[u] = static_cast<uint8_t>(c);
      }
    }
  }
  {
    const kmp::FeistelPerm fp(kmp::num_units(n), iter_seed);
    const u32 units = (pos_hi - pos_lo) >> 6;
    const u32 u0 = pos_lo >> 6;
    for (u32 uix = blockIdx.x * blockDim.x + threadIdx.x; uix < units; uix += stride) {
      const u32 vb = fp(u0 + uix);
      if (unit_active[vb]) {
        unit_active[vb] = 0;
      }
    }
  }
}

// Activate neighbours of admitted movers. A wave takes a batch of 64
// entries, one per lane, so the s_to -> seg_off/prefix_len and s_u -> xadj
// chains of the whole batch run in parallel; the admitted rows' edges are
// then concatenated through the prefix of their degrees and spread over all
// 64 lanes (nearly all movers have degree <= 16, which left three quarters
// of a wave-per-entry walk idle). The entries of a batch lie waves_total
// apart in the list: a batch of 64 CONSECUTIVE entries measured 7x slower
// (456 vs 65 us per launch at R-MAT scale 26, degree-bucket order), because
// list neighbours come from the same 64-vertex unit and are equally heavy,
// and one wave then walks 64 heavy rows alone. blockDim.x = kActWaves * 64.
constexpr u32 kActWaves = 4;
constexpr u32 kActUnroll = 4;  // adjncy loads in flight per lane
constexpr u32 kActHub = 4096;  // rows above this are walked one at a time

__global__ void k_activate_v2(
    u32 k,
    const u32 *__restrict__ seg_off,
    const u32 *__restrict__ prefix_len,
    const u32 *__restrict__ s_u,
    const uint16_t *__restrict__ s_to,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    uint8_t *__restrict__ active,
    uint8_t *__restrict__ unit_active
) {
  // per wave: exclusive degree prefix and row start of its 64 batch entries
  __shared__ u32 s_pref[kActWaves][kWave];
  __shared__ u64 s_row[kActWaves][kWave];
  const u32 count = seg_off[k];
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = threadIdx.x >> 6;
  const u32 waves_total = (gridDim.x * blockDim.x) >> 6;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  for (u64 b0 = wave_id; b0 < count; b0 += static_cast<u64>(waves_total) * kWave) {
    // one entry per lane, 64 chains at once. The wave's entries lie
    // waves_total apart, as in a wave-per-entry walk: movers of one 64-vertex
    // unit are neighbours in the list and, under a degree-ordered numbering,
    // equally heavy, so consecutive entries on one wave would serialize them
    const u64 i64 = b0 + static_cast<u64>(lane) * waves_total;
    const u32 i = static_cast<u32>(i64);
    u64 row = 0;
    u32 deg = 0;
    if (i64 < count) {
      const u32 c = s_to[i];
      const u32 u = s_u[i];
      // c < k: entries past a round-1 cutoff are unwritten (see k_apply_v2)
      if (c < k && i - seg_off[c] < prefix_len[c]) {
        row = xadj[u];
        deg = static_cast<u32>(xadj[u + 1] - row);
      }
    }
    // rows above kActHub are walked on their own below; the rest are
    // concatenated (prefix <= 64 * kActHub, no overflow)
    const u32 dsm = deg <= kActHub ? deg : 0;
    u32 inc = dsm;
    for (int off = 1; off < 64; off <<= 1) {
      const u32 o = __shfl_up(inc, off, kWave);
      if (lane >= static_cast<u32>(off)) {
        inc += o;
      }
    }
    const u32 total = __shfl(inc, 63, kWave);
    s_pref[wv][lane] = inc - dsm;
    s_row[wv][lane] = row;
    __threadfence_block(); // LDS ordering; the tables are private to this wave

    // concatenated edges over all 64 lanes, kActUnroll loads in flight each
    for (u32 t0 = 0; t0 < total; t0 += kActUnroll * kWave) {
      u32 vv[kActUnroll];
#pragma unroll
      for (u32 j = 0; j < kActUnroll; ++j) {
        const u32 t = t0 + j * kWave + lane;
        // past the end: search for the last edge again (a valid address, so
        // the kActUnroll searches and loads stay free of branches) and
        // drop the value
        const u32 tc = t < total ? t : total - 1;
        // largest entry whose exclusive prefix is <= tc (skips empty rows)
        u32 lo = 0;
#pragma unroll
        for (u32 step = 32; step > 0; step >>= 1) {
          lo += s_pref[wv][lo + step] <= tc ? step : 0;
        }
        const u32 vj = adjncy[s_row[wv][lo] + (tc - s_pref[wv][lo])];
        vv[j] = t < total ? vj : kInvalid;
      }
#pragma unroll
      for (u32 j = 0; j < kActUnroll; ++j) {
        if (vv[j] != kInvalid) {
          // blind stores: measured FASTER than read-test-write (the reads
          // add serialized gather latency; the dirty-line cost is smaller)
          active[vv[j]] = 1;
          unit_active[vv[j] >> 6] = 1;
        }
      }
    }

    // hub rows: the whole wave walks each one
    unsigned long long hubs = __ballot(deg > kActHub);
    while (hubs) {
      const int src = __ffsll(hubs) - 1;
      hubs &= hubs - 1;
      const u64 hrow = s_row[wv][src];
      const u32 hdeg = __shfl(deg, src, kWave);
      for (u32 e0 = 0; e0 < hdeg; e0 += kActUnroll * kWave) {
        u32 vv[kActUnroll];
#pragma unroll
        for (u32 j = 0; j < kActUnroll; ++j) {
          const u32 e2 = e0 + j * kWave + lane;
          vv[j] = e2 < hdeg ? adjncy[hrow + e2] : kInvalid;
        }
#pragma unroll
        for (u32 j = 0; j < kActUnroll; ++j) {
          if (vv[j] != kInvalid) {
            active[vv[j]] = 1;
            unit_active[vv[j] >> 6] = 1;
          }
        }
      }
    }
    __threadfence_block(); // table reuse across grid-stride iterations
  }
}

} // namespace

// ================================================================ engine
struct kmp_lp_t {
  u32 n = 0;
  u64 m = 0;
  u32 k = 0;
  u64 seed = 1;
  u32 C = 0; // positions per chunk
  u32 P = 0; // total positions (pos_count)
  bool has_vwgt = false, has_adjwgt = false;

  // device graph (xadj is u64 device-side: EdgeID-64 everywhere removes the
  // 2^32-arc ceiling at ~zero cost -- xadj reads are per-vertex + coalesced)
  u64 *d_xadj = nullptr;
  u32 *d_adjncy = nullptr;
  i32 *d_vwgt = nullptr;
  i32 *d_adjwgt = nullptr;

  // device LP state
  u32 *d_labels = nullptr;
  u32 *d_labels0 = nullptr;   // initial labels (for kmp_lp_reset)
  uint8_t *d_labels8 = nullptr;   // u8 shadow for refine gathers (k <= 256:
                                  // 64 MB at scale 26, Infinity-Cache-resident)
  uint16_t *d_labels16 = nullptr; // u16 shadow for refine gathers (k <= 2048
                                  // fits; halves the gather cache footprint:
                                  // scale-26 labels 128 MB -> L3-resident)
  i64 *d_weights = nullptr;
  i64 *d_maxw = nullptr;
  i64 *d_minw = nullptr; // per-block minimums (underload mode; else null)
  u32 *d_comm = nullptr; // per-vertex communities (clusterer; else null)
  // communities of e->isolated, in its order (isolated-chain community
  // breaks), and a bound on the community ids: max + 1 of a host array, the
  // partition's k after kmp_lp_set_communities_resident
  std::vector<u32> iso_comm;
  u64 comm_k = 0;
  // scratch of the V-cycle drivers (block weights, isolated-vertex gather):
  // kept and grown on demand, so a cycle pays no hipMalloc / hipFree per call
  void *d_vc_scratch = nullptr;
  size_t vc_scratch_bytes = 0;
  uint8_t *d_active = nullptr;
  uint8_t *d_unit_active = nullptr; // one byte per 64-vertex unit

  // phase buffers
  Prop *d_slots = nullptr; // C
  Prop *d_props = nullptr; // C (compacted; legacy/sharded commit input)
  u64 *d_m_list = nullptr;  // C (built by k_build_lists)
  u32 *d_m_count = nullptr; // base of a 4-u32 alloc; [1]=l, [2]=m2
  u64 *d_l_list = nullptr; // C
  u32 *d_l_count = nullptr; // = d_m_count + 1
  u64 *d_m2_list = nullptr; // C (clustering per-WG hash tier)
  u32 *d_m2_count = nullptr; // = d_m_count + 2
  u32 *d_l_off = nullptr;   // l_cap + 1 (slice prefix)
  u32 *d_l_sizes = nullptr; // l_cap + 1 (slice counts, scan input)
  void *d_lscan_temp = nullptr;
  size_t lscan_temp_bytes = 0;
  i32 *d_l_gains = nullptr; // l_cap x k (refine_begin; dense path, k <= kMaxDenseK)
  u32 l_cap = 0;
  u32 *d_prop_count = nullptr;
  unsigned long long *d_arcs = nullptr;
  unsigned long long *d_moves = nullptr;

  // commit buffers
  u32 *d_sort_keys[2] = {nullptr, nullptr};
  u32 *d_sort_vals[2] = {nullptr, nullptr};
  void *d_sort_temp = nullptr;
  size_t sort_temp_bytes = 0;
  void *d_select_temp = nullptr;
  size_t select_temp_bytes = 0;
  i64 *d_sw = nullptr;
  i64 *d_pw = nullptr;
  void *d_scan_temp = nullptr;
  size_t scan_temp_bytes = 0;
  u32 *d_seg_begin = nullptr, *d_seg_end = nullptr, *d_prefix_len = nullptr;
  unsigned long long *d_dep = nullptr;
  int *d_changed = nullptr;
  u32 *d_admitted_flags = nullptr;
  unsigned long long *d_cut = nullptr;

  // commit v2 (refine, k <= 256): counting sort + cooperative fixpoint.
  // Replaces the per-chunk radix sort / scan-by-key / host fixpoint loop
  // with 4 fixed-shape launches and ZERO host syncs per chunk.
  u32 *d_s_u = nullptr;       // C (sorted-by-target source vertices)
  u32 *d_s_w = nullptr;       // C (their node weights)
  u32 *d_s_r = nullptr;       // C (global ranks; sharded-commit cutoffs)
  uint16_t *d_s_to = nullptr; // C (target block per sorted index)
  uint16_t *d_s_b = nullptr;  // C (source block, frozen at scatter)
  u32 *d_histT = nullptr;     // k x rows column-major histogram
  u32 *d_offT = nullptr;      // its exclusive scan
  u32 *d_seg_off = nullptr;   // k+1 segment offsets
  u32 *d_bar = nullptr;       // grid barrier state (sub[8], root, gen)
  i64 *d_blocksums = nullptr; // coop pw-scan block partials
  u32 coop_nblk = 0;          // resident-guaranteed grid for k_scan_coop
  u32 rows_v2 = 0;            // histogram rows for current k
  u32 max_deg = 0;            // max degree (gates the L-path launches)
  // The v2 train has no memset nodes: d_m_count[0..3) and d_dep (all
  // replicas) are zero between chunks, each cleared by the train kernel that runs after
  // its last reader (k_apply_v2, k_fixpoint_v2). Set by every other path
  // that uses them (v2_clear_train_state restores the invariant).
  bool v2_dirty = true;

  // clustering state
  u32 *d_favored = nullptr;      // n (two-hop favored clusters)
  uint8_t *d_eflag = nullptr;    // n (emptied-cluster flags)
  u32 *d_pool_keys = nullptr;    // pooled L hash
  i32 *d_pool_vals = nullptr;
  u32 *d_l_clist = nullptr;      // claimed-slot lists (pool_slots/2)
  u32 *d_l_ccnt = nullptr;       // C (per-L-vertex claimed counts)
  u64 pool_slots = 0;
  u64 *d_l_hoff = nullptr;       // l_cap+1
  u32 *d_l_hbits = nullptr;      // l_cap
  unsigned long long *d_l_hacc = nullptr; // total region demand of the chunk
  u64 *d_cand = nullptr;         // n (two-hop candidate slots)
  u64 *d_cand2 = nullptr;        // n (sorted)
  u32 *d_cfav = nullptr;         // n
  u32 *d_crank = nullptr;        // n
  u32 *d_cones = nullptr;        // n
  void *d_cand_select_temp = nullptr;
  size_t cand_select_temp_bytes = 0;
  void *d_cand_sort_temp = nullptr;
  size_t cand_sort_temp_bytes = 0;
  void *d_cand_scan_temp = nullptr;
  size_t cand_scan_temp_bytes = 0;
  unsigned long long *d_emptied = nullptr;
  std::vector<u32> isolated;   // host: vertices with degree 0
  std::vector<i32> iso_weights; // their node weights
  bool clusterer = false;
  int balance = 0; // balance mode: overloaded vertices lose "stay" (select)
  // host time of the last kmp_lp_balance: [0] the isolated-vertex pre-pass,
  // [1] the per-chunk fallback downloads + scans (kmp_lp_balance_host_ns)
  u64 balance_host_ns[2] = {0, 0};
  std::vector<i64> maxw_host; // refine caps (host copy, for the fallback)
  i64 maxw_uniform = 0;
  int mp_count = 0; // CUs (for the resident-grid commit kernel)

  // pinned host mirrors
  u32 *h_count = nullptr;
  int *h_changed = nullptr;
  unsigned long long *h_hacc = nullptr;
  unsigned long long *h_moves = nullptr; // [0..1]=moves before/after [2..3]=emptied
  u64 last_emptied = 0;

  // resident label state (rules: include/kaminpar_lp.h, "resident labels"):
  // what d_labels is known to hold, and for a partition the k its values are
  // below. shadows_ok: d_labels16 (and d_labels8 when label_k <= 256) equal
  // d_labels -- true after refine / jet / rebalance, whose every label write
  // also writes the shadows; false after set_labels and project, which write
  // d_labels only.
  enum LabelKind { kLabelsNone = 0, kLabelsClustering = 1, kLabelsPartition = 2 };
  int label_kind = kLabelsNone;
  u32 label_k = 0;
  bool shadows_ok = false;
  // child of kmp_contract_engine: the fine->coarse map of that contraction
  // (parent_n entries, owned) and the parent's identity, compared only
  u32 *d_parent_map = nullptr;
  const void *parent_addr = nullptr;
  u32 parent_n = 0;

  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr; // saved when an external stream is adopted

  // run bookkeeping
  double phase_a_ms = 0.0;
  double commit_ms = 0.0;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;

  hipEvent_t sync_ev = nullptr;

  // captured per-sweep launch trains (v2 refine): graph[i] replays sweep i
  // (all 64 chunk trains + timing events); rebuilt lazily after every
  // refine_begin (buffer pointers change). Replay cost ~launch-free.
  static constexpr int kMaxSweepGraphs = 16;
  hipGraphExec_t sweep_graph[kMaxSweepGraphs] = {};
  uint8_t sweep_seen[kMaxSweepGraphs] = {}; // capture only on the 2nd run
  bool graphs_ok = true; // capture failed once -> plain launches

  void ev_pair(hipEvent_t &a, hipEvent_t &b) {
    if (ev_used + 2 > ev_pool.size()) {
      hipEvent_t x, y;
      HIP_CHECK(hipEventCreate(&x));
      HIP_CHECK(hipEventCreate(&y));
      ev_pool.push_back(x);
      ev_pool.push_back(y);
    }
    a = ev_pool[ev_used];
    b = ev_pool[ev_used + 1];
    ev_used += 2;
  }
};

namespace {

u32 ceil_div(u64 a, u64 b) { return static_cast<u32>((a + b - 1) / b); }

// Blocking hipStreamSynchronize waits cost ~100+ us each on a busy queue
// (yield/interrupt based); the per-chunk control syncs are latency-critical,
// so spin on an event instead (~5 us).
void sync_spin(kmp_lp_t *e);

void engine_alloc_k_buffers(kmp_lp_t *e, u32 k_or_n) {
  // the v2 commit keeps two halves of kDepRep replicas each (dep_slot); the
  // sharded commit uses the first 2 * k entries, legacy paths the first k_or_n
  const u64 dep_n = static_cast<u64>(k_or_n) * (k_or_n <= 256 ? 2 * kDepRep : 1);
  HIP_CHECK(hipMalloc(&e->d_seg_begin, sizeof(u32) * k_or_n));
  HIP_CHECK(hipMalloc(&e->d_seg_end, sizeof(u32) * k_or_n));
  HIP_CHECK(hipMalloc(&e->d_prefix_len, sizeof(u32) * k_or_n));
  HIP_CHECK(hipMalloc(&e->d_dep, sizeof(unsigned long long) * dep_n));
  HIP_CHECK(hipMemsetAsync(e->d_seg_begin, 0, sizeof(u32) * k_or_n, e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_seg_end, 0, sizeof(u32) * k_or_n, e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_prefix_len, 0, sizeof(u32) * k_or_n, e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_dep, 0, sizeof(unsigned long long) * dep_n, e->stream));
}

void engine_destroy_sweep_graphs(kmp_lp_t *e) {
  for (int i = 0; i < kmp_lp_t::kMaxSweepGraphs; ++i) {
    if (e->sweep_graph[i]) {
      (void)hipGraphExecDestroy(e->sweep_graph[i]);
      e->sweep_graph[i] = nullptr;
    }
    e->sweep_seen[i] = 0;
  }
  e->graphs_ok = true;
}

void engine_free_k_buffers(kmp_lp_t *e) {
  if (e->d_seg_begin) {
    HIP_CHECK(hipFree(e->d_seg_begin));
    e->d_seg_begin = nullptr;
  }
  if (e->d_seg_end) {
    HIP_CHECK(hipFree(e->d_seg_end));
    e->d_seg_end = nullptr;
  }
  if (e->d_prefix_len) {
    HIP_CHECK(hipFree(e->d_prefix_len));
    e->d_prefix_len = nullptr;
  }
  if (e->d_dep) {
    HIP_CHECK(hipFree(e->d_dep));
    e->d_dep = nullptr;
  }
}

void sync_spin(kmp_lp_t *e) {
  HIP_CHECK(hipEventRecord(e->sync_ev, e->stream));
  while (true) {
    const hipError_t st = hipEventQuery(e->sync_ev);
    if (st == hipSuccess) {
      return;
    }
    if (st != hipErrorNotReady) {
      HIP_CHECK(st);
    }
  }
}

// Everything an engine allocates beyond the graph arrays themselves
// (LP state, phase/commit buffers, rocprim temps, pinned mirrors).
// Requires e->n, e->m, e->C, e->stream to be set.
void engine_alloc_common(kmp_lp_t *e) {
  HIP_CHECK(hipMalloc(&e->d_labels, sizeof(u32) * e->n));
  HIP_CHECK(hipMalloc(&e->d_labels0, sizeof(u32) * e->n));
  HIP_CHECK(hipMalloc(&e->d_labels16, sizeof(uint16_t) * e->n));
  HIP_CHECK(hipMalloc(&e->d_labels8, e->n));
  HIP_CHECK(hipMalloc(&e->d_active, e->n));
  HIP_CHECK(hipMalloc(&e->d_unit_active, kmp::num_units(e->n)));

  const u32 C = e->C;
  HIP_CHECK(hipMalloc(&e->d_slots, sizeof(Prop) * C));
  HIP_CHECK(hipMalloc(&e->d_props, sizeof(Prop) * C));
  HIP_CHECK(hipMalloc(&e->d_m_list, sizeof(u64) * C));
  HIP_CHECK(hipMalloc(&e->d_m_count, sizeof(u32) * 4)); // [0]=m, [1]=l, [2]=m2
  e->d_l_count = e->d_m_count + 1;
  e->d_m2_count = e->d_m_count + 2;
  HIP_CHECK(hipMalloc(&e->d_l_list, sizeof(u64) * C));
  HIP_CHECK(hipMalloc(&e->d_m2_list, sizeof(u64) * C));

  // commit v2 buffers (sized for the largest supported k = 256 rows layout)
  HIP_CHECK(hipMalloc(&e->d_s_u, sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_s_w, sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_s_to, sizeof(uint16_t) * C));
  HIP_CHECK(hipMalloc(&e->d_s_r, sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_s_b, sizeof(uint16_t) * C));
  HIP_CHECK(hipMalloc(&e->d_histT, sizeof(u32) * 262144));
  HIP_CHECK(hipMalloc(&e->d_offT, sizeof(u32) * 262144));
  HIP_CHECK(hipMalloc(&e->d_seg_off, sizeof(u32) * 257));
  HIP_CHECK(hipMalloc(&e->d_bar, sizeof(u32) * 16));
  HIP_CHECK(hipMemsetAsync(e->d_bar, 0, sizeof(u32) * 16, e->stream));
  HIP_CHECK(hipMalloc(&e->d_blocksums, sizeof(i64) * 512));
  HIP_CHECK(hipMalloc(&e->d_prop_count, sizeof(u32)));
  HIP_CHECK(hipMalloc(&e->d_arcs, sizeof(unsigned long long)));
  HIP_CHECK(hipMalloc(&e->d_moves, sizeof(unsigned long long)));

  HIP_CHECK(hipMalloc(&e->d_sort_keys[0], sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_sort_keys[1], sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_sort_vals[0], sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_sort_vals[1], sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_sw, sizeof(i64) * C));
  HIP_CHECK(hipMalloc(&e->d_pw, sizeof(i64) * C));
  HIP_CHECK(hipMalloc(&e->d_changed, sizeof(int) * 2)); // [round-parity] for coop
  HIP_CHECK(hipMalloc(&e->d_admitted_flags, sizeof(u32) * C));
  HIP_CHECK(hipMalloc(&e->d_cut, sizeof(unsigned long long)));

  rocprim::double_buffer<u32> keys(e->d_sort_keys[0], e->d_sort_keys[1]);
  rocprim::double_buffer<u32> vals(e->d_sort_vals[0], e->d_sort_vals[1]);
  HIP_CHECK(rocprim::radix_sort_pairs(nullptr, e->sort_temp_bytes, keys, vals, C, 0, 32));
  HIP_CHECK(hipMalloc(&e->d_sort_temp, e->sort_temp_bytes));
  HIP_CHECK(rocprim::inclusive_scan_by_key(
      nullptr, e->scan_temp_bytes, e->d_sort_keys[0], e->d_sw, e->d_pw, C, rocprim::plus<i64>(),
      rocprim::equal_to<u32>()
  ));
  HIP_CHECK(hipMalloc(&e->d_scan_temp, e->scan_temp_bytes));
  HIP_CHECK(rocprim::select(
      nullptr, e->select_temp_bytes, e->d_slots, e->d_props, e->d_prop_count, C, PropValid()
  ));
  HIP_CHECK(hipMalloc(&e->d_select_temp, e->select_temp_bytes));

  HIP_CHECK(hipHostMalloc(&e->h_count, sizeof(u32) * 2));
  HIP_CHECK(hipHostMalloc(&e->h_changed, sizeof(int)));
  HIP_CHECK(hipHostMalloc(&e->h_moves, sizeof(unsigned long long) * 4));
  HIP_CHECK(hipHostMalloc(&e->h_hacc, sizeof(unsigned long long)));
}

// A fresh engine that is about to receive its device arrays (kmp_lp_create,
// kmp_contract_engine, kmp_subgraphs_engine, kmp_lp_create_from_edges): its
// own stream, the sync event and the CU count. The caller sets the graph
// arrays, then engine_set_size, engine_alloc_common and an isolated scan.
kmp_lp_t *engine_new_shell() {
  auto *e = new kmp_lp_t();
  HIP_CHECK(hipStreamCreate(&e->stream));
  HIP_CHECK(hipEventCreateWithFlags(&e->sync_ev, hipEventDisableTiming));
  static int cached_mp = 0; // hipGetDeviceProperties costs ms; per-level calls add up
  if (cached_mp == 0) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, dev));
    cached_mp = props.multiProcessorCount;
  }
  e->mp_count = cached_mp;
  return e;
}

void engine_set_size(kmp_lp_t *e, u32 n, u64 m, bool has_vwgt, bool has_adjwgt) {
  e->n = n;
  e->m = m;
  e->C = kmp::chunk_size_for(n);
  e->P = kmp::pos_count(n);
  e->has_vwgt = has_vwgt;
  e->has_adjwgt = has_adjwgt;
}

// Isolated-vertex scan used by the clusterer's isolated-node handling
// (lp_clusterer.cc cluster_isolated_nodes semantics).
template <typename XT>
void engine_scan_isolated(kmp_lp_t *e, const XT *xadj, const i32 *vwgt) {
  u32 maxd = 0;
  for (u32 u = 0; u < e->n; ++u) {
    const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
    if (deg > maxd) {
      maxd = deg;
    }
    if (deg == 0) {
      e->isolated.push_back(u);
      e->iso_weights.push_back(vwgt ? vwgt[u] : 1);
    }
  }
  e->max_deg = maxd;
}

// The same isolated list, weights and max_deg as engine_scan_isolated, from
// the device CSR: only the compacted list and its weights cross PCIe. Runs
// right after engine_alloc_common, when the engine holds no label state yet,
// so the scan borrows d_active (flags), d_labels0 (ids) and d_labels
// (weights) instead of allocating n-sized scratch.
void engine_scan_isolated_device(kmp_lp_t *e) {
  const u32 n = e->n;
  e->max_deg = 0;
  if (n == 0) {
    return;
  }
  hipStream_t s = e->stream;
  u32 *d_stats = e->d_m_count; // 4 u32; [0] max degree, [1] isolated, [2] selected
  kmp_resident::iso_flags(n, e->d_xadj, e->d_active, d_stats, s);
  u32 stats[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  e->max_deg = stats[0];
  const u32 count = stats[1];
  if (count > 0) {
    size_t temp_bytes = 0;
    void *temp = nullptr;
    kmp_resident::iso_select(nullptr, temp_bytes, e->d_active, n, e->d_labels0, d_stats + 2, s);
    HIP_CHECK(hipMalloc(&temp, temp_bytes > 0 ? temp_bytes : 1));
    kmp_resident::iso_select(temp, temp_bytes, e->d_active, n, e->d_labels0, d_stats + 2, s);
    i32 *d_w = reinterpret_cast<i32 *>(e->d_labels);
    kmp_resident::iso_weights(e->d_labels0, count, e->d_vwgt, d_w, s);
    e->isolated.resize(count);
    e->iso_weights.resize(count);
    HIP_CHECK(hipMemcpyAsync(e->isolated.data(), e->d_labels0, sizeof(u32) * count,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(e->iso_weights.data(), d_w, sizeof(i32) * count,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipFree(temp));
  }
  // leave the borrowed counters as every later path expects to find them
  HIP_CHECK(hipMemsetAsync(e->d_m_count, 0, sizeof(u32) * 4, s));
}

hipEvent_t ev_one(kmp_lp_t *e) {
  if (e->ev_used >= e->ev_pool.size()) {
    hipEvent_t x;
    HIP_CHECK(hipEventCreate(&x));
    e->ev_pool.push_back(x);
  }
  return e->ev_pool[e->ev_used++];
}

// ---- commit v2 driver (refine, k <= 256; zero host syncs per chunk) ----

bool v2_eligible(const kmp_lp_t *e) {
  return !e->clusterer && !e->balance && e->k <= 256 && e->coop_nblk >= 8;
}

// Zero what the v2 train expects zero on entry (see kmp_lp_t::v2_dirty).
void v2_clear_train_state(kmp_lp_t *e) {
  HIP_CHECK(hipMemsetAsync(e->d_m_count, 0, sizeof(u32) * 3, e->stream));
  if (e->d_dep != nullptr && e->k <= 256) {
    HIP_CHECK(hipMemsetAsync(
        e->d_dep, 0, sizeof(unsigned long long) * 2 * kDepRep * e->k, e->stream
    ));
  }
  e->v2_dirty = false;
}

// k_build_lists over [pos_lo, pos_hi): M list for degrees in (kSmallDeg,
// mid_hi], M2 list up to m2_hi, L list above; arcs (may be null) receives the
// arcs-scanned tally.
void launch_build_lists(
    kmp_lp_t *e, u32 pos_lo, u32 pos_hi, u64 iseed, u32 mid_hi, u32 m2_hi,
    unsigned long long *arcs
) {
  const u32 rows_bl = 4096;
  const u32 T_bl = ((pos_hi + 63) >> 6) - (pos_lo >> 6);
  const u32 tpw = (T_bl + rows_bl - 1) / rows_bl;
  hipLaunchKernelGGL(
      k_build_lists, dim3(rows_bl / 4), dim3(256), 0, e->stream, pos_lo, pos_hi, e->n, iseed,
      rows_bl, tpw, kSmallDeg, mid_hi, m2_hi, 0xFFFFFFFFu, e->d_xadj, e->d_active,
      e->d_unit_active, e->d_m_list, e->d_m_count, e->d_m2_list, e->d_m2_count, e->d_l_list,
      e->d_l_count, arcs
  );
  LAUNCH_CHECK();
}

// The L prep of the dense tiers. kLPrepKernel: k_l_prep_r, one launch and no
// host call, as the v2 train needs under stream capture. kLPrepScan:
// k_l_sizes and a rocprim scan (the legacy path; slots pre-marked invalid by
// the caller). kLPrepKernel also gates the whole L tier on the graph's
// maximum degree (skip_l_tier in phase_a_dense_tiers).
enum LPrep { kLPrepKernel, kLPrepScan };

// Refine / balance / underload phase A up to kMaxDenseK: the dense gain tiers.
// LT is the gather type, labels_s the shadow of that type. s_always_write is
// k_phase_s's flag (1: it writes every slot of an active unit, so the caller
// needs no slot memset); arcs goes to k_build_lists.
template <typename LT>
void phase_a_dense_tiers(
    kmp_lp_t *e, const LT *labels_s, u32 pos_lo, u32 pos_hi, u32 chunk_base, u64 iseed, u32 mode,
    u32 fallback, u32 s_always_write, unsigned long long *arcs, LPrep l_prep
) {
  const u32 threads = 256;
  const u32 max_degree = 0xFFFFFFFFu;
  const u32 span = pos_hi - pos_lo;
  launch_build_lists(e, pos_lo, pos_hi, iseed, kMidDeg, kMidDeg, arcs);
  // S: kSWavePos positions/wave (unit-gated)
  hipLaunchKernelGGL(
      k_phase_s<LT>, dim3(ceil_div(static_cast<u64>(ceil_div(span, kSWavePos)) * kWave, threads)),
      dim3(threads), 0, e->stream, pos_lo, pos_hi, chunk_base, e->n, iseed, mode, fallback,
      max_degree, s_always_write, e->d_xadj, e->d_adjncy, e->d_vwgt, e->d_adjwgt, e->d_labels,
      e->d_weights, e->d_maxw, e->d_minw, labels_s, e->d_active, e->d_unit_active, e->d_slots
  );
  LAUNCH_CHECK();
  // one wave per M-listed vertex (grid-stride; list built by k_build_lists)
  {
    const size_t lds =
        static_cast<size_t>(threads / kWave) * e->k * gain_replicas(e->k) * sizeof(i32);
    auto *kern = e->has_adjwgt ? k_phase_m<false, LT> : k_phase_m<true, LT>;
    hipLaunchKernelGGL(
        kern, dim3(4096), dim3(threads), lds, e->stream, pos_lo, chunk_base, e->k, iseed, mode,
        fallback, e->d_xadj, e->d_adjncy, e->d_adjwgt, e->d_vwgt, e->d_labels, labels_s,
        e->d_weights, e->d_maxw, e->d_minw, e->d_m_list, e->d_m_count, e->d_slots
    );
    LAUNCH_CHECK();
  }
  // L: slice-parallel accumulation over the (rare) high-degree list. The v2
  // train launches none of the four L kernels on a graph with no row above
  // kMidDeg (every launch counts there); the legacy path always runs the tier.
  const bool skip_l_tier = l_prep == kLPrepKernel && e->max_deg <= kMidDeg;
  if (skip_l_tier) {
    return;
  }
  if (l_prep == kLPrepKernel) {
    hipLaunchKernelGGL(
        k_l_prep_r, dim3(1), dim3(256), 0, e->stream, e->d_l_list, e->d_l_count, e->d_xadj,
        e->l_cap, refine_l_slice(e->k), e->d_l_off
    );
    LAUNCH_CHECK();
  } else {
    HIP_CHECK(hipMemsetAsync(e->d_l_sizes, 0, sizeof(u32) * (e->l_cap + 1), e->stream));
    hipLaunchKernelGGL(
        k_l_sizes, dim3(ceil_div(e->l_cap, 256)), dim3(256), 0, e->stream, e->d_l_list,
        e->d_l_count, e->d_xadj, e->l_cap, refine_l_slice(e->k), e->d_l_sizes
    );
    LAUNCH_CHECK();
    size_t ltb = e->lscan_temp_bytes;
    HIP_CHECK(rocprim::exclusive_scan(
        e->d_lscan_temp, ltb, e->d_l_sizes, e->d_l_off, 0u, e->l_cap + 1, rocprim::plus<u32>(),
        e->stream
    ));
  }
  {
    const size_t hist_lds = static_cast<size_t>(e->k) * gain_replicas(e->k) * sizeof(i32);
    auto *kern = e->has_adjwgt ? k_phase_l_acc<false, LT> : k_phase_l_acc<true, LT>;
    hipLaunchKernelGGL(
        kern, dim3(2048), dim3(256), hist_lds, e->stream, e->k, e->d_xadj, e->d_adjncy,
        e->d_adjwgt, labels_s, e->d_l_list, e->d_l_count, e->l_cap, refine_l_slice(e->k),
        e->d_l_off, e->d_l_gains
    );
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(
      k_phase_l_sel, dim3(2048), dim3(256), 0, e->stream, mode, fallback, pos_lo, chunk_base,
      iseed, e->k, e->d_xadj, e->d_vwgt, e->d_labels, e->d_weights, e->d_maxw, e->d_minw,
      e->d_l_list, e->d_l_count, e->l_cap, e->d_l_gains, e->d_slots
  );
  LAUNCH_CHECK();
  // pathological overflow beyond l_cap: direct per-vertex workgroups
  {
    const size_t lds =
        ((static_cast<size_t>(e->k) * gain_replicas(e->k) + 1) & ~1ull) * sizeof(i32) +
        16 * sizeof(i64);
    auto *kern = e->has_adjwgt ? k_phase_l_direct<false, LT> : k_phase_l_direct<true, LT>;
    hipLaunchKernelGGL(
        kern, dim3(512), dim3(256), lds, e->stream, mode, fallback, pos_lo, chunk_base, iseed,
        e->k, e->d_xadj, e->d_adjncy, e->d_vwgt, e->d_adjwgt, e->d_labels, labels_s, e->d_weights,
        e->d_maxw, e->d_minw, e->d_l_list, e->d_l_count, e->l_cap, e->d_slots
    );
    LAUNCH_CHECK();
  }
}

// Phase A of the v2 train (refine, k <= 256), without slot memsets: S/M/L
// freshly write every slot of an active unit; inactive units are gated
// downstream by unit_active. Issues no host call that syncs (it runs under
// stream capture). The list counters are zero on entry inside the v2 train
// (k_apply_v2 clears them at the end of every chunk); a caller outside it,
// whose commit has no k_apply_v2, passes zero_lists.
void phase_a_v2(
    kmp_lp_t *e, int iter, u32 pos_lo, u32 pos_hi, u32 chunk_base, bool zero_lists
) {
  if (zero_lists) {
    HIP_CHECK(hipMemsetAsync(e->d_m_count, 0, sizeof(u32) * 3, e->stream));
    e->v2_dirty = true;
  }
  phase_a_dense_tiers<uint8_t>(
      e, e->d_labels8, pos_lo, pos_hi, chunk_base, iter_seed_of(e->seed, iter), 0u, kInvalid, 1u,
      e->d_arcs, kLPrepKernel
  );
}

void commit_v2(kmp_lp_t *e, int iter, u32 pos_lo, u32 pos_hi) {
  const u64 iseed = iter_seed_of(e->seed, iter);
  const u32 span = pos_hi - pos_lo;
  const u32 T = span >> 6;
  // clamp the histogram rows to the chunk's tile count (small chunks need
  // neither the full table nor the resident-grid scan)
  u32 rows = (T + 3) & ~3u;
  if (rows < 4) {
    rows = 4;
  }
  if (rows > e->rows_v2) {
    rows = e->rows_v2;
  }
  const u32 tpw = (T + rows - 1) / rows;
  const u32 threads = 256;
  // unit node weights: round 1 of the admission fixpoint runs on the full
  // grid, split over the histogram and the scatter (see k_scatter_v2)
  const bool unit_w = !e->has_vwgt;
  const size_t lds_w = static_cast<size_t>(threads / kWave) * e->k * sizeof(u32);
  const size_t lds_h = unit_w ? 2 * lds_w : lds_w;
  {
    auto *kern = unit_w ? k_hist_v2<true> : k_hist_v2<false>;
    hipLaunchKernelGGL(
        kern, dim3(rows / 4), dim3(threads), lds_h, e->stream, span, pos_lo, e->n, iseed, e->k,
        rows, tpw, e->d_slots, e->d_unit_active, e->d_labels16, e->d_histT, e->d_dep
    );
    LAUNCH_CHECK();
  }
  if (e->k * rows <= 8192) {
    hipLaunchKernelGGL(
        k_scan_small<false>, dim3(1), dim3(threads), 0, e->stream, e->k, rows, e->d_histT,
        e->d_offT, e->d_seg_off, e->d_prefix_len, e->d_dep, e->d_changed
    );
  } else {
    hipLaunchKernelGGL(
        k_scan_coop, dim3(e->coop_nblk), dim3(threads), 0, e->stream, e->k, rows, e->coop_nblk,
        e->d_histT, e->d_offT, e->d_seg_off, e->d_blocksums, e->d_bar
    );
  }
  LAUNCH_CHECK();
  {
    // per-wave cnt, then the u64 hist pair (weighted) or the segment starts,
    // round-1 cutoffs and per-wave departure counts (unit)
    const size_t lds_sc =
        lds_w + (unit_w ? static_cast<size_t>(2 * e->k) * sizeof(u32) + lds_w
                        : static_cast<size_t>(2 * e->k) * sizeof(unsigned long long));
    auto *kern = unit_w ? k_scatter_v2<true> : k_scatter_v2<false>;
    hipLaunchKernelGGL(
        kern, dim3(rows / 4), dim3(threads), lds_sc, e->stream, span, pos_lo, e->n, iseed, e->k,
        rows, tpw, e->d_slots, e->d_unit_active, e->d_offT, e->d_labels16, e->d_seg_off,
        e->d_weights, e->d_maxw, e->d_s_u, e->d_s_w, e->d_s_to, e->d_s_b, e->d_dep
    );
    LAUNCH_CHECK();
  }
  {
    auto *kern = unit_w ? k_fixpoint_v2<false> : k_fixpoint_v2<true>;
    hipLaunchKernelGGL(
        kern, dim3(1), dim3(threads), 0, e->stream, e->k, e->d_seg_off, e->d_prefix_len,
        e->d_dep, e->d_s_w, e->d_s_b, e->d_weights, e->d_maxw, e->d_moves, e->d_pw
    );
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(
      k_apply_v2, dim3(2048), dim3(threads), 0, e->stream, e->k, pos_lo, pos_hi, e->n, iseed,
      e->d_seg_off, e->d_prefix_len, e->d_s_u, e->d_s_to, e->d_labels, e->d_labels16,
      e->d_labels8, e->d_unit_active, e->d_m_count
  );
  LAUNCH_CHECK();
  // one thread per chunk position (the entry count cannot exceed the span),
  // capped at the resident grid: small chunks then still fill the lanes of
  // their waves instead of leaving one entry each to 8192 waves
  const u32 act_threads = kActWaves * kWave;
  const u32 act_blocks_span = ceil_div(span, act_threads);
  const u32 act_blocks = act_blocks_span < 2048u ? act_blocks_span : 2048u;
  hipLaunchKernelGGL(
      k_activate_v2, dim3(act_blocks), dim3(act_threads), 0, e->stream, e->k, e->d_seg_off,
      e->d_prefix_len, e->d_s_u, e->d_s_to, e->d_xadj, e->d_adjncy, e->d_active,
      e->d_unit_active
  );
  LAUNCH_CHECK();
}

// One sweep = 64 chunk trains enqueued back-to-back with no host sync; the
// single sync per sweep reads the device move counter (early-exit check)
// and settles the per-chunk timing events.
// Enqueue one full sweep's chunk trains (the capture body; zero host syncs
// inside). Events use a per-sweep slice of the pool so each captured graph
// owns distinct event objects across replays.
void enqueue_sweep_v2(kmp_lp_t *e, int iter, size_t *ev_base_io) {
  e->ev_used = *ev_base_io;
  for (u32 chunk = 0; chunk < kmp::kNumChunks; ++chunk) {
    const u32 pos_lo = chunk * e->C;
    const u32 pos_hi = pos_lo + e->C > e->P ? e->P : pos_lo + e->C;
    if (pos_lo >= pos_hi) {
      continue;
    }
    hipEvent_t a0 = ev_one(e), a1 = ev_one(e), c1 = ev_one(e);
    HIP_CHECK(hipEventRecord(a0, e->stream));
    phase_a_v2(e, iter, pos_lo, pos_hi, pos_lo, false);
    HIP_CHECK(hipEventRecord(a1, e->stream));
    commit_v2(e, iter, pos_lo, pos_hi);
    HIP_CHECK(hipEventRecord(c1, e->stream));
  }
  *ev_base_io = e->ev_used;
}

i64 run_sweeps_v2(kmp_lp_t *e, int iters) {
  if (e->v2_dirty) {
    v2_clear_train_state(e); // another path ran on this engine since setup
  }
  HIP_CHECK(hipMemcpyAsync(&e->h_moves[0], e->d_moves, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, e->stream));
  sync_spin(e);
  unsigned long long last = e->h_moves[0];
  u64 total = 0;
  // per-sweep event slice size (3 events per non-empty chunk)
  u32 nonempty = 0;
  for (u32 chunk = 0; chunk < kmp::kNumChunks; ++chunk) {
    const u32 pos_lo = chunk * e->C;
    if (pos_lo < e->P) {
      ++nonempty;
    }
  }
  const size_t slice = static_cast<size_t>(nonempty) * 3;
  for (int iter = 0; iter < iters; ++iter) {
    size_t ev_base = (iter < kmp_lp_t::kMaxSweepGraphs ? iter : 0) * slice;
    const size_t ev_lo = ev_base;
    // capture only on the sweep's SECOND execution: one-shot callers (the
    // multilevel levels) skip the instantiate cost, repeated callers (the
    // bench steps) replay launch-overhead-free from step 2
    const bool can_graph = e->graphs_ok && iter < kmp_lp_t::kMaxSweepGraphs &&
                           e->sweep_seen[iter] != 0;
    if (iter < kmp_lp_t::kMaxSweepGraphs && e->sweep_seen[iter] == 0) {
      e->sweep_seen[iter] = 1;
    }
    if (can_graph && e->sweep_graph[iter] == nullptr) {
      // capture this sweep's train once; replays are launch-overhead-free
      // (the train is fixed-shape: counts are read on device, no host
      // syncs, and the per-chunk args depend only on (iter, chunk))
      hipError_t st = hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed);
      if (st == hipSuccess) {
        enqueue_sweep_v2(e, iter, &ev_base);
        hipGraph_t graph = nullptr;
        st = hipStreamEndCapture(e->stream, &graph);
        if (st == hipSuccess && graph != nullptr) {
          st = hipGraphInstantiate(&e->sweep_graph[iter], graph, nullptr, nullptr, 0);
          (void)hipGraphDestroy(graph);
        }
      }
      if (st != hipSuccess || e->sweep_graph[iter] == nullptr) {
        (void)hipGetLastError();
        e->graphs_ok = false; // fall back to plain launches for good
        e->sweep_graph[iter] = nullptr;
      }
    }
    if (can_graph && e->sweep_graph[iter] != nullptr) {
      HIP_CHECK(hipGraphLaunch(e->sweep_graph[iter], e->stream));
      ev_base = ev_lo + slice;
    } else {
      enqueue_sweep_v2(e, iter, &ev_base);
    }
    HIP_CHECK(hipMemcpyAsync(&e->h_moves[1], e->d_moves, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, e->stream));
    sync_spin(e);
    for (size_t i = ev_lo; i + 2 < ev_base; i += 3) {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
      e->phase_a_ms += ms;
      HIP_CHECK(hipEventElapsedTime(&ms, e->ev_pool[i + 1], e->ev_pool[i + 2]));
      e->commit_ms += ms;
    }
    const unsigned long long cur = e->h_moves[1];
    const u64 sweep_moves = cur - last;
    last = cur;
    total += sweep_moves;
    if (sweep_moves == 0) {
      break;
    }
  }
  return static_cast<i64>(total);
}

// The pooled global hash of the L tier and its per-list-entry arrays (the
// clusterer's, and the refiner's above kMaxDenseK). Allocated once.
void engine_ensure_l_pool(kmp_lp_t *e) {
  if (e->d_pool_keys != nullptr) {
    return;
  }
  HIP_CHECK(hipMalloc(&e->d_l_hacc, sizeof(unsigned long long)));
  HIP_CHECK(hipMalloc(&e->d_l_hoff, sizeof(u64) * (e->C + 1)));
  HIP_CHECK(hipMalloc(&e->d_l_hbits, sizeof(u32) * e->C));
  // pooled hash for high-degree rows: ~8 slots per average chunk arc
  u64 slots = (e->m / kmp::kNumChunks) * 8;
  if (slots < (1ull << 22)) {
    slots = 1ull << 22;
  }
  if (slots > (1ull << 27)) {
    slots = 1ull << 27;
  }
  e->pool_slots = slots;
  HIP_CHECK(hipMalloc(&e->d_pool_keys, sizeof(u32) * slots));
  HIP_CHECK(hipMalloc(&e->d_pool_vals, sizeof(i32) * slots));
  HIP_CHECK(hipMemset(e->d_pool_keys, 0xFF, sizeof(u32) * slots));
  HIP_CHECK(hipMemset(e->d_pool_vals, 0, sizeof(i32) * slots));
  HIP_CHECK(hipMalloc(&e->d_l_clist, sizeof(u32) * (slots / 2)));
  HIP_CHECK(hipMalloc(&e->d_l_ccnt, sizeof(u32) * e->C));
}

// After k_l_prep_c: read back the L count and the chunk's total hash-region
// demand, and run launch_batch(lo, hi) over the L list. When the demand
// exceeds the pool (hub-dense chunks, e.g. after degree-bucket rearrangement
// packs 64 hubs per permutation unit), the list goes in pool-sized batches --
// the selection kernels clear each region after reading it, so batches can
// reuse the pool safely.
template <typename F>
void l_pool_batches(kmp_lp_t *e, F launch_batch) {
  HIP_CHECK(hipMemcpyAsync(
      e->h_count + 1, e->d_l_count, sizeof(u32), hipMemcpyDeviceToHost, e->stream
  ));
  HIP_CHECK(hipMemcpyAsync(
      e->h_hacc, e->d_l_hacc, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream
  ));
  sync_spin(e);
  const u32 lcount = e->h_count[1] < e->l_cap ? e->h_count[1] : e->l_cap;
  const u64 hacc = *e->h_hacc;
  if (lcount > 0 && hacc <= e->pool_slots) {
    launch_batch(0u, lcount);
  } else if (lcount > 0) {
    std::vector<u64> hoff(lcount + 1);
    HIP_CHECK(hipMemcpyAsync(
        hoff.data(), e->d_l_hoff, sizeof(u64) * (lcount + 1), hipMemcpyDeviceToHost, e->stream
    ));
    sync_spin(e);
    u32 lo = 0;
    while (lo < lcount) {
      const u64 need_one = hoff[lo + 1] - hoff[lo];
      if (need_one > e->pool_slots) {
        // a single region larger than the pool: grow it
        HIP_CHECK(hipFree(e->d_pool_keys));
        HIP_CHECK(hipFree(e->d_pool_vals));
        HIP_CHECK(hipFree(e->d_l_clist));
        e->pool_slots = need_one;
        HIP_CHECK(hipMalloc(&e->d_pool_keys, sizeof(u32) * e->pool_slots));
        HIP_CHECK(hipMalloc(&e->d_pool_vals, sizeof(i32) * e->pool_slots));
        HIP_CHECK(hipMalloc(&e->d_l_clist, sizeof(u32) * (e->pool_slots / 2)));
        HIP_CHECK(hipMemsetAsync(e->d_pool_keys, 0xFF, sizeof(u32) * e->pool_slots, e->stream));
        HIP_CHECK(hipMemsetAsync(e->d_pool_vals, 0, sizeof(i32) * e->pool_slots, e->stream));
      }
      u32 hi = lo + 1;
      while (hi < lcount && hoff[hi + 1] - hoff[lo] <= e->pool_slots) {
        ++hi;
      }
      launch_batch(lo, hi);
      lo = hi;
    }
  }
}

// Balance mode: the per-chunk fallback target = lightest block with room, for
// overloaded vertices with no admissible adjacent candidate. O(k) on the host.
u32 balance_fallback(kmp_lp_t *e) {
  u32 fallback = kInvalid;
  if (e->balance == 1) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<i64> w(e->k);
    HIP_CHECK(hipMemcpyAsync(w.data(), e->d_weights, sizeof(i64) * e->k, hipMemcpyDeviceToHost,
                             e->stream));
    sync_spin(e);
    i64 bw = -1;
    for (u32 c = 0; c < e->k; ++c) {
      if (w[c] < e->maxw_host[c] && (bw < 0 || w[c] < bw)) {
        bw = w[c];
        fallback = c;
      }
    }
    e->balance_host_ns[1] += static_cast<u64>(
        std::chrono::duration_cast<std::chrono::nanoseconds>(
            std::chrono::steady_clock::now() - t0).count());
  }
  return fallback;
}

// Block weights of the current d_labels into the zeroed d_weights.
void launch_init_weights(kmp_lp_t *e) {
  const u32 threads = 256;
  auto *w = reinterpret_cast<unsigned long long *>(e->d_weights);
  if (e->k > kMaxDenseK) {
    u32 grid = ceil_div(e->n, threads);
    if (grid > 2048) {
      grid = 2048;
    }
    hipLaunchKernelGGL(
        k_init_weights_direct, dim3(grid), dim3(threads), 0, e->stream, e->n, e->d_labels,
        e->d_vwgt, w
    );
  } else {
    const size_t lds = static_cast<size_t>(e->k) * sizeof(unsigned long long);
    hipLaunchKernelGGL(
        k_init_weights, dim3(2048), dim3(threads), lds, e->stream, e->n, e->k, e->d_labels,
        e->d_vwgt, w
    );
  }
  LAUNCH_CHECK();
}

// Refine / balance phase A above kMaxDenseK: the hash gain tiers. The S kernel
// is k_phase_s itself; only its gather type changes.
template <typename LT>
void phase_a_hash_tiers(
    kmp_lp_t *e, const LT *labels_s, u32 pos_lo, u32 pos_hi, u32 chunk_base, u64 iseed,
    u32 fallback
) {
  const u32 threads = 256;
  const u32 max_degree = 0xFFFFFFFFu;
  const u32 span = pos_hi - pos_lo;
  const u32 mode = static_cast<u32>(e->balance);
  launch_build_lists(e, pos_lo, pos_hi, iseed, kClusterMidDeg, kClusterM2Deg, nullptr);
  hipLaunchKernelGGL(
      k_phase_s<LT>, dim3(ceil_div(static_cast<u64>(ceil_div(span, kSWavePos)) * kWave, threads)),
      dim3(threads), 0, e->stream, pos_lo, pos_hi, chunk_base, e->n, iseed, mode, fallback,
      max_degree, 0u, e->d_xadj, e->d_adjncy, e->d_vwgt, e->d_adjwgt, e->d_labels, e->d_weights,
      e->d_maxw, static_cast<const i64 *>(nullptr), labels_s, e->d_active, e->d_unit_active,
      e->d_slots
  );
  LAUNCH_CHECK();
  {
    const size_t lds = static_cast<size_t>(threads / kWave) * 2 * kHashSlots * sizeof(u32);
    auto *kern = e->has_adjwgt ? k_phase_m_h<false, LT> : k_phase_m_h<true, LT>;
    hipLaunchKernelGGL(
        kern, dim3(4096), dim3(threads), lds, e->stream, pos_lo, chunk_base, iseed, mode, fallback,
        e->d_xadj, e->d_adjncy, e->d_adjwgt, e->d_vwgt, e->d_labels, labels_s, e->d_weights,
        e->d_maxw, e->d_m_list, e->d_m_count, e->d_slots
    );
    LAUNCH_CHECK();
    auto *kern2 = e->has_adjwgt ? k_phase_m2_h<false, LT> : k_phase_m2_h<true, LT>;
    hipLaunchKernelGGL(
        kern2, dim3(1024), dim3(threads), 0, e->stream, pos_lo, chunk_base, iseed, mode, fallback,
        e->d_xadj, e->d_adjncy, e->d_adjwgt, e->d_vwgt, e->d_labels, labels_s, e->d_weights,
        e->d_maxw, e->d_m2_list, e->d_m2_count, e->d_slots
    );
    LAUNCH_CHECK();
  }
  if (e->max_deg > kClusterM2Deg) {
    hipLaunchKernelGGL(
        k_l_prep_c, dim3(1), dim3(1024), 0, e->stream, e->d_l_list, e->d_l_count, e->d_xadj,
        e->l_cap, e->d_l_off, e->d_l_hoff, e->d_l_hbits, e->d_l_ccnt, e->d_l_hacc
    );
    LAUNCH_CHECK();
    auto *kern = e->has_adjwgt ? k_phase_l_acc_c<false> : k_phase_l_acc_c<true>;
    l_pool_batches(e, [&](u32 lo, u32 hi) {
      hipLaunchKernelGGL(
          kern, dim3(2048), dim3(256), 0, e->stream, e->d_xadj, e->d_adjncy, e->d_adjwgt,
          e->d_labels, e->d_l_list, lo, hi, e->d_l_off, e->d_l_hoff, e->d_l_hbits, e->d_pool_keys,
          e->d_pool_vals, e->d_l_clist, e->d_l_ccnt
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_phase_l_sel_h, dim3(2048), dim3(256), 0, e->stream, pos_lo, chunk_base, iseed, mode,
          fallback, e->d_vwgt, e->d_labels, e->d_weights, e->d_maxw, e->d_l_list, lo, hi,
          e->d_l_hoff, e->d_pool_keys, e->d_pool_vals, e->d_l_clist, e->d_l_ccnt, e->d_slots
      );
      LAUNCH_CHECK();
    });
  }
}

} // namespace

extern "C" {

kmp_lp_t *kmp_lp_create(const kmp_graph_t *g) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fprintf(stderr, "kaminpar_amd: no HIP device available -- the LP engine requires a GPU\n");
    return nullptr;
  }

  (void)hipSetDeviceFlags(hipDeviceScheduleSpin); // ignore if context exists
  kmp_lp_t *e = engine_new_shell();
  engine_set_size(
      e, kmp_graph_n(g), kmp_graph_m(g), kmp_graph_vwgt(g) != nullptr,
      kmp_graph_adjwgt(g) != nullptr
  );

  HIP_CHECK(hipMalloc(&e->d_xadj, sizeof(u64) * (e->n + 1)));
  HIP_CHECK(hipMalloc(&e->d_adjncy, sizeof(u32) * e->m));
  // device xadj is u64 (EdgeID-64); widen u32 host offsets on upload
  const u64 *xadj64 = kmp_graph_xadj64(g);
  if (xadj64 != nullptr) {
    HIP_CHECK(
        hipMemcpy(e->d_xadj, xadj64, sizeof(u64) * (e->n + 1), hipMemcpyHostToDevice)
    );
  } else {
    const u32 *x32 = kmp_graph_xadj(g);
    std::vector<u64> wide(static_cast<size_t>(e->n) + 1);
    for (u32 i = 0; i <= e->n; ++i) {
      wide[i] = x32[i];
    }
    HIP_CHECK(
        hipMemcpy(e->d_xadj, wide.data(), sizeof(u64) * (e->n + 1), hipMemcpyHostToDevice)
    );
  }
  HIP_CHECK(hipMemcpy(e->d_adjncy, kmp_graph_adjncy(g), sizeof(u32) * e->m, hipMemcpyHostToDevice));
  if (e->has_vwgt) {
    HIP_CHECK(hipMalloc(&e->d_vwgt, sizeof(i32) * e->n));
    HIP_CHECK(hipMemcpy(e->d_vwgt, kmp_graph_vwgt(g), sizeof(i32) * e->n, hipMemcpyHostToDevice));
  }
  if (e->has_adjwgt) {
    HIP_CHECK(hipMalloc(&e->d_adjwgt, sizeof(i32) * e->m));
    HIP_CHECK(
        hipMemcpy(e->d_adjwgt, kmp_graph_adjwgt(g), sizeof(i32) * e->m, hipMemcpyHostToDevice)
    );
  }

  engine_alloc_common(e);
  if (kmp_graph_xadj64(g) != nullptr) {
    engine_scan_isolated(e, kmp_graph_xadj64(g), kmp_graph_vwgt(g));
  } else {
    engine_scan_isolated(e, kmp_graph_xadj(g), kmp_graph_vwgt(g));
  }
  return e;
}

void kmp_lp_free(kmp_lp_t *e) {
  if (!e) {
    return;
  }
  HIP_CHECK(hipDeviceSynchronize());
  engine_destroy_sweep_graphs(e);
  for (hipEvent_t ev : e->ev_pool) {
    (void)hipEventDestroy(ev);
  }
  if (e->sync_ev) {
    (void)hipEventDestroy(e->sync_ev);
  }
  engine_free_k_buffers(e);
  for (void *p : {(void *)e->d_xadj, (void *)e->d_adjncy, (void *)e->d_vwgt, (void *)e->d_adjwgt,
                  (void *)e->d_labels, (void *)e->d_labels0, (void *)e->d_labels16, (void *)e->d_labels8, (void *)e->d_weights, (void *)e->d_maxw, (void *)e->d_minw, (void *)e->d_comm, (void *)e->d_active, (void *)e->d_unit_active,
                  (void *)e->d_slots, (void *)e->d_props,
                  (void *)e->d_m_list, (void *)e->d_m_count, (void *)e->d_m2_list,
                  (void *)e->d_l_list, (void *)e->d_l_off, (void *)e->d_l_sizes, (void *)e->d_lscan_temp, (void *)e->d_l_gains, (void *)e->d_prop_count, (void *)e->d_arcs,
                  (void *)e->d_moves, (void *)e->d_sort_keys[0], (void *)e->d_sort_keys[1],
                  (void *)e->d_sort_vals[0], (void *)e->d_sort_vals[1], (void *)e->d_sort_temp,
                  (void *)e->d_select_temp, (void *)e->d_sw, (void *)e->d_pw,
                  (void *)e->d_scan_temp, (void *)e->d_changed, (void *)e->d_admitted_flags,
                  (void *)e->d_cut, (void *)e->d_s_u, (void *)e->d_s_w, (void *)e->d_s_r, (void *)e->d_s_to,
                  (void *)e->d_s_b, (void *)e->d_histT, (void *)e->d_offT, (void *)e->d_seg_off,
                  (void *)e->d_bar, (void *)e->d_blocksums, (void *)e->d_parent_map,
                  e->d_vc_scratch}) {
    if (p) {
      (void)hipFree(p);
    }
  }
  for (void *p : {(void *)e->d_favored, (void *)e->d_eflag, (void *)e->d_pool_keys,
                  (void *)e->d_pool_vals, (void *)e->d_l_clist, (void *)e->d_l_ccnt,
                  (void *)e->d_l_hoff, (void *)e->d_l_hbits,
                  (void *)e->d_l_hacc, (void *)e->d_cand, (void *)e->d_cand2,
                  (void *)e->d_cfav, (void *)e->d_crank, (void *)e->d_cones,
                  (void *)e->d_cand_select_temp, (void *)e->d_cand_sort_temp,
                  (void *)e->d_cand_scan_temp, (void *)e->d_emptied}) {
    if (p) {
      (void)hipFree(p);
    }
  }
  if (e->h_count) {
    (void)hipHostFree(e->h_count);
  }
  if (e->h_changed) {
    (void)hipHostFree(e->h_changed);
  }
  if (e->h_moves) {
    (void)hipHostFree(e->h_moves);
  }
  if (e->h_hacc) {
    (void)hipHostFree(e->h_hacc);
  }
  (void)hipStreamDestroy(e->own_stream != nullptr ? e->own_stream : e->stream);
  delete e;
}

u32 kmp_lp_num_chunks(const kmp_lp_t *) { return kmp::kNumChunks; }

// Adopt an external HIP stream (e.g. torch's current stream) so the
// multi-GPU driver's collectives and the engine's kernels share ONE stream
// and the per-call cross-stream hipStreamSynchronize bridges disappear.
// Pass 0 to restore the engine's own stream. The engine must be idle.
int kmp_lp_set_stream(kmp_lp_t *e, void *external_stream) {
  HIP_CHECK(hipStreamSynchronize(e->stream));
  engine_destroy_sweep_graphs(e); // graphs are bound to the old stream
  if (external_stream != nullptr) {
    if (e->own_stream == nullptr) {
      e->own_stream = e->stream;
    }
    e->stream = static_cast<hipStream_t>(external_stream);
  } else if (e->own_stream != nullptr) {
    e->stream = e->own_stream;
    e->own_stream = nullptr;
  }
  return 0;
}

// kmp_lp_refine_begin in three parts, so that a caller holding labels on the
// device (kmp_lp_jet's rebalance step) can restart balance sweeps without
// reallocating the per-k buffers or moving n-sized arrays over PCIe:
//   refine_setup        per-k buffers, caps (once per call)
//   refine_load_state   LP state derived from the CURRENT d_labels
//   refine_setup_commit commit-v2 launch shape
static int refine_setup(kmp_lp_t *e, u32 k, const i64 *max_block_weights, u64 seed) {
  if (k > KMP_LP_MAX_K) {
    fprintf(stderr, "kaminpar_amd: refine supports k <= %u (got %u)\n",
            static_cast<u32>(KMP_LP_MAX_K), k);
    return -1;
  }
  const bool hash_tiers = k > kMaxDenseK;
  e->k = k;
  e->seed = seed;
  e->clusterer = false;
  e->maxw_host.assign(max_block_weights, max_block_weights + k);
  e->phase_a_ms = 0.0;
  e->commit_ms = 0.0;
  e->ev_used = 0;

  engine_destroy_sweep_graphs(e);
  engine_free_k_buffers(e);
  engine_alloc_k_buffers(e, k);

  if (e->d_weights) {
    HIP_CHECK(hipFree(e->d_weights));
  }
  if (e->d_maxw) {
    HIP_CHECK(hipFree(e->d_maxw));
  }
  HIP_CHECK(hipMalloc(&e->d_weights, sizeof(i64) * k));
  HIP_CHECK(hipMalloc(&e->d_maxw, sizeof(i64) * k));
  if (e->d_l_off) {
    HIP_CHECK(hipFree(e->d_l_off));
  }
  if (e->d_l_gains) {
    HIP_CHECK(hipFree(e->d_l_gains));
    e->d_l_gains = nullptr;
  }
  if (e->d_l_sizes) {
    HIP_CHECK(hipFree(e->d_l_sizes));
    e->d_l_sizes = nullptr;
  }
  if (e->d_lscan_temp) {
    HIP_CHECK(hipFree(e->d_lscan_temp));
    e->d_lscan_temp = nullptr;
  }
  if (hash_tiers) {
    // the L tier is the pooled hash, sized by degree: no l_cap x k gain rows,
    // and the L list may hold a whole chunk
    e->l_cap = e->C;
    HIP_CHECK(hipMalloc(&e->d_l_off, sizeof(u32) * (e->l_cap + 1)));
    engine_ensure_l_pool(e);
    HIP_CHECK(hipMemcpy(e->d_maxw, max_block_weights, sizeof(i64) * k, hipMemcpyHostToDevice));
    return 0;
  }
  e->l_cap = (1u << 22) / k;
  if (e->l_cap > e->C) {
    e->l_cap = e->C;
  }
  if (e->l_cap < 1024) {
    e->l_cap = 1024;
  }
  HIP_CHECK(hipMalloc(&e->d_l_off, sizeof(u32) * (e->l_cap + 1)));
  HIP_CHECK(hipMalloc(&e->d_l_sizes, sizeof(u32) * (e->l_cap + 1)));
  HIP_CHECK(rocprim::exclusive_scan(
      nullptr, e->lscan_temp_bytes, e->d_l_sizes, e->d_l_off, 0u, e->l_cap + 1
  ));
  HIP_CHECK(hipMalloc(&e->d_lscan_temp, e->lscan_temp_bytes));
  HIP_CHECK(hipMalloc(&e->d_l_gains, sizeof(i32) * e->l_cap * k));
  HIP_CHECK(hipMemsetAsync(e->d_l_gains, 0, sizeof(i32) * e->l_cap * k, e->stream));
  HIP_CHECK(hipMemcpy(e->d_maxw, max_block_weights, sizeof(i64) * k, hipMemcpyHostToDevice));
  return 0;
}

static void refine_load_state(kmp_lp_t *e, bool snapshot_initial) {
  const u32 k = e->k;
  if (snapshot_initial) {
    HIP_CHECK(hipMemcpyAsync(
        e->d_labels0, e->d_labels, sizeof(u32) * e->n, hipMemcpyDeviceToDevice, e->stream
    ));
  }
  HIP_CHECK(hipMemsetAsync(e->d_active, 1, e->n, e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_unit_active, 1, kmp::num_units(e->n), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_arcs, 0, sizeof(unsigned long long), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_moves, 0, sizeof(unsigned long long), e->stream));

  HIP_CHECK(hipMemsetAsync(e->d_weights, 0, sizeof(i64) * k, e->stream));
  {
    const u32 threads = 256;
    hipLaunchKernelGGL(
        k_sync_labels16, dim3(ceil_div(e->n, threads)), dim3(threads), 0, e->stream, e->n,
        e->d_labels, e->d_labels16, e->d_labels8
    );
    LAUNCH_CHECK();
    launch_init_weights(e);
  }
}

static void refine_setup_commit(kmp_lp_t *e) {
  const u32 k = e->k;
  // commit v2 setup: histogram row count + resident-guaranteed grid for the
  // single-launch commit kernel (falls back to the legacy commit if the
  // occupancy query says the grid cannot be made co-resident). The grid is
  // deliberately SMALL (64 blocks): the commit stages are latency-bound and
  // the grid barrier cost grows with the block count (tools/bar_bench.hip).
  {
    // histogram rows: enough waves to hide tile-load latency even at
    // k = 256 (a 256-row table serialized 256 tiles per wave at scale 28 --
    // measured regression); table <= 262144 entries = 1 MB
    u32 rows = (262144u / k) & ~3u;
    if (rows < 256) {
      rows = 256;
    }
    if (rows > 4096) {
      rows = 4096;
    }
    e->rows_v2 = rows;
  }
  e->coop_nblk = 0;
  if (k <= 256) {
    int occ_scan = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_scan, k_scan_coop, 256, 0) ==
            hipSuccess &&
        occ_scan > 0 && e->mp_count > 0) {
      u64 nb = static_cast<u64>(occ_scan) * static_cast<u64>(e->mp_count);
      if (nb > 64) {
        nb = 64;
      }
      nb &= ~7ull;
      e->coop_nblk = static_cast<u32>(nb);
    }
  }
  v2_clear_train_state(e);
}

// The resident forms of refine / jet / rebalance start from e->d_labels as it
// is. Every way into the partition kind is validated (kmp_lp_set_labels on
// the host; the refiners and the projection by construction), so this host
// comparison replaces the n-label validation pass: no kernel indexing a
// k-sized LDS table ever sees an unvalidated label.
static int resident_partition_ok(const kmp_lp_t *e, u32 k, const char *who) {
  if (e->label_kind != kmp_lp_t::kLabelsPartition) {
    fprintf(stderr, "kaminpar_amd: %s: no resident partition (partition == NULL needs one)\n",
            who);
    return -1;
  }
  if (e->label_k > k) {
    fprintf(stderr, "kaminpar_amd: %s: the resident partition has k = %u, the call k = %u\n", who,
            e->label_k, k);
    return -1;
  }
  return 0;
}

// partition == nullptr: start from the labels already in e->d_labels. counted:
// the upload is label traffic of a counted entry point (see label_traffic).
static int labels_below_k(const u32 *partition, u32 n, u32 k, const char *who) {
  for (u32 u = 0; u < n; ++u) {
    if (partition[u] >= k) {
      fprintf(stderr, "kaminpar_amd: %s: partition[%u] = %u is not below k = %u\n", who, u,
              partition[u], k);
      return -1;
    }
  }
  return 0;
}

// Jet, the selection rebalancer and the underload balancer keep k-sized LDS
// tables of their own: they stay at kMaxDenseK whatever refine accepts.
static int dense_k_ok(u32 k, const char *who) {
  if (k > kMaxDenseK) {
    fprintf(stderr, "kaminpar_amd: %s supports k <= %u (got %u)\n", who, kMaxDenseK, k);
    return -1;
  }
  return 0;
}

static int refine_begin_impl(
    kmp_lp_t *e, u32 k, const i64 *max_block_weights, const u32 *partition, u64 seed, bool counted
) {
  // above kMaxDenseK labels index k-sized global arrays: reject out-of-range
  // input on the host (a resident partition was validated when it became one)
  if (k > kMaxDenseK && k <= KMP_LP_MAX_K && partition != nullptr &&
      labels_below_k(partition, e->n, k, "refine") != 0) {
    return -1;
  }
  if (refine_setup(e, k, max_block_weights, seed) != 0) {
    return -1;
  }
  if (partition != nullptr) {
    const size_t bytes = sizeof(u32) * e->n;
    HIP_CHECK(hipMemcpy(e->d_labels, partition, counted ? label_traffic(bytes) : bytes,
                        hipMemcpyHostToDevice));
  }
  refine_load_state(e, true);
  refine_setup_commit(e);
  HIP_CHECK(hipStreamSynchronize(e->stream));
  return 0;
}

int kmp_lp_refine_begin(
    kmp_lp_t *e, u32 k, const i64 *max_block_weights, const u32 *partition, u64 seed
) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  return refine_begin_impl(e, k, max_block_weights, partition, seed, false);
}

i64 kmp_lp_phase_a(
    kmp_lp_t *e, int iter, u32 chunk, u32 pos_lo, u32 pos_hi, void *d_out, u32 cap
) {
  const u64 iseed = iter_seed_of(e->seed, iter);
  const u32 chunk_base = chunk * e->C;
  Prop *out = static_cast<Prop *>(d_out);
  const u32 span = pos_hi - pos_lo;
  if (span == 0) {
    return 0; // empty rank slice
  }
  const u32 threads = 256;
  const u32 max_degree = 0xFFFFFFFFu;

  HIP_CHECK(hipMemsetAsync(e->d_m_count, 0, sizeof(u32) * 3, e->stream)); // m+l counts
  e->v2_dirty = true;
  // pre-mark every slot invalid (the legacy/sharded/clusterer commit reads
  // compacted proposals; the clusterer S kernel does not always-write)
  HIP_CHECK(hipMemsetAsync(e->d_slots, 0xFF, sizeof(Prop) * span, e->stream));

  hipEvent_t ev0, ev1;
  e->ev_pair(ev0, ev1);
  HIP_CHECK(hipEventRecord(ev0, e->stream));

  if (!e->clusterer && e->k > kMaxDenseK) {
    // hash gain tiers; the u16 shadow holds truncated labels above 65536
    const u32 fallback = balance_fallback(e);
    if (e->k <= 65536) {
      phase_a_hash_tiers<uint16_t>(e, e->d_labels16, pos_lo, pos_hi, chunk_base, iseed, fallback);
    } else {
      phase_a_hash_tiers<u32>(e, e->d_labels, pos_lo, pos_hi, chunk_base, iseed, fallback);
    }
  } else if (!e->clusterer) {
    const u32 fallback = balance_fallback(e);
    const u32 mode = static_cast<u32>(e->balance);
    if (e->k <= 256) {
      phase_a_dense_tiers<uint8_t>(
          e, e->d_labels8, pos_lo, pos_hi, chunk_base, iseed, mode, fallback, 0u, nullptr,
          kLPrepScan
      );
    } else {
      phase_a_dense_tiers<uint16_t>(
          e, e->d_labels16, pos_lo, pos_hi, chunk_base, iseed, mode, fallback, 0u, nullptr,
          kLPrepScan
      );
    }
  } else {
    // clustering: hash-based gain maps, favored-cluster tracking
    launch_build_lists(e, pos_lo, pos_hi, iseed, kClusterMidDeg, kClusterM2Deg, nullptr);
    hipLaunchKernelGGL(
        k_phase_s_c, dim3(ceil_div(static_cast<u64>(ceil_div(span, 4)) * kWave, threads)),
        dim3(threads), 0, e->stream, pos_lo, pos_hi, chunk_base, e->n, iseed, max_degree,
        e->maxw_uniform, e->d_xadj, e->d_adjncy, e->d_vwgt, e->d_adjwgt, e->d_labels, e->d_weights,
        e->d_comm, e->d_active, e->d_unit_active, e->d_favored, e->d_slots
    );
    LAUNCH_CHECK();
    {
      const size_t lds = static_cast<size_t>(threads / kWave) * 2 * kHashSlots * sizeof(u32);
      auto *kern = e->has_adjwgt ? k_phase_m_c<false> : k_phase_m_c<true>;
      hipLaunchKernelGGL(
          kern, dim3(4096), dim3(threads), lds, e->stream, pos_lo, chunk_base, iseed,
          e->maxw_uniform, e->d_xadj, e->d_adjncy, e->d_adjwgt, e->d_vwgt, e->d_labels,
          e->d_weights, e->d_comm, e->d_m_list, e->d_m_count, e->d_favored, e->d_slots
      );
      LAUNCH_CHECK();
      auto *kern2 = e->has_adjwgt ? k_phase_m2_c<false> : k_phase_m2_c<true>;
      hipLaunchKernelGGL(
          kern2, dim3(1024), dim3(threads), 0, e->stream, pos_lo, chunk_base, iseed,
          e->maxw_uniform, e->d_xadj, e->d_adjncy, e->d_adjwgt, e->d_vwgt, e->d_labels,
          e->d_weights, e->d_comm, e->d_m2_list, e->d_m2_count, e->d_favored, e->d_slots
      );
      LAUNCH_CHECK();
    }
    {
      hipLaunchKernelGGL(
          k_l_prep_c, dim3(1), dim3(1024), 0, e->stream, e->d_l_list, e->d_l_count, e->d_xadj,
          e->l_cap, e->d_l_off, e->d_l_hoff, e->d_l_hbits, e->d_l_ccnt, e->d_l_hacc
      );
      LAUNCH_CHECK();
      auto *kern = e->has_adjwgt ? k_phase_l_acc_c<false> : k_phase_l_acc_c<true>;
      l_pool_batches(e, [&](u32 lo, u32 hi) {
        hipLaunchKernelGGL(
            kern, dim3(2048), dim3(256), 0, e->stream, e->d_xadj, e->d_adjncy, e->d_adjwgt,
            e->d_labels, e->d_l_list, lo, hi, e->d_l_off, e->d_l_hoff, e->d_l_hbits,
            e->d_pool_keys, e->d_pool_vals, e->d_l_clist, e->d_l_ccnt
        );
        LAUNCH_CHECK();
        hipLaunchKernelGGL(
            k_phase_l_sel_c, dim3(2048), dim3(256), 0, e->stream, pos_lo, chunk_base, iseed,
            e->n, e->maxw_uniform, e->d_vwgt, e->d_labels, e->d_weights, e->d_l_list, lo, hi,
            e->d_l_hoff, e->d_l_hbits, e->d_pool_keys, e->d_pool_vals, e->d_l_clist,
            e->d_l_ccnt, e->d_comm, e->d_favored, e->d_slots
        );
        LAUNCH_CHECK();
      });
    }
  }
  // compact valid slots in position order (stable select)
  {
    size_t tb = e->select_temp_bytes;
    HIP_CHECK(rocprim::select(
        e->d_select_temp, tb, e->d_slots, out, e->d_prop_count, span, PropValid(), e->stream
    ));
  }
  HIP_CHECK(hipEventRecord(ev1, e->stream));

  HIP_CHECK(
      hipMemcpyAsync(e->h_count, e->d_prop_count, sizeof(u32), hipMemcpyDeviceToHost, e->stream)
  );
  sync_spin(e);
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
  e->phase_a_ms += ms;

  if (*e->h_count > cap) {
    fprintf(stderr, "kaminpar_amd: proposal buffer overflow (%u > %u)\n", *e->h_count, cap);
    return -1;
  }
  return static_cast<i64>(*e->h_count);
}

i64 kmp_lp_commit(kmp_lp_t *e, int iter, u32 chunk, const void *d_props, u32 count) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  const u64 iseed = iter_seed_of(e->seed, iter);
  const u32 threads = 256;
  const u32 chunk_lo = chunk * e->C;
  const u32 chunk_hi = chunk_lo + e->C > e->P ? e->P : chunk_lo + e->C;
  const bool big_k = e->clusterer; // cluster space = n

  hipEvent_t cev0, cev1;
  e->ev_pair(cev0, cev1);
  HIP_CHECK(hipEventRecord(cev0, e->stream));
  HIP_CHECK(hipMemcpyAsync(&e->h_moves[0], e->d_moves, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, e->stream));
  if (big_k) {
    HIP_CHECK(hipMemcpyAsync(&e->h_moves[2], e->d_emptied, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, e->stream));
  }

  const Prop *props = static_cast<const Prop *>(d_props);
  u32 *order = nullptr;
  u32 *sto = nullptr;

  if (count > 0) {
    const u32 grid = ceil_div(count, threads);
    hipLaunchKernelGGL(
        k_make_keys, dim3(grid), dim3(threads), 0, e->stream, props, count, e->d_sort_keys[0],
        e->d_sort_vals[0]
    );
    LAUNCH_CHECK();
    rocprim::double_buffer<u32> keys(e->d_sort_keys[0], e->d_sort_keys[1]);
    rocprim::double_buffer<u32> vals(e->d_sort_vals[0], e->d_sort_vals[1]);
    size_t tb = e->sort_temp_bytes;
    HIP_CHECK(rocprim::radix_sort_pairs(e->d_sort_temp, tb, keys, vals, count, 0, 32, e->stream));
    order = vals.current();
    sto = keys.current();

    hipLaunchKernelGGL(
        k_extract_w, dim3(grid), dim3(threads), 0, e->stream, order, props, count, e->d_sw
    );
    LAUNCH_CHECK();
    size_t sb = e->scan_temp_bytes;
    HIP_CHECK(rocprim::inclusive_scan_by_key(
        e->d_scan_temp, sb, sto, e->d_sw, e->d_pw, count, rocprim::plus<i64>(),
        rocprim::equal_to<u32>(), e->stream
    ));
    hipLaunchKernelGGL(
        k_seg_bounds, dim3(grid), dim3(threads), 0, e->stream, sto, count, e->d_seg_begin,
        e->d_seg_end
    );
    LAUNCH_CHECK();
    hipLaunchKernelGGL(
        k_seg_len_heads, dim3(grid), dim3(threads), 0, e->stream, sto, count, e->d_seg_begin,
        e->d_seg_end, e->d_prefix_len
    );
    LAUNCH_CHECK();

    // greatest-fixpoint rollback (kaminpar-dist lp_refiner.cc:296-333).
    // Two rounds per host sync; the second round's changed flag decides.
    const u32 kgrid = big_k ? 0 : ceil_div(e->k, threads);
    while (true) {
      for (int half = 0; half < 2; ++half) {
        if (big_k) {
          hipLaunchKernelGGL(
              k_dep_reset_touched, dim3(grid), dim3(threads), 0, e->stream, props, count,
              e->d_labels, e->d_dep
          );
          LAUNCH_CHECK();
          hipLaunchKernelGGL(
              k_dep_direct, dim3(grid), dim3(threads), 0, e->stream, order, props, sto, count,
              e->d_seg_begin, e->d_prefix_len, e->d_labels, e->d_dep
          );
          LAUNCH_CHECK();
          HIP_CHECK(hipMemsetAsync(e->d_changed, 0, sizeof(int), e->stream));
          hipLaunchKernelGGL(
              k_cutoff_heads, dim3(grid), dim3(threads), 0, e->stream, sto, count, e->d_seg_begin,
              e->d_seg_end, e->d_prefix_len, e->d_pw, e->d_weights, e->maxw_uniform, e->d_dep,
              e->d_changed
          );
          LAUNCH_CHECK();
        } else {
          hipLaunchKernelGGL(
              k_dep_reset_all, dim3(kgrid), dim3(threads), 0, e->stream, e->k, e->d_dep
          );
          LAUNCH_CHECK();
          if (e->k > kMaxDenseK) {
            // k_dep's k-sized LDS histogram does not fit: global atomics
            // (integer sums, any order)
            hipLaunchKernelGGL(
                k_dep_direct, dim3(grid), dim3(threads), 0, e->stream, order, props, sto, count,
                e->d_seg_begin, e->d_prefix_len, e->d_labels, e->d_dep
            );
          } else {
            hipLaunchKernelGGL(
                k_dep, dim3(grid > 2048 ? 2048 : grid), dim3(threads),
                static_cast<size_t>(e->k) * sizeof(unsigned long long), e->stream, order, props,
                sto, count, e->k, e->d_seg_begin, e->d_prefix_len, e->d_labels, e->d_dep
            );
          }
          LAUNCH_CHECK();
          HIP_CHECK(hipMemsetAsync(e->d_changed, 0, sizeof(int), e->stream));
          hipLaunchKernelGGL(
              k_cutoff, dim3(kgrid), dim3(threads), 0, e->stream, e->k, e->d_seg_begin,
              e->d_seg_end, e->d_prefix_len, e->d_pw, e->d_weights, e->d_maxw, e->d_dep,
              e->d_changed
          );
          LAUNCH_CHECK();
        }
      }
      HIP_CHECK(
          hipMemcpyAsync(e->h_changed, e->d_changed, sizeof(int), hipMemcpyDeviceToHost, e->stream)
      );
      sync_spin(e);
      if (!*e->h_changed) {
        break;
      }
    }

    if (big_k) {
      hipLaunchKernelGGL(
          k_weights_update_big, dim3(grid), dim3(threads), 0, e->stream, order, props, sto, count,
          e->d_seg_begin, e->d_prefix_len, e->d_pw, e->d_labels, e->d_dep, e->d_weights
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_emptied_count, dim3(grid), dim3(threads), 0, e->stream, order, props, sto, count,
          e->d_seg_begin, e->d_prefix_len, e->d_labels, e->d_weights, e->d_eflag, e->d_emptied
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_emptied_reset, dim3(grid), dim3(threads), 0, e->stream, order, props, count,
          e->d_labels, e->d_eflag
      );
      LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL(
          k_weights_update, dim3(ceil_div(e->k, threads)), dim3(threads), 0, e->stream, e->k,
          e->d_seg_begin, e->d_seg_end, e->d_prefix_len, e->d_pw, e->d_dep, e->d_weights
      );
      LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(
        k_apply, dim3(grid), dim3(threads), 0, e->stream, order, props, sto, count, e->d_seg_begin,
        e->d_prefix_len, e->d_labels, big_k ? nullptr : e->d_labels16,
        (big_k || e->k > 256) ? nullptr : e->d_labels8, e->d_admitted_flags,
        e->d_moves
    );
    LAUNCH_CHECK();
  }

  // clear active for the WHOLE chunk's processed set (identical on all
  // ranks) and tally scanned arcs
  hipLaunchKernelGGL(
      k_clear_active, dim3(ceil_div(chunk_hi - chunk_lo, threads)), dim3(threads), 0, e->stream,
      chunk_lo, chunk_hi, e->n, iseed, 0xFFFFFFFFu, e->d_xadj, e->d_active, e->d_unit_active,
      e->d_arcs
  );
  LAUNCH_CHECK();
  if (count > 0) {
    hipLaunchKernelGGL(
        k_activate, dim3(ceil_div(static_cast<u64>(count) * kWave, threads)), dim3(threads), 0,
        e->stream, order, e->d_admitted_flags, props, count, e->d_xadj, e->d_adjncy, e->d_active,
        e->d_unit_active
    );
    LAUNCH_CHECK();
    hipLaunchKernelGGL(
        k_reset_segs, dim3(ceil_div(count, threads)), dim3(threads), 0, e->stream, props, count,
        e->d_seg_begin, e->d_seg_end, e->d_prefix_len
    );
    LAUNCH_CHECK();
  }

  HIP_CHECK(hipEventRecord(cev1, e->stream));
  HIP_CHECK(hipMemcpyAsync(&e->h_moves[1], e->d_moves, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, e->stream));
  if (big_k) {
    HIP_CHECK(hipMemcpyAsync(&e->h_moves[3], e->d_emptied, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, e->stream));
  }
  sync_spin(e);
  float cms = 0;
  HIP_CHECK(hipEventElapsedTime(&cms, cev0, cev1));
  e->commit_ms += cms;
  e->last_emptied = big_k ? (e->h_moves[3] - e->h_moves[2]) : 0;
  return static_cast<i64>(e->h_moves[1] - e->h_moves[0]);
}

// ---- sharded commit ABI (multi-GPU; see kernel block comment) ----
// d_* arguments are DEVICE pointers (e.g. torch tensors' data_ptr()).

int kmp_lp_shard_begin(
    kmp_lp_t *e, u32 c_lo, u32 c_hi, const void *d_props, u32 count,
    long long *d_dep_out /* k+1 i64, pre-zeroed by caller */
) {
  const u32 threads = 256;
  const u32 rows = 1024;
  const u32 T = (count + 63) >> 6;
  const u32 tpw = (T + rows - 1) / rows;
  const Prop *props = static_cast<const Prop *>(d_props);
  const size_t lds_h = static_cast<size_t>(threads / kWave) * e->k * sizeof(u32);
  // stage the (host-known) count into the device scalar the kernels read
  // (kernel arg by value: no pinned-buffer reuse races)
  hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, e->stream, e->d_prop_count, count);
  LAUNCH_CHECK();
  // reset local arr slot
  HIP_CHECK(hipMemsetAsync(e->d_dep, 0, sizeof(unsigned long long) * 2 * e->k, e->stream));
  e->v2_dirty = true;
  if (count > 0) {
    hipLaunchKernelGGL(
        k_hist_props, dim3(rows / 4), dim3(threads), lds_h, e->stream, e->d_prop_count, e->k,
        rows, tpw, c_lo, c_hi, props, e->d_histT
    );
    LAUNCH_CHECK();
  } else {
    HIP_CHECK(hipMemsetAsync(e->d_histT, 0, sizeof(u32) * e->k * rows, e->stream));
  }
  hipLaunchKernelGGL(
      k_scan_small<true>, dim3(1), dim3(threads), 0, e->stream, e->k, rows, e->d_histT,
      e->d_offT, e->d_seg_off, e->d_prefix_len, e->d_dep, e->d_changed
  );
  LAUNCH_CHECK();
  if (count > 0) {
    const size_t lds_sc = lds_h + static_cast<size_t>(2 * e->k) * sizeof(unsigned long long);
    hipLaunchKernelGGL(
        k_scatter_props, dim3(rows / 4), dim3(threads), lds_sc, e->stream, e->d_prop_count,
        e->k, rows, tpw, c_lo, c_hi, props, e->d_offT, e->d_labels, e->d_s_u, e->d_s_w,
        e->d_s_r, e->d_s_to, e->d_s_b, d_dep_out,
        reinterpret_cast<unsigned long long *>(e->d_dep) + e->k
    );
    LAUNCH_CHECK();
    if (e->has_vwgt) {
      hipLaunchKernelGGL(
          k_shard_pw, dim3(64), dim3(threads), 0, e->stream, e->k, c_lo, c_hi, e->d_seg_off,
          e->d_prefix_len, e->d_s_w, e->d_pw
      );
      LAUNCH_CHECK();
    }
  }
  if (e->own_stream == nullptr) {
    HIP_CHECK(hipStreamSynchronize(e->stream)); // cross-stream caller
  }
  return 0;
}

int kmp_lp_shard_round(
    kmp_lp_t *e, u32 c_lo, u32 c_hi, const long long *d_dep_global,
    long long *d_delta_out /* k+1 */
) {
  hipLaunchKernelGGL(
      k_shard_round, dim3(1), dim3(256), 0, e->stream, e->k, c_lo, c_hi,
      static_cast<u32>(e->has_vwgt ? 1 : 0), e->d_seg_off, e->d_prefix_len,
      reinterpret_cast<unsigned long long *>(e->d_dep) + e->k, d_dep_global, e->d_s_w,
      e->d_s_b, e->d_pw, e->d_weights, e->d_maxw, d_delta_out
  );
  LAUNCH_CHECK();
  if (e->own_stream == nullptr) {
    HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

int kmp_lp_shard_finish_meta(
    kmp_lp_t *e, u32 c_lo, u32 c_hi,
    unsigned long long *d_cutoff_out /* k i64, pre-zeroed */,
    long long *d_arr_out /* k i64, pre-zeroed */
) {
  hipLaunchKernelGGL(
      k_shard_finish_meta, dim3(ceil_div(e->k, 256u)), dim3(256), 0, e->stream, e->k, c_lo,
      c_hi, e->d_seg_off, e->d_prefix_len,
      reinterpret_cast<unsigned long long *>(e->d_dep) + e->k, e->d_s_r, d_cutoff_out,
      d_arr_out
  );
  LAUNCH_CHECK();
  if (e->own_stream == nullptr) {
    HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

i64 kmp_lp_shard_apply(
    kmp_lp_t *e, int iter, u32 chunk, const void *d_props, u32 count,
    const unsigned long long *d_cutoff_all, const long long *d_arr_all,
    const long long *d_dep_global
) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  const u32 threads = 256;
  const u64 iseed = iter_seed_of(e->seed, iter);
  const u32 chunk_lo = chunk * e->C;
  const u32 chunk_hi = chunk_lo + e->C > e->P ? e->P : chunk_lo + e->C;
  const Prop *props = static_cast<const Prop *>(d_props);
  hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, e->stream, e->d_prop_count, count);
  LAUNCH_CHECK();
  {
    const u32 span = count > e->k ? count : e->k;
    hipLaunchKernelGGL(
        k_shard_apply, dim3(ceil_div(span, threads)), dim3(threads), 0, e->stream,
        e->d_prop_count, e->k, props, d_cutoff_all, d_arr_all, d_dep_global, e->d_weights,
        e->d_labels, e->d_labels16, e->k <= 256 ? e->d_labels8 : nullptr, e->d_admitted_flags,
        e->d_moves
    );
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(
      k_clear_active, dim3(ceil_div(chunk_hi - chunk_lo, threads)), dim3(threads), 0, e->stream,
      chunk_lo, chunk_hi, e->n, iseed, 0xFFFFFFFFu, e->d_xadj, e->d_active, e->d_unit_active,
      e->d_arcs
  );
  LAUNCH_CHECK();
  if (count > 0) {
    hipLaunchKernelGGL(
        k_activate, dim3(ceil_div(static_cast<u64>(count) * kWave, threads)), dim3(threads), 0,
        e->stream, static_cast<const u32 *>(nullptr), e->d_admitted_flags, props, count,
        e->d_xadj, e->d_adjncy, e->d_active, e->d_unit_active
    );
    LAUNCH_CHECK();
  }
  // no per-call moves readback: callers poll the cumulative counter per
  // sweep via kmp_lp_get_stats (one sync per sweep instead of per chunk)
  return 0;
}

// partition == nullptr: the labels stay on the device.
static i64 refine_end_impl(kmp_lp_t *e, u32 *partition, kmp_lp_stats_t *stats, bool counted) {
  HIP_CHECK(hipMemsetAsync(e->d_cut, 0, sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(
      k_edge_cut, dim3(32768), dim3(256), 0, e->stream, e->n, e->d_xadj, e->d_adjncy, e->d_adjwgt,
      e->d_labels, e->d_cut
  );
  LAUNCH_CHECK();
  unsigned long long cut2 = 0, arcs = 0, moves = 0;
  HIP_CHECK(hipMemcpyAsync(&cut2, e->d_cut, sizeof(cut2), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipMemcpyAsync(&arcs, e->d_arcs, sizeof(arcs), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipMemcpyAsync(&moves, e->d_moves, sizeof(moves), hipMemcpyDeviceToHost, e->stream));
  if (partition != nullptr) {
    const size_t bytes = sizeof(u32) * e->n;
    HIP_CHECK(hipMemcpy(partition, e->d_labels, counted ? label_traffic(bytes) : bytes,
                        hipMemcpyDeviceToHost));
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));

  if (stats) {
    stats->arcs_scanned = arcs;
    stats->moves = moves;
    stats->phase_a_ns = static_cast<u64>(e->phase_a_ms * 1e6);
    stats->total_ns = static_cast<u64>(e->commit_ms * 1e6); // commit-region time
    stats->num_clusters = 0;
    stats->edge_cut = static_cast<i64>(cut2 / 2);
  }
  return static_cast<i64>(cut2 / 2);
}

i64 kmp_lp_refine_end(kmp_lp_t *e, u32 *partition, kmp_lp_stats_t *stats) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  return refine_end_impl(e, partition, stats, false);
}

// Reset the engine to the initial partition of the last refine_begin, fully
// on-device (no host transfers): labels, weights, active flags, counters.
int kmp_lp_reset(kmp_lp_t *e) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  HIP_CHECK(hipMemcpyAsync(
      e->d_labels, e->d_labels0, sizeof(u32) * e->n, hipMemcpyDeviceToDevice, e->stream
  ));
  HIP_CHECK(hipMemsetAsync(e->d_active, 1, e->n, e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_unit_active, 1, kmp::num_units(e->n), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_arcs, 0, sizeof(unsigned long long), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_moves, 0, sizeof(unsigned long long), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_weights, 0, sizeof(i64) * e->k, e->stream));
  v2_clear_train_state(e);
  e->phase_a_ms = 0.0;
  e->commit_ms = 0.0;
  e->ev_used = 0;
  {
    const u32 threads = 256;
    hipLaunchKernelGGL(
        k_sync_labels16, dim3(ceil_div(e->n, threads)), dim3(threads), 0, e->stream, e->n,
        e->d_labels, e->d_labels16, e->d_labels8
    );
    LAUNCH_CHECK();
    launch_init_weights(e);
  }
  return 0;
}

// Run the LP sweeps on the current device state (the timed region: all data
// resident in HBM; the v2 path does ONE host sync per sweep, the legacy
// path syncs per chunk). Returns total committed moves.
i64 kmp_lp_run_sweeps(kmp_lp_t *e, int iters) {
  e->label_kind = kmp_lp_t::kLabelsNone; // the callers that keep a kind set it afterwards
  if (v2_eligible(e)) {
    return run_sweeps_v2(e, iters);
  }
  u64 total_moves = 0;
  for (int iter = 0; iter < iters; ++iter) {
    u64 sweep_moves = 0;
    for (u32 chunk = 0; chunk < kmp::kNumChunks; ++chunk) {
      const u32 pos_lo = chunk * e->C;
      const u32 pos_hi = pos_lo + e->C > e->P ? e->P : pos_lo + e->C;
      if (pos_lo >= pos_hi) {
        continue;
      }
      const i64 cnt = kmp_lp_phase_a(e, iter, chunk, pos_lo, pos_hi, e->d_props, e->C);
      if (cnt < 0) {
        return -1;
      }
      const i64 mv = kmp_lp_commit(e, iter, chunk, e->d_props, static_cast<u32>(cnt));
      if (mv < 0) {
        return -1;
      }
      sweep_moves += mv;
    }
    total_moves += sweep_moves;
    if (sweep_moves == 0) {
      break;
    }
  }
  return static_cast<i64>(total_moves);
}

// Light stats (no cut kernel, no label download).
int kmp_lp_get_stats(kmp_lp_t *e, kmp_lp_stats_t *stats) {
  unsigned long long arcs = 0, moves = 0;
  HIP_CHECK(hipMemcpyAsync(&arcs, e->d_arcs, sizeof(arcs), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipMemcpyAsync(&moves, e->d_moves, sizeof(moves), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  stats->arcs_scanned = arcs;
  stats->moves = moves;
  stats->phase_a_ns = static_cast<u64>(e->phase_a_ms * 1e6);
  stats->total_ns = static_cast<u64>(e->commit_ms * 1e6);
  stats->num_clusters = 0;
  stats->edge_cut = -1;
  return 0;
}

static i64 refine_impl(
    kmp_lp_t *e, u32 k, const i64 *max_block_weights, u32 *partition, u64 seed, int iters,
    kmp_lp_stats_t *stats, bool counted
) {
  if (refine_begin_impl(e, k, max_block_weights, partition, seed, counted) != 0) {
    return -1;
  }
  if (kmp_lp_run_sweeps(e, iters) < 0) {
    return -1;
  }
  return refine_end_impl(e, partition, stats, counted);
}

i64 kmp_lp_refine(
    kmp_lp_t *e,
    u32 k,
    const i64 *max_block_weights,
    u32 *partition,
    u64 seed,
    int iters,
    kmp_lp_stats_t *stats
) {
  if (partition == nullptr && resident_partition_ok(e, k, "refine") != 0) {
    e->label_kind = kmp_lp_t::kLabelsNone;
    return -1;
  }
  e->label_kind = kmp_lp_t::kLabelsNone;
  const i64 cut = refine_impl(e, k, max_block_weights, partition, seed, iters, stats, true);
  if (cut >= 0) {
    // the sweeps only ever write labels below k, shadows included; above
    // 65536 the u16 shadow holds truncated values and is no copy
    e->label_kind = kmp_lp_t::kLabelsPartition;
    e->label_k = k;
    e->shadows_ok = k <= 65536;
  }
  return cut;
}

// Overload-balancer mode (the role of the reference's OVERLOAD_BALANCER
// bracketing LP in the default refiner chain, presets.cc:332-338): same
// deterministic schedule and commit as kmp_lp_refine, but a vertex whose
// block exceeds its cap loses "stay" as a candidate, so overloaded blocks
// shed their boundary vertices to the best admissible targets even at
// negative gain (interior vertices follow over subsequent sweeps as the
// boundary peels). Feasible partitions are left untouched up to normal LP
// moves. Returns the resulting edge cut, or -1.
i64 kmp_lp_balance(
    kmp_lp_t *e,
    u32 k,
    const i64 *max_block_weights,
    u32 *partition,
    u64 seed,
    int iters,
    kmp_lp_stats_t *stats
) {
  // Isolated vertices have no LP candidates and can never move through the
  // sweeps: assign those sitting in over-cap blocks to the lightest block
  // with room first (deterministic; zero cut impact -- they have no edges).
  // The blocks are kept ordered by (weight, id), so "lightest with room,
  // lowest id on ties" is the first fitting entry: a linear scan per vertex
  // measured 13.1 s at R-MAT scale 20, k = 65536.
  if (k > kMaxDenseK && k <= KMP_LP_MAX_K &&
      labels_below_k(partition, e->n, k, "balance") != 0) {
    e->label_kind = kmp_lp_t::kLabelsNone;
    return -1;
  }
  e->balance_host_ns[0] = e->balance_host_ns[1] = 0;
  if (!e->isolated.empty()) {
    if (kmp_lp_refine_begin(e, k, max_block_weights, partition, seed) != 0) {
      return -1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<i64> w(k);
    HIP_CHECK(hipMemcpyAsync(w.data(), e->d_weights, sizeof(i64) * k,
                             hipMemcpyDeviceToHost, e->stream));
    sync_spin(e);
    std::set<std::pair<i64, u32>> by_weight;
    for (u32 c = 0; c < k; ++c) {
      by_weight.insert({w[c], c});
    }
    for (size_t i = 0; i < e->isolated.size(); ++i) {
      const u32 u = e->isolated[i];
      const i32 uw = e->iso_weights[i];
      const u32 b = partition[u];
      if (w[b] <= max_block_weights[b]) {
        continue;
      }
      u32 t = b;
      for (const auto &wc : by_weight) {
        const u32 c = wc.second;
        if (c != b && wc.first + uw <= max_block_weights[c]) {
          t = c;
          break;
        }
      }
      if (t != b) {
        by_weight.erase({w[b], b});
        by_weight.erase({w[t], t});
        w[b] -= uw;
        w[t] += uw;
        by_weight.insert({w[b], b});
        by_weight.insert({w[t], t});
        partition[u] = t;
      }
    }
    e->balance_host_ns[0] = static_cast<u64>(
        std::chrono::duration_cast<std::chrono::nanoseconds>(
            std::chrono::steady_clock::now() - t0).count());
  }
  e->label_kind = kmp_lp_t::kLabelsNone;
  e->balance = 1;
  const i64 cut = refine_impl(e, k, max_block_weights, partition, seed, iters, stats, false);
  e->balance = 0;
  return cut;
}

void kmp_lp_balance_host_ns(const kmp_lp_t *e, uint64_t out[2]) {
  out[0] = e->balance_host_ns[0];
  out[1] = e->balance_host_ns[1];
}

// Clusterer::set_communities (coarsening/clusterer.h:35,
// lp_clusterer.cc:61-66,193-194): when set, clustering never merges across
// community boundaries (cluster ids are vertex ids, so the per-vertex array
// indexes both sides of the check). Pass null to clear.
int kmp_lp_set_communities(kmp_lp_t *e, const u32 *communities) {
  if (e->d_comm) {
    HIP_CHECK(hipFree(e->d_comm));
    e->d_comm = nullptr;
  }
  e->iso_comm.clear();
  e->comm_k = 0;
  if (communities != nullptr) {
    HIP_CHECK(hipMalloc(&e->d_comm, sizeof(u32) * e->n));
    HIP_CHECK(
        hipMemcpy(e->d_comm, communities, sizeof(u32) * e->n, hipMemcpyHostToDevice)
    );
    e->iso_comm.reserve(e->isolated.size());
    for (const u32 u : e->isolated) {
      e->iso_comm.push_back(communities[u]);
    }
    u32 top = 0;
    for (u32 u = 0; u < e->n; ++u) {
      top = communities[u] > top ? communities[u] : top;
    }
    e->comm_k = static_cast<u64>(top) + 1;
  }
  return 0;
}

// The resident partition becomes the communities, device to device; the
// chain over the isolated vertices gets theirs through a gather of
// e->isolated.size() entries (no label traffic: nothing n-sized moves).
static void *vc_scratch(kmp_lp_t *e, size_t bytes) {
  if (bytes > e->vc_scratch_bytes) {
    if (e->d_vc_scratch != nullptr) {
      HIP_CHECK(hipFree(e->d_vc_scratch));
      e->d_vc_scratch = nullptr;
    }
    HIP_CHECK(hipMalloc(&e->d_vc_scratch, bytes));
    e->vc_scratch_bytes = bytes;
  }
  return e->d_vc_scratch;
}

int kmp_lp_set_communities_resident(kmp_lp_t *e) {
  if (e->label_kind != kmp_lp_t::kLabelsPartition) {
    fprintf(stderr, "kaminpar_amd: set_communities_resident: the engine holds no resident "
                    "partition\n");
    return -1;
  }
  if (e->d_comm == nullptr) {
    HIP_CHECK(hipMalloc(&e->d_comm, sizeof(u32) * e->n));
  }
  HIP_CHECK(hipMemcpyAsync(e->d_comm, e->d_labels, sizeof(u32) * e->n, hipMemcpyDeviceToDevice,
                           e->stream));
  const u32 icount = static_cast<u32>(e->isolated.size());
  e->iso_comm.assign(icount, 0);
  if (icount > 0) {
    u32 *d_ids = static_cast<u32 *>(vc_scratch(e, sizeof(u32) * icount * 2));
    HIP_CHECK(hipMemcpyAsync(d_ids, e->isolated.data(), sizeof(u32) * icount,
                             hipMemcpyHostToDevice, e->stream));
    kmp_vcycle::gather(d_ids, icount, e->d_comm, d_ids + icount, e->stream);
    HIP_CHECK(hipMemcpyAsync(e->iso_comm.data(), d_ids + icount, sizeof(u32) * icount,
                             hipMemcpyDeviceToHost, e->stream));
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->comm_k = e->label_k;
  return 0;
}

// Underload-balancer mode (the reference's UNDERLOAD_BALANCER closing the
// default refiner chain, presets.cc:332-338; semantics restated from
// refinement/balancer/underload_balancer.cc): fill blocks below their
// minimum weight with best-gain admissible vertices under the deterministic
// chunk schedule; admission is serial in rank order with BOTH per-block
// minima and maxima re-checked per move (the batch analogue of the
// reference's locked per-move checks). No-op when minima are satisfied.
i64 kmp_lp_underload(
    kmp_lp_t *e,
    u32 k,
    const i64 *max_block_weights,
    const i64 *min_block_weights,
    u32 *partition,
    u64 seed,
    int iters,
    kmp_lp_stats_t *stats
) {
  if (dense_k_ok(k, "underload") != 0) {
    return -1;
  }
  if (kmp_lp_refine_begin(e, k, max_block_weights, partition, seed) != 0) {
    return -1;
  }
  if (e->d_minw) {
    HIP_CHECK(hipFree(e->d_minw));
    e->d_minw = nullptr;
  }
  HIP_CHECK(hipMalloc(&e->d_minw, sizeof(i64) * k));
  HIP_CHECK(hipMemcpy(e->d_minw, min_block_weights, sizeof(i64) * k, hipMemcpyHostToDevice));
  e->balance = 2;
  const u32 threads = 256;
  HIP_CHECK(hipMemcpyAsync(&e->h_moves[0], e->d_moves, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, e->stream));
  sync_spin(e);
  unsigned long long last = e->h_moves[0];
  for (int iter = 0; iter < iters; ++iter) {
    for (u32 chunk = 0; chunk < kmp::kNumChunks; ++chunk) {
      const u32 pos_lo = chunk * e->C;
      const u32 pos_hi = pos_lo + e->C > e->P ? e->P : pos_lo + e->C;
      if (pos_lo >= pos_hi) {
        continue;
      }
      const i64 cnt = kmp_lp_phase_a(e, iter, chunk, pos_lo, pos_hi, e->d_props, e->C);
      if (cnt < 0) {
        e->balance = 0;
        return -1;
      }
      const u64 iseed = iter_seed_of(e->seed, iter);
      hipLaunchKernelGGL(
          k_commit_underload, dim3(1), dim3(64), 0, e->stream, e->d_props, e->d_prop_count,
          e->d_maxw, e->d_minw, e->d_weights, e->d_labels, e->d_labels16,
          k <= 256 ? e->d_labels8 : nullptr, e->d_admitted_flags, e->d_moves
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_clear_active, dim3(ceil_div(pos_hi - pos_lo, threads)), dim3(threads), 0, e->stream,
          pos_lo, pos_hi, e->n, iseed, 0xFFFFFFFFu, e->d_xadj, e->d_active, e->d_unit_active,
          e->d_arcs
      );
      LAUNCH_CHECK();
      if (cnt > 0) {
        hipLaunchKernelGGL(
            k_activate, dim3(ceil_div(static_cast<u64>(cnt) * kWave, threads)), dim3(threads), 0,
            e->stream, static_cast<const u32 *>(nullptr), e->d_admitted_flags, e->d_props,
            static_cast<u32>(cnt), e->d_xadj, e->d_adjncy, e->d_active, e->d_unit_active
        );
        LAUNCH_CHECK();
      }
    }
    HIP_CHECK(hipMemcpyAsync(&e->h_moves[1], e->d_moves, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, e->stream));
    sync_spin(e);
    const unsigned long long cur = e->h_moves[1];
    const u64 sweep_moves = cur - last;
    last = cur;
    if (sweep_moves == 0) {
      break;
    }
  }
  e->balance = 0;
  return kmp_lp_refine_end(e, partition, stats);
}

i64 kmp_lp_cluster(
    kmp_lp_t *e, i64 max_cluster_weight, u32 desired_clusters, u32 *clustering, u64 seed,
    int iters, kmp_lp_stats_t *stats
) {
  const u32 n = e->n;
  const u32 threads = 256;
  e->label_kind = kmp_lp_t::kLabelsNone;
  e->k = n;
  e->seed = seed;
  e->clusterer = true;
  e->maxw_uniform = max_cluster_weight;
  e->phase_a_ms = 0.0;
  e->commit_ms = 0.0;
  e->ev_used = 0;

  engine_free_k_buffers(e);
  engine_alloc_k_buffers(e, n);
  if (e->d_weights) {
    HIP_CHECK(hipFree(e->d_weights));
    e->d_weights = nullptr;
  }
  HIP_CHECK(hipMalloc(&e->d_weights, sizeof(i64) * n));
  if (!e->d_favored) {
    HIP_CHECK(hipMalloc(&e->d_favored, sizeof(u32) * n));
    HIP_CHECK(hipMalloc(&e->d_eflag, n));
    HIP_CHECK(hipMemset(e->d_eflag, 0, n));
    HIP_CHECK(hipMalloc(&e->d_emptied, sizeof(unsigned long long)));
    engine_ensure_l_pool(e);
    // two-hop buffers + temps
    HIP_CHECK(hipMalloc(&e->d_cand, sizeof(u64) * n));
    HIP_CHECK(hipMalloc(&e->d_cand2, sizeof(u64) * n));
    HIP_CHECK(hipMalloc(&e->d_cfav, sizeof(u32) * n));
    HIP_CHECK(hipMalloc(&e->d_crank, sizeof(u32) * n));
    HIP_CHECK(hipMalloc(&e->d_cones, sizeof(u32) * n));
    HIP_CHECK(rocprim::select(
        nullptr, e->cand_select_temp_bytes, e->d_cand, e->d_cand2, e->d_prop_count, n, CandValid()
    ));
    HIP_CHECK(hipMalloc(&e->d_cand_select_temp, e->cand_select_temp_bytes));
    rocprim::double_buffer<u64> ckeys(e->d_cand2, e->d_cand);
    HIP_CHECK(rocprim::radix_sort_keys(nullptr, e->cand_sort_temp_bytes, ckeys, n));
    HIP_CHECK(hipMalloc(&e->d_cand_sort_temp, e->cand_sort_temp_bytes));
    HIP_CHECK(rocprim::inclusive_scan_by_key(
        nullptr, e->cand_scan_temp_bytes, e->d_cfav, e->d_cones, e->d_crank, n,
        rocprim::plus<u32>(), rocprim::equal_to<u32>()
    ));
    HIP_CHECK(hipMalloc(&e->d_cand_scan_temp, e->cand_scan_temp_bytes));
  }
  // the L list cap is the full chunk span for clustering (a refine run may
  // have shrunk l_cap for its dense-gains buffer)
  e->l_cap = e->C;
  if (e->d_l_off) {
    HIP_CHECK(hipFree(e->d_l_off));
  }
  HIP_CHECK(hipMalloc(&e->d_l_off, sizeof(u32) * (e->l_cap + 1)));
  HIP_CHECK(hipMemsetAsync(e->d_emptied, 0, sizeof(unsigned long long), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_arcs, 0, sizeof(unsigned long long), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_moves, 0, sizeof(unsigned long long), e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_active, 1, n, e->stream));
  HIP_CHECK(hipMemsetAsync(e->d_unit_active, 1, kmp::num_units(e->n), e->stream));

  const u32 ngrid = ceil_div(n, threads);
  hipLaunchKernelGGL(k_iota, dim3(ngrid), dim3(threads), 0, e->stream, n, e->d_labels);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_iota, dim3(ngrid), dim3(threads), 0, e->stream, n, e->d_favored);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(
      k_init_cluster_weights, dim3(ngrid), dim3(threads), 0, e->stream, n, e->d_vwgt, e->d_weights
  );
  LAUNCH_CHECK();
  HIP_CHECK(hipStreamSynchronize(e->stream));

  // ---- LP sweeps (driver: lp_clusterer.cc:89-109 + should_stop) ----
  u64 live = n;
  for (int iter = 0; iter < iters; ++iter) {
    u64 sweep_moves = 0;
    bool stopped = false;
    for (u32 chunk = 0; chunk < kmp::kNumChunks && !stopped; ++chunk) {
      const u32 pos_lo = chunk * e->C;
      const u32 pos_hi = pos_lo + e->C > e->P ? e->P : pos_lo + e->C;
      if (pos_lo >= pos_hi) {
        continue;
      }
      const i64 cnt = kmp_lp_phase_a(e, iter, chunk, pos_lo, pos_hi, e->d_props, e->C);
      if (cnt < 0) {
        return -1;
      }
      const i64 mv = kmp_lp_commit(e, iter, chunk, e->d_props, static_cast<u32>(cnt));
      if (mv < 0) {
        return -1;
      }
      sweep_moves += mv;
      live -= e->last_emptied;
      if (desired_clusters > 0 && live <= desired_clusters) {
        stopped = true;
      }
    }
    if (sweep_moves == 0) {
      break;
    }
  }

  // ---- isolated nodes + two-hop (default preset strategies;
  //      lp_clusterer.cc:112-162, oracle parity contract) ----
  const bool handle_two_hop = (1.0 - 1.0 * live / n) <= 0.5;
  if (handle_two_hop) {
    // isolated nodes, MATCH semantics: deterministic host chain (isolated
    // clusters stay singletons through LP, so their weights are the node
    // weights captured at engine creation)
    std::vector<u64> pairs;
    u32 pending = 0xFFFFFFFFu;
    size_t pending_i = 0;
    i64 pending_w = 0;
    for (size_t i = 0; i < e->isolated.size(); ++i) {
      const u32 cu = e->isolated[i];
      const i64 w = e->iso_weights[i];
      // communities are a hard constraint: chains break at boundaries
      // (keep in sync with the oracle twin)
      if (pending != 0xFFFFFFFFu && !e->iso_comm.empty() &&
          e->iso_comm[pending_i] != e->iso_comm[i]) {
        pending = cu;
        pending_i = i;
        pending_w = w;
        continue;
      }
      if (pending != 0xFFFFFFFFu && pending_w + w <= max_cluster_weight) {
        pairs.push_back((static_cast<u64>(pending) << 32) | cu);
        pending = 0xFFFFFFFFu;
      } else {
        pending = cu;
        pending_i = i;
        pending_w = w;
      }
    }
    if (!pairs.empty()) {
      HIP_CHECK(hipMemcpyAsync(
          e->d_cand, pairs.data(), sizeof(u64) * pairs.size(), hipMemcpyHostToDevice, e->stream
      ));
      hipLaunchKernelGGL(
          k_apply_pairs, dim3(ceil_div(pairs.size(), threads)), dim3(threads), 0, e->stream,
          e->d_cand, static_cast<u32>(pairs.size()), e->d_labels, e->d_weights
      );
      LAUNCH_CHECK();
      live -= pairs.size();
    }

    // two-hop matching (MATCH_THREADWISE single-chain semantics): collect
    // singleton candidates, sort by (favored, u), pair consecutive equals
    hipLaunchKernelGGL(
        k_twohop_cand, dim3(ngrid), dim3(threads), 0, e->stream, n, max_cluster_weight, e->d_xadj,
        e->d_vwgt, e->d_labels, e->d_weights, e->d_favored, e->d_cand
    );
    LAUNCH_CHECK();
    size_t stb = e->cand_select_temp_bytes;
    HIP_CHECK(rocprim::select(
        e->d_cand_select_temp, stb, e->d_cand, e->d_cand2, e->d_prop_count, n, CandValid(),
        e->stream
    ));
    u32 cand_count = 0;
    HIP_CHECK(hipMemcpyAsync(
        &cand_count, e->d_prop_count, sizeof(u32), hipMemcpyDeviceToHost, e->stream
    ));
    HIP_CHECK(hipStreamSynchronize(e->stream));
    if (cand_count > 1) {
      rocprim::double_buffer<u64> ckeys(e->d_cand2, e->d_cand);
      size_t ktb = e->cand_sort_temp_bytes;
      HIP_CHECK(rocprim::radix_sort_keys(e->d_cand_sort_temp, ktb, ckeys, cand_count, 0, 64,
                                         e->stream));
      const u64 *sorted = ckeys.current();
      const u32 cgrid = ceil_div(cand_count, threads);
      hipLaunchKernelGGL(
          k_extract_fav, dim3(cgrid), dim3(threads), 0, e->stream, sorted, cand_count, e->d_cfav
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_ones, dim3(cgrid), dim3(threads), 0, e->stream, cand_count, e->d_cones
      );
      LAUNCH_CHECK();
      size_t sctb = e->cand_scan_temp_bytes;
      HIP_CHECK(rocprim::inclusive_scan_by_key(
          e->d_cand_scan_temp, sctb, e->d_cfav, e->d_cones, e->d_crank, cand_count,
          rocprim::plus<u32>(), rocprim::equal_to<u32>(), e->stream
      ));
      HIP_CHECK(hipMemsetAsync(e->d_emptied, 0, sizeof(unsigned long long), e->stream));
      hipLaunchKernelGGL(
          k_twohop_pair, dim3(cgrid), dim3(threads), 0, e->stream, sorted, e->d_crank, cand_count,
          e->d_labels, e->d_weights, e->d_emptied
      );
      LAUNCH_CHECK();
      unsigned long long merged = 0;
      HIP_CHECK(hipMemcpyAsync(&merged, e->d_emptied, sizeof(merged), hipMemcpyDeviceToHost,
                               e->stream));
      HIP_CHECK(hipStreamSynchronize(e->stream));
      live -= merged;
    }
  }

  // exact non-empty cluster count + download
  HIP_CHECK(hipMemsetAsync(e->d_cut, 0, sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(
      k_count_nonempty, dim3(ngrid), dim3(threads), 0, e->stream, n, e->d_weights, e->d_cut
  );
  LAUNCH_CHECK();
  unsigned long long nonempty = 0, arcs = 0, moves = 0;
  HIP_CHECK(hipMemcpyAsync(&nonempty, e->d_cut, sizeof(nonempty), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipMemcpyAsync(&arcs, e->d_arcs, sizeof(arcs), hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipMemcpyAsync(&moves, e->d_moves, sizeof(moves), hipMemcpyDeviceToHost, e->stream));
  if (clustering != nullptr) {
    HIP_CHECK(hipMemcpy(clustering, e->d_labels, label_traffic(sizeof(u32) * n),
                        hipMemcpyDeviceToHost));
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->label_kind = kmp_lp_t::kLabelsClustering;
  e->shadows_ok = false;

  if (stats) {
    stats->arcs_scanned = arcs;
    stats->moves = moves;
    stats->phase_a_ns = static_cast<u64>(e->phase_a_ms * 1e6);
    stats->total_ns = static_cast<u64>(e->commit_ms * 1e6);
    stats->num_clusters = nonempty;
    stats->edge_cut = 0;
  }
  return static_cast<i64>(nonempty);
}

} // extern "C"

// ==================== Jet refiner driver ====================
// Schedule, rebalancing and best-snapshot bookkeeping of kmp_lp_jet (see
// include/kaminpar_lp.h); the find / afterburner kernels live in jet_hip.hip.
// Inside the iteration loop nothing of size n crosses PCIe: per iteration the
// host reads the k block weights, two counters and the cut.

namespace {

// Counts isolated vertices that sit in over-cap blocks (the only ones the
// balancer's isolated pre-pass can move).
__global__ void k_jet_iso_probe(
    const u32 *__restrict__ idx, u32 count, const u32 *__restrict__ labels,
    const i64 *__restrict__ weights, const i64 *__restrict__ maxw, u32 *__restrict__ hits
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  bool hit = false;
  if (i < count) {
    const u32 b = labels[idx[i]];
    hit = weights[b] > maxw[b];
  }
  const unsigned long long mask = __ballot(hit);
  if ((threadIdx.x & (kWave - 1)) == 0 && mask) {
    atomicAdd(hits, static_cast<u32>(__popcll(mask)));
  }
}

__global__ void k_jet_iso_gather(
    const u32 *__restrict__ idx, u32 count, const u32 *__restrict__ labels, u32 *__restrict__ out
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    out[i] = labels[idx[i]];
  }
}

__global__ void k_jet_iso_scatter(
    const u32 *__restrict__ idx, u32 count, const u32 *__restrict__ in, u32 *__restrict__ labels,
    uint16_t *__restrict__ labels16, uint8_t *__restrict__ labels8
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    const u32 u = idx[i];
    const u32 l = in[i];
    labels[u] = l;
    labels16[u] = static_cast<uint16_t>(l);
    labels8[u] = static_cast<uint8_t>(l);
  }
}

struct JetRun {
  kmp_lp_t *e = nullptr;
  kmp_jet::View view{};
  u32 m_count = 0, l_count = 0;
  u32 *d_best = nullptr;
  u32 *d_iso_idx = nullptr, *d_iso_lab = nullptr, *d_iso_hits = nullptr;
  unsigned long long *d_counters = nullptr; // [0] arcs, [1] moves
  std::vector<i64> w; // host copy of the block weights
  std::vector<u32> iso_lab;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  void free_all() {
    for (void *p : {(void *)view.lock, (void *)view.rec, (void *)view.m_list, (void *)view.l_list,
                    (void *)view.tier_counts, (void *)d_best, (void *)d_iso_idx,
                    (void *)d_iso_lab, (void *)d_iso_hits, (void *)d_counters}) {
      if (p) {
        (void)hipFree(p);
      }
    }
    if (ev0) {
      (void)hipEventDestroy(ev0);
    }
    if (ev1) {
      (void)hipEventDestroy(ev1);
    }
  }
};

void jet_read_weights(JetRun &r) {
  kmp_lp_t *e = r.e;
  HIP_CHECK(hipMemcpyAsync(r.w.data(), e->d_weights, sizeof(i64) * e->k, hipMemcpyDeviceToHost,
                           e->stream));
  sync_spin(e);
}

bool jet_feasible(const JetRun &r) {
  for (u32 c = 0; c < r.e->k; ++c) {
    if (r.w[c] > r.e->maxw_host[c]) {
      return false;
    }
  }
  return true;
}

// Step 5. Same sum as k_edge_cut, over the Jet degree tiers: k_edge_cut gives
// every row 16 lanes and serializes on hub rows (measured 21.7 ms per pass on
// R-MAT scale 23, against 3.1 ms for find + filter).
i64 jet_device_cut(JetRun &r) {
  kmp_lp_t *e = r.e;
  kmp_jet::edge_cut2(r.view, r.m_count, r.l_count, e->d_cut, e->stream);
  unsigned long long cut2 = 0;
  HIP_CHECK(hipMemcpyAsync(&cut2, e->d_cut, sizeof(cut2), hipMemcpyDeviceToHost, e->stream));
  sync_spin(e);
  return static_cast<i64>(cut2 / 2);
}

// Step 4 with balancer == 0 (balancer == 1: select_rebalance below):
// kmp_lp_balance on the device-resident labels (isolated pre-pass included,
// same order and rule). r.w holds the current weights on entry.
// Returns the committed balancer moves, or -1.
i64 jet_rebalance(JetRun &r, u64 seed, int iters) {
  kmp_lp_t *e = r.e;
  const u32 k = e->k;
  const u32 threads = 256;
  const u32 icount = static_cast<u32>(e->isolated.size());
  if (icount > 0) {
    const u32 grid = ceil_div(icount, threads);
    HIP_CHECK(hipMemsetAsync(r.d_iso_hits, 0, sizeof(u32), e->stream));
    hipLaunchKernelGGL(
        k_jet_iso_probe, dim3(grid), dim3(threads), 0, e->stream, r.d_iso_idx, icount,
        e->d_labels, e->d_weights, e->d_maxw, r.d_iso_hits
    );
    LAUNCH_CHECK();
    u32 hits = 0;
    HIP_CHECK(hipMemcpyAsync(&hits, r.d_iso_hits, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    sync_spin(e);
    if (hits > 0) {
      hipLaunchKernelGGL(
          k_jet_iso_gather, dim3(grid), dim3(threads), 0, e->stream, r.d_iso_idx, icount,
          e->d_labels, r.d_iso_lab
      );
      LAUNCH_CHECK();
      HIP_CHECK(hipMemcpyAsync(r.iso_lab.data(), r.d_iso_lab, sizeof(u32) * icount,
                               hipMemcpyDeviceToHost, e->stream));
      sync_spin(e);
      std::vector<i64> w = r.w;
      for (u32 i = 0; i < icount; ++i) {
        const i32 uw = e->iso_weights[i];
        const u32 b = r.iso_lab[i];
        if (w[b] <= e->maxw_host[b]) {
          continue;
        }
        i64 best = -1;
        u32 t = b;
        for (u32 c = 0; c < k; ++c) {
          if (c != b && w[c] + uw <= e->maxw_host[c] && (best < 0 || w[c] < best)) {
            best = w[c];
            t = c;
          }
        }
        if (t != b) {
          w[b] -= uw;
          w[t] += uw;
          r.iso_lab[i] = t;
        }
      }
      HIP_CHECK(hipMemcpyAsync(r.d_iso_lab, r.iso_lab.data(), sizeof(u32) * icount,
                               hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(
          k_jet_iso_scatter, dim3(grid), dim3(threads), 0, e->stream, r.d_iso_idx, icount,
          r.d_iso_lab, e->d_labels, e->d_labels16, e->d_labels8
      );
      LAUNCH_CHECK();
      sync_spin(e); // iso_lab is pageable: keep it alive until the copy landed
    }
  }
  refine_load_state(e, false); // active set, counters and weights from d_labels
  e->seed = seed;
  e->ev_used = 0;
  e->balance = 1;
  const i64 moved = kmp_lp_run_sweeps(e, iters);
  e->balance = 0;
  return moved;
}

// Workspace and running totals of the selection rebalancer
// (kmp_lp_rebalance, and kmp_lp_jet's step 4 with balancer == 1). Allocated
// on first use, once per call: nothing is allocated inside the pass loop.
struct RebalRun {
  kmp_jet::Rebal rb{};
  std::vector<void *> owned;
  std::vector<i64> tables; // over | room | cum, k each
  unsigned long long seen[3] = {0, 0, 0}; // arcs, selected, moves: last read
  u64 passes = 0;
  double score_ms = 0.0;
  bool ready = false;

  template <typename T>
  void take(T *&p, size_t count) {
    HIP_CHECK(hipMalloc(&p, sizeof(T) * (count > 0 ? count : 1)));
    owned.push_back(p);
  }

  void alloc(u32 n, u32 k, hipStream_t stream) {
    tables.resize(static_cast<size_t>(k) * 3);
    take(rb.over, static_cast<size_t>(k) * 3);
    rb.room = rb.over + k;
    rb.cum = rb.room + k;
    take(rb.key, n);
    take(rb.to, n);
    take(rb.flag, n);
    take(rb.ids[0], n);
    take(rb.ids[1], n);
    take(rb.keys[0], n);
    take(rb.keys[1], n);
    take(rb.seg, n);
    take(rb.wt, n);
    take(rb.pre, n);
    take(rb.count, 1);
    take(rb.arcs, 3);
    rb.selected = rb.arcs + 1;
    rb.moves = rb.arcs + 2;
    rb.temp_bytes = kmp_jet::rebalance_temp_bytes(n);
    uint8_t *temp = nullptr;
    take(temp, rb.temp_bytes);
    rb.temp = temp;
    HIP_CHECK(hipMemsetAsync(rb.arcs, 0, sizeof(unsigned long long) * 3, stream));
    ready = true;
  }

  void free_all() {
    for (void *p : owned) {
      (void)hipFree(p);
    }
    owned.clear();
    ready = false;
  }
};

u32 rebal_read_count(JetRun &r, RebalRun &b) {
  u32 count = 0;
  HIP_CHECK(hipMemcpyAsync(&count, b.rb.count, sizeof(u32), hipMemcpyDeviceToHost, r.e->stream));
  sync_spin(r.e);
  return count;
}

// Block weights and the three counters; true iff the pass admitted a move.
bool rebal_read_state(JetRun &r, RebalRun &b) {
  unsigned long long now[3] = {0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(now, b.rb.arcs, sizeof(now), hipMemcpyDeviceToHost, r.e->stream));
  jet_read_weights(r); // synchronizes
  const bool moved = now[2] != b.seen[2];
  b.seen[0] = now[0];
  b.seen[1] = now[1];
  b.seen[2] = now[2];
  return moved;
}

// Up to max_passes passes of the selection rebalancer on the device-resident
// labels (rule: include/kaminpar_lp.h). r.w holds the current weights on entry
// and on return. Per pass the host uploads the three k-sized tables and reads
// two list lengths, three counters and the k block weights. Returns the
// admitted moves of this call.
i64 select_rebalance(JetRun &r, RebalRun &b, int max_passes) {
  kmp_lp_t *e = r.e;
  const u32 k = e->k;
  if (!b.ready) {
    b.alloc(e->n, k, e->stream);
  }
  const unsigned long long moves0 = b.seen[2];
  for (int pass = 0; pass < max_passes; ++pass) {
    i64 *over = b.tables.data();
    i64 *room = over + k;
    i64 *cum = room + k;
    bool any_over = false;
    i64 acc = 0;
    u32 best = 0;
    for (u32 c = 0; c < k; ++c) {
      over[c] = r.w[c] - e->maxw_host[c];
      room[c] = -over[c];
      any_over = any_over || over[c] > 0;
      acc += room[c] > 0 ? room[c] : 0;
      cum[c] = acc;
      if (room[c] > room[best]) {
        best = c;
      }
    }
    if (!any_over) {
      break;
    }
    b.rb.total_room = acc;
    b.rb.best_target = best;
    b.rb.pass = static_cast<u32>(pass);
    HIP_CHECK(hipMemcpyAsync(b.rb.over, over, sizeof(i64) * 3 * k, hipMemcpyHostToDevice,
                             e->stream));
    HIP_CHECK(hipEventRecord(r.ev0, e->stream));
    kmp_jet::rebalance_score(r.view, b.rb, r.m_count, r.l_count, e->stream);
    HIP_CHECK(hipEventRecord(r.ev1, e->stream));
    const u32 candidates = rebal_read_count(r, b);
    {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, r.ev0, r.ev1));
      b.score_ms += ms;
    }
    b.passes += 1;
    if (candidates == 0) { // nothing can leave: stalled
      rebal_read_state(r, b);
      break;
    }
    kmp_jet::rebalance_order(r.view, b.rb, candidates, false, e->stream);
    kmp_jet::rebalance_select(r.view, b.rb, candidates, e->stream);
    const u32 selected = rebal_read_count(r, b);
    kmp_jet::rebalance_order(r.view, b.rb, selected, true, e->stream);
    kmp_jet::rebalance_apply(r.view, b.rb, selected, e->stream);
    if (!rebal_read_state(r, b)) { // admitted nothing: stalled
      break;
    }
  }
  return static_cast<i64>(b.seen[2] - moves0);
}

// Degree tiers, counters and events shared by kmp_lp_jet and
// kmp_lp_rebalance; the labels are on the device and the LP state is loaded.
void jet_run_setup(JetRun &r, kmp_lp_t *e) {
  const u32 n = e->n;
  const size_t nn = n > 0 ? n : 1;
  r.e = e;
  r.w.resize(e->k);
  HIP_CHECK(hipMalloc(&r.view.m_list, sizeof(u32) * nn));
  HIP_CHECK(hipMalloc(&r.view.l_list, sizeof(u32) * nn));
  HIP_CHECK(hipMalloc(&r.view.tier_counts, sizeof(u32) * 2));
  HIP_CHECK(hipMalloc(&r.d_counters, sizeof(unsigned long long) * 2));
  HIP_CHECK(hipEventCreate(&r.ev0));
  HIP_CHECK(hipEventCreate(&r.ev1));
  r.view.n = n;
  r.view.k = e->k;
  r.view.xadj = e->d_xadj;
  r.view.adjncy = e->d_adjncy;
  r.view.adjwgt = e->d_adjwgt;
  r.view.vwgt = e->d_vwgt;
  r.view.labels = e->d_labels;
  r.view.labels16 = e->d_labels16;
  r.view.labels8 = e->d_labels8;
  r.view.weights = e->d_weights;
  r.view.arcs = r.d_counters;
  r.view.moves = r.d_counters + 1;
  HIP_CHECK(hipMemsetAsync(r.d_counters, 0, sizeof(unsigned long long) * 2, e->stream));
  kmp_jet::build_tiers(r.view, e->stream);
  u32 counts[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(counts, r.view.tier_counts, sizeof(counts), hipMemcpyDeviceToHost,
                           e->stream));
  sync_spin(e);
  r.m_count = counts[0];
  r.l_count = counts[1];
}

} // namespace

extern "C" {

kmp_jet_params_t kmp_jet_params_default(int coarse_level) {
  kmp_jet_params_t p;
  p.num_rounds = 1;
  p.max_iterations = 0;
  p.max_fruitless = 12;
  p.fruitless_threshold = 0.999;
  p.initial_gain_temp = coarse_level != 0 ? 0.75 : 0.25;
  p.final_gain_temp = p.initial_gain_temp;
  p.balance_iters = 2; // measured choice: DESIGN.md section 8
  p.balancer = 0;
  p.balance_passes = 16;
  return p;
}

int kmp_jet_params_valid(const kmp_jet_params_t *params) {
  if (params == nullptr) {
    return 0;
  }
  const kmp_jet_params_t &p = *params;
  return !(p.num_rounds < 1 || p.max_iterations < 0 || p.max_fruitless < 0 ||
           p.balance_iters < 1 || (p.max_iterations == 0 && p.max_fruitless == 0) ||
           !(p.fruitless_threshold >= 0.0) || !(p.fruitless_threshold <= 1.0) ||
           !(p.initial_gain_temp >= 0.0) || !(p.final_gain_temp >= 0.0) ||
           !std::isfinite(p.initial_gain_temp) || !std::isfinite(p.final_gain_temp) ||
           (p.balancer != 0 && p.balancer != 1) || (p.balancer == 1 && p.balance_passes < 1));
}

i64 kmp_lp_rebalance(
    kmp_lp_t *e, u32 k, const i64 *max_block_weights, u32 *partition, int max_passes,
    kmp_rebalance_stats_t *stats
) {
  if (max_passes < 1) {
    fprintf(stderr, "kaminpar_amd: rebalance: max_passes %d is not >= 1\n", max_passes);
    e->label_kind = kmp_lp_t::kLabelsNone;
    return -1;
  }
  if (dense_k_ok(k, "rebalance") != 0) {
    return -1;
  }
  const auto wall0 = std::chrono::steady_clock::now();
  const u32 n = e->n;
  const bool resident = partition == nullptr;
  const bool resident_ok = resident && resident_partition_ok(e, k, "rebalance") == 0;
  e->label_kind = kmp_lp_t::kLabelsNone;
  if (resident && !resident_ok) {
    return -1;
  }
  // labels index the kernels' k-sized LDS tables: reject out-of-range input
  // (a resident partition was validated when it became one)
  for (u32 u = 0; !resident && u < n; ++u) {
    if (partition[u] >= k) {
      fprintf(stderr, "kaminpar_amd: rebalance: partition[%u] = %u is not below k = %u\n", u,
              partition[u], k);
      return -1;
    }
  }
  if (refine_setup(e, k, max_block_weights, 0) != 0) {
    return -1;
  }
  if (!resident) {
    HIP_CHECK(hipMemcpy(e->d_labels, partition, label_traffic(sizeof(u32) * n),
                        hipMemcpyHostToDevice));
  }
  refine_load_state(e, true);
  refine_setup_commit(e);

  JetRun r;
  RebalRun rebal;
  jet_run_setup(r, e);
  jet_read_weights(r);
  if (!jet_feasible(r)) {
    select_rebalance(r, rebal, max_passes);
  }
  const i64 cut = jet_device_cut(r);
  const bool feasible = jet_feasible(r);
  if (!resident) {
    HIP_CHECK(hipMemcpy(partition, e->d_labels, label_traffic(sizeof(u32) * n),
                        hipMemcpyDeviceToHost));
  }
  r.free_all();
  rebal.free_all();
  e->label_kind = kmp_lp_t::kLabelsPartition; // moves go to blocks below k only
  e->label_k = k;
  e->shadows_ok = true; // refine_load_state synced them; k_rb_apply writes all three
  if (stats) {
    kmp_rebalance_stats_t st{};
    st.passes = rebal.passes;
    st.selected = rebal.seen[1];
    st.moves = rebal.seen[2];
    st.arcs_scanned = rebal.seen[0];
    st.score_ns = static_cast<u64>(rebal.score_ms * 1e6);
    st.total_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                       std::chrono::steady_clock::now() - wall0)
                                       .count());
    st.edge_cut = cut;
    st.feasible = feasible ? 1 : 0;
    *stats = st;
  }
  return cut;
}

i64 kmp_lp_jet(
    kmp_lp_t *e, u32 k, const i64 *max_block_weights, u32 *partition, u64 seed,
    const kmp_jet_params_t *params, kmp_jet_stats_t *stats
) {
  if (params == nullptr) {
    fprintf(stderr, "kaminpar_amd: jet needs parameters (see kmp_jet_params_default)\n");
    e->label_kind = kmp_lp_t::kLabelsNone;
    return -1;
  }
  const kmp_jet_params_t p = *params;
  if (!kmp_jet_params_valid(params)) {
    fprintf(stderr,
            "kaminpar_amd: bad jet parameters (rounds %d, max_iterations %d, max_fruitless %d, "
            "threshold %g, temperatures %g..%g, balance_iters %d, balancer %d, "
            "balance_passes %d)\n",
            p.num_rounds, p.max_iterations, p.max_fruitless, p.fruitless_threshold,
            p.initial_gain_temp, p.final_gain_temp, p.balance_iters, p.balancer,
            p.balance_passes);
    e->label_kind = kmp_lp_t::kLabelsNone;
    return -1;
  }
  if (dense_k_ok(k, "jet") != 0) {
    return -1;
  }
  const auto wall0 = std::chrono::steady_clock::now();
  const u32 n = e->n;
  const bool resident = partition == nullptr;
  const bool resident_ok = resident && resident_partition_ok(e, k, "jet") == 0;
  e->label_kind = kmp_lp_t::kLabelsNone;
  if (resident && !resident_ok) {
    return -1;
  }
  // labels index the kernels' k-sized LDS tables: reject out-of-range input
  // (a resident partition was validated when it became one)
  for (u32 u = 0; !resident && u < n; ++u) {
    if (partition[u] >= k) {
      fprintf(stderr, "kaminpar_amd: jet: partition[%u] = %u is not below k = %u\n", u,
              partition[u], k);
      return -1;
    }
  }
  if (refine_setup(e, k, max_block_weights, seed) != 0) {
    return -1;
  }
  if (!resident) {
    HIP_CHECK(hipMemcpy(e->d_labels, partition, label_traffic(sizeof(u32) * n),
                        hipMemcpyHostToDevice));
  }
  refine_load_state(e, true);
  refine_setup_commit(e);

  JetRun r;
  RebalRun rebal;
  const size_t nn = n > 0 ? n : 1;
  HIP_CHECK(hipMalloc(&r.view.lock, nn));
  HIP_CHECK(hipMalloc(&r.view.rec, sizeof(kmp_jet::Rec) * nn));
  HIP_CHECK(hipMalloc(&r.d_best, sizeof(u32) * nn));
  const u32 icount = static_cast<u32>(e->isolated.size());
  if (icount > 0 && p.balancer == 0) {
    HIP_CHECK(hipMalloc(&r.d_iso_idx, sizeof(u32) * icount));
    HIP_CHECK(hipMalloc(&r.d_iso_lab, sizeof(u32) * icount));
    HIP_CHECK(hipMalloc(&r.d_iso_hits, sizeof(u32)));
    HIP_CHECK(hipMemcpy(r.d_iso_idx, e->isolated.data(), sizeof(u32) * icount,
                        hipMemcpyHostToDevice));
    r.iso_lab.resize(icount);
  }
  HIP_CHECK(hipMemsetAsync(r.view.lock, 0, nn, e->stream));
  jet_run_setup(r, e);

  jet_read_weights(r);
  bool best_f = jet_feasible(r);
  i64 best_cut = jet_device_cut(r);
  HIP_CHECK(hipMemcpyAsync(r.d_best, e->d_labels, sizeof(u32) * n, hipMemcpyDeviceToDevice,
                           e->stream));

  kmp_jet_stats_t st{};
  double ff_ms = 0.0;
  u64 global_iter = 0;
  bool failed = false;
  for (int round = 0; round < p.num_rounds && !failed; ++round) {
    const double temp =
        p.num_rounds > 1
            ? p.initial_gain_temp + (static_cast<double>(round) / (p.num_rounds - 1)) *
                                        (p.final_gain_temp - p.initial_gain_temp)
            : (p.initial_gain_temp + p.final_gain_temp) / 2.0;
    int iters = 0;
    int fruitless = 0;
    bool cur_is_best = true;
    while (true) {
      HIP_CHECK(hipEventRecord(r.ev0, e->stream));
      kmp_jet::find(r.view, temp, r.m_count, r.l_count, e->stream);
      kmp_jet::filter_commit(r.view, r.m_count, r.l_count, e->stream);
      HIP_CHECK(hipEventRecord(r.ev1, e->stream));
      jet_read_weights(r);
      {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, r.ev0, r.ev1));
        ff_ms += ms;
      }
      if (!jet_feasible(r)) {
        const auto bal0 = std::chrono::steady_clock::now();
        const i64 moved = p.balancer == 1
                              ? select_rebalance(r, rebal, p.balance_passes)
                              : jet_rebalance(r, seed + global_iter, p.balance_iters);
        if (moved < 0) {
          failed = true;
          break;
        }
        st.balancer_calls += 1;
        st.balancer_moves += static_cast<u64>(moved);
        jet_read_weights(r);
        st.balancer_ns += static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                               std::chrono::steady_clock::now() - bal0)
                                               .count());
      }
      const i64 c = jet_device_cut(r);
      const bool f = jet_feasible(r);
      st.feasible_iterations += f ? 1 : 0;
      ++global_iter;
      ++iters;
      st.iterations += 1;

      const bool gained = f && !best_f;
      ++fruitless;
      if (gained || (f == best_f && static_cast<double>(best_cut - c) >
                                        (1.0 - p.fruitless_threshold) *
                                            static_cast<double>(best_cut))) {
        fruitless = 0;
      }
      if (gained || (f == best_f && c <= best_cut)) {
        HIP_CHECK(hipMemcpyAsync(r.d_best, e->d_labels, sizeof(u32) * n,
                                 hipMemcpyDeviceToDevice, e->stream));
        cur_is_best = true;
      } else {
        cur_is_best = false;
      }
      if (gained) {
        best_cut = c;
        best_f = true;
      } else if (f == best_f && c < best_cut) {
        best_cut = c;
      }
      if ((p.max_iterations != 0 && iters == p.max_iterations) ||
          (p.max_fruitless != 0 && fruitless == p.max_fruitless)) {
        break;
      }
    }
    if (!failed && !cur_is_best) {
      // roll back to the best state and rederive shadows + block weights
      HIP_CHECK(hipMemcpyAsync(e->d_labels, r.d_best, sizeof(u32) * n, hipMemcpyDeviceToDevice,
                               e->stream));
      refine_load_state(e, false);
    }
  }

  unsigned long long counters[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(counters, r.d_counters, sizeof(counters), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  if (!failed && !resident) {
    HIP_CHECK(hipMemcpy(partition, r.d_best, label_traffic(sizeof(u32) * n),
                        hipMemcpyDeviceToHost));
  }
  r.free_all();
  rebal.free_all();
  if (failed) {
    return -1;
  }
  // every round ends with d_labels equal to the best state: either the last
  // iteration was the best, or the rollback above restored it and
  // refine_load_state resynced the shadows. All writers in between (filter,
  // balance sweeps, k_rb_apply, the isolated scatter) write all three arrays.
  e->label_kind = kmp_lp_t::kLabelsPartition;
  e->label_k = k;
  e->shadows_ok = true;
  if (stats) {
    st.jet_moves = counters[1];
    st.arcs_scanned = counters[0];
    st.balancer_passes = rebal.passes;
    st.find_filter_ns = static_cast<u64>(ff_ms * 1e6);
    st.total_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                       std::chrono::steady_clock::now() - wall0)
                                       .count());
    st.edge_cut = best_cut;
    *stats = st;
  }
  return best_cut;
}

} // extern "C"

// ==================== cluster contraction (GPU) ====================
// Restates kaminpar-shm/coarsening/contraction/ semantics (see
// kmp_contract in include/kaminpar_lp.h). All steps are order-free integer
// sums / stable sorts, so the result is deterministic and bit-identical to
// the CPU oracle and (canonically sorted) to the reference implementation.

namespace {

__global__ void k_mark_clusters(
    u32 n, const u32 *__restrict__ clus, u32 *__restrict__ rank
) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n) {
    rank[clus[u]] = 1;
  }
}

__global__ void k_map_ranks(
    u32 n, const u32 *__restrict__ clus, const u32 *__restrict__ rank, u32 *__restrict__ map
) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n) {
    map[u] = rank[clus[u]] - 1;
  }
}

__global__ void k_coarse_vwgt(
    u32 n, const u32 *__restrict__ map, const i32 *__restrict__ vwgt, i32 *__restrict__ cvw
) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n) {
    atomicAdd(&cvw[map[u]], vwgt ? vwgt[u] : 1);
  }
}

// One 16-lane subgroup per vertex (grid-stride): emit (cu<<32|cv) keys per
// arc; intra-cluster arcs get the ~0 sentinel (sorted to the end, dropped).
__global__ void k_arc_keys(
    u32 n,
    const u64 *__restrict__ xadj,
    const u32 *__restrict__ adjncy,
    const i32 *__restrict__ adjwgt,
    const u32 *__restrict__ map,
    u64 *__restrict__ keys,
    i32 *__restrict__ vals
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  for (u32 base = wave_id * 4; base < n; base += num_waves * 4) {
    const u32 u = base + sub;
    if (u >= n) {
      continue;
    }
    const u64 row = xadj[u];
    const u32 deg = static_cast<u32>(xadj[u + 1] - row);
    const u32 cu = map[u];
    for (u32 e = slot; e < deg; e += 16) {
      const u32 cv = map[adjncy[row + e]];
      keys[row + e] = (cu == cv) ? ~0ull : ((static_cast<u64>(cu) << 32) | cv);
      vals[row + e] = adjwgt ? adjwgt[row + e] : 1;
    }
  }
}

__global__ void k_coarse_hist(
    u32 c_m, const u64 *__restrict__ ukeys, unsigned long long *__restrict__ cxadj
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c_m) {
    atomicAdd(&cxadj[(ukeys[i] >> 32) + 1], 1ull);
  }
}

__global__ void k_coarse_adj(
    u32 c_m, const u64 *__restrict__ ukeys, u32 *__restrict__ cadj
) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c_m) {
    cadj[i] = static_cast<u32>(ukeys[i] & 0xFFFFFFFFu);
  }
}

} // namespace

extern "C" {

namespace {

// Output of contract_core: right-sized device arrays the caller either
// downloads (kmp_contract) or adopts into a new engine (kmp_contract_engine).
struct ContractOut {
  u32 c_n = 0;
  u32 c_m = 0;
  u32 *d_map = nullptr;   // n
  u64 *d_cxadj = nullptr; // c_n + 1 (prefix-summed)
  u32 *d_cadj = nullptr;  // max(c_m, 1)
  i32 *d_cvw = nullptr;   // c_n
  i32 *d_cwgt = nullptr;  // max(c_m, 1)
};

// clustering == nullptr: contract the clustering in e->d_labels, read in
// place (the caller has checked that the engine holds one).
int contract_core(kmp_lp_t *e, const u32 *clustering, ContractOut &o) {
  const u32 n = e->n;
  const u64 m = e->m;
  if (m > 0xFFFFFFFFull) {
    fprintf(stderr, "kaminpar_amd: kmp_contract supports m < 2^32 arcs\n");
    return -1;
  }
  const u32 threads = 256;
  const u32 ngrid = ceil_div(n, threads);
  hipStream_t s = e->stream;

  u32 *d_clus = nullptr, *d_rank = nullptr;
  i32 *d_cvw_full = nullptr, *d_vals[2] = {nullptr, nullptr}, *d_usums = nullptr;
  u64 *d_keys[2] = {nullptr, nullptr}, *d_ukeys = nullptr;
  u32 *d_uniq = nullptr;
  u32 *d_clus_own = nullptr; // staging copy of a host clustering
  if (clustering != nullptr) {
    HIP_CHECK(hipMalloc(&d_clus_own, sizeof(u32) * n));
    d_clus = d_clus_own;
  } else {
    d_clus = e->d_labels;
  }
  HIP_CHECK(hipMalloc(&d_rank, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&o.d_map, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_cvw_full, sizeof(i32) * n));
  HIP_CHECK(hipMalloc(&d_keys[0], sizeof(u64) * m));
  HIP_CHECK(hipMalloc(&d_keys[1], sizeof(u64) * m));
  HIP_CHECK(hipMalloc(&d_vals[0], sizeof(i32) * m));
  HIP_CHECK(hipMalloc(&d_vals[1], sizeof(i32) * m));
  HIP_CHECK(hipMalloc(&d_ukeys, sizeof(u64) * m));
  HIP_CHECK(hipMalloc(&d_usums, sizeof(i32) * m));
  HIP_CHECK(hipMalloc(&d_uniq, sizeof(u32)));

  if (clustering != nullptr) {
    HIP_CHECK(hipMemcpyAsync(d_clus_own, clustering, label_traffic(sizeof(u32) * n),
                             hipMemcpyHostToDevice, s));
  }
  HIP_CHECK(hipMemsetAsync(d_rank, 0, sizeof(u32) * n, s));
  hipLaunchKernelGGL(k_mark_clusters, dim3(ngrid), dim3(threads), 0, s, n, d_clus, d_rank);
  LAUNCH_CHECK();

  void *tmp = nullptr;
  size_t tmp_bytes = 0;
  HIP_CHECK(rocprim::inclusive_scan(nullptr, tmp_bytes, d_rank, d_rank, n, rocprim::plus<u32>()));
  HIP_CHECK(hipMalloc(&tmp, tmp_bytes));
  HIP_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, d_rank, d_rank, n, rocprim::plus<u32>(), s));
  u32 c_n = 0;
  HIP_CHECK(hipMemcpyAsync(&c_n, d_rank + n - 1, sizeof(u32), hipMemcpyDeviceToHost, s));
  hipLaunchKernelGGL(k_map_ranks, dim3(ngrid), dim3(threads), 0, s, n, d_clus, d_rank, o.d_map);
  LAUNCH_CHECK();
  HIP_CHECK(hipMemsetAsync(d_cvw_full, 0, sizeof(i32) * n, s));
  hipLaunchKernelGGL(
      k_coarse_vwgt, dim3(ngrid), dim3(threads), 0, s, n, o.d_map, e->d_vwgt, d_cvw_full
  );
  LAUNCH_CHECK();
  hipLaunchKernelGGL(
      k_arc_keys, dim3(16384), dim3(threads), 0, s, n, e->d_xadj, e->d_adjncy, e->d_adjwgt,
      o.d_map, d_keys[0], d_vals[0]
  );
  LAUNCH_CHECK();

  rocprim::double_buffer<u64> kb(d_keys[0], d_keys[1]);
  rocprim::double_buffer<i32> vb(d_vals[0], d_vals[1]);
  void *tmp2 = nullptr;
  size_t tmp2_bytes = 0;
  HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp2_bytes, kb, vb, m, 0, 64));
  HIP_CHECK(hipMalloc(&tmp2, tmp2_bytes));
  HIP_CHECK(rocprim::radix_sort_pairs(tmp2, tmp2_bytes, kb, vb, m, 0, 64, s));

  void *tmp3 = nullptr;
  size_t tmp3_bytes = 0;
  HIP_CHECK(rocprim::reduce_by_key(
      nullptr, tmp3_bytes, kb.current(), vb.current(), m, d_ukeys, d_usums, d_uniq,
      rocprim::plus<i32>(), rocprim::equal_to<u64>()
  ));
  HIP_CHECK(hipMalloc(&tmp3, tmp3_bytes));
  HIP_CHECK(rocprim::reduce_by_key(
      tmp3, tmp3_bytes, kb.current(), vb.current(), m, d_ukeys, d_usums, d_uniq,
      rocprim::plus<i32>(), rocprim::equal_to<u64>(), s
  ));
  u32 uniq = 0;
  HIP_CHECK(hipMemcpyAsync(&uniq, d_uniq, sizeof(u32), hipMemcpyDeviceToHost, s));
  u64 last_key = 0;
  HIP_CHECK(hipStreamSynchronize(s));
  if (uniq > 0) {
    HIP_CHECK(hipMemcpy(&last_key, d_ukeys + uniq - 1, sizeof(u64), hipMemcpyDeviceToHost));
  }
  const u32 c_m = (uniq > 0 && last_key == ~0ull) ? uniq - 1 : uniq;

  HIP_CHECK(hipMalloc(&o.d_cxadj, sizeof(u64) * (c_n + 1)));
  HIP_CHECK(hipMalloc(&o.d_cadj, sizeof(u32) * (c_m > 0 ? c_m : 1)));
  HIP_CHECK(hipMemsetAsync(o.d_cxadj, 0, sizeof(u64) * (c_n + 1), s));
  if (c_m > 0) {
    hipLaunchKernelGGL(
        k_coarse_hist, dim3(ceil_div(c_m, threads)), dim3(threads), 0, s, c_m, d_ukeys,
        reinterpret_cast<unsigned long long *>(o.d_cxadj)
    );
    LAUNCH_CHECK();
    hipLaunchKernelGGL(
        k_coarse_adj, dim3(ceil_div(c_m, threads)), dim3(threads), 0, s, c_m, d_ukeys, o.d_cadj
    );
    LAUNCH_CHECK();
  }
  void *tmp4 = nullptr;
  size_t tmp4_bytes = 0;
  HIP_CHECK(rocprim::inclusive_scan(
      nullptr, tmp4_bytes, o.d_cxadj, o.d_cxadj, c_n + 1, rocprim::plus<u64>()
  ));
  HIP_CHECK(hipMalloc(&tmp4, tmp4_bytes));
  HIP_CHECK(rocprim::inclusive_scan(
      tmp4, tmp4_bytes, o.d_cxadj, o.d_cxadj, c_n + 1, rocprim::plus<u64>(), s
  ));

  // right-size the coarse node/edge weights
  HIP_CHECK(hipMalloc(&o.d_cvw, sizeof(i32) * (c_n > 0 ? c_n : 1)));
  HIP_CHECK(hipMalloc(&o.d_cwgt, sizeof(i32) * (c_m > 0 ? c_m : 1)));
  HIP_CHECK(
      hipMemcpyAsync(o.d_cvw, d_cvw_full, sizeof(i32) * c_n, hipMemcpyDeviceToDevice, s)
  );
  if (c_m > 0) {
    HIP_CHECK(hipMemcpyAsync(o.d_cwgt, d_usums, sizeof(i32) * c_m, hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));

  for (void *p : {(void *)d_clus_own, (void *)d_rank, (void *)d_cvw_full, (void *)d_keys[0],
                  (void *)d_keys[1], (void *)d_vals[0], (void *)d_vals[1], (void *)d_ukeys,
                  (void *)d_usums, (void *)d_uniq, tmp, tmp2, tmp3, tmp4}) {
    if (p) {
      (void)hipFree(p);
    }
  }
  o.c_n = c_n;
  o.c_m = c_m;
  return 0;
}

void contract_out_free(ContractOut &o) {
  for (void *p : {(void *)o.d_map, (void *)o.d_cxadj, (void *)o.d_cadj, (void *)o.d_cvw,
                  (void *)o.d_cwgt}) {
    if (p) {
      (void)hipFree(p);
    }
  }
}

} // namespace

i64 kmp_contract(
    kmp_lp_t *e, const u32 *clustering, u32 *mapping_out, kmp_graph_t **coarse_out
) {
  ContractOut o;
  if (contract_core(e, clustering, o) != 0) {
    return -1;
  }
  hipStream_t s = e->stream;
  const u32 c_n = o.c_n, c_m = o.c_m;

  std::vector<u64> h_cxadj64(c_n + 1);
  std::vector<u32> h_cxadj(c_n + 1), h_cadj(c_m);
  std::vector<i32> h_cvw(c_n), h_cwgt(c_m);
  HIP_CHECK(hipMemcpyAsync(mapping_out, o.d_map, label_traffic(sizeof(u32) * e->n),
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(h_cxadj64.data(), o.d_cxadj, sizeof(u64) * (c_n + 1),
                           hipMemcpyDeviceToHost, s));
  if (c_m > 0) {
    HIP_CHECK(
        hipMemcpyAsync(h_cadj.data(), o.d_cadj, sizeof(u32) * c_m, hipMemcpyDeviceToHost, s)
    );
    HIP_CHECK(
        hipMemcpyAsync(h_cwgt.data(), o.d_cwgt, sizeof(i32) * c_m, hipMemcpyDeviceToHost, s)
    );
  }
  HIP_CHECK(hipMemcpyAsync(h_cvw.data(), o.d_cvw, sizeof(i32) * c_n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (u32 i = 0; i <= c_n; ++i) {
    h_cxadj[i] = static_cast<u32>(h_cxadj64[i]); // c_m < 2^32 (entry guard)
  }

  *coarse_out = kmp_graph_from_csr(
      c_n, c_m, h_cxadj.data(), h_cadj.data(), h_cvw.data(), c_m ? h_cwgt.data() : nullptr
  );
  contract_out_free(o);
  return static_cast<i64>(c_n);
}

namespace {

// The pass of kmp_contract_engine_sparsified on the contraction's device
// output, in place (rule: include/kaminpar_lp.h). Not triggered: o is left as
// it is. One read-back, of the select's result and the kept total.
void sparsify_contract_out(
    kmp_lp_t *e, ContractOut &o, const kmp_sparsify_params_t &p, u64 seed,
    kmp_sparsify_stats_t &st
) {
  st = kmp_sparsify_stats_t{};
  const u32 c_n = o.c_n, c_m = o.c_m;
  st.m_before = c_m;
  st.m_after = c_m;
  if (c_m == 0) {
    return;
  }
  const double old_n = static_cast<double>(e->n), old_m = static_cast<double>(e->m);
  const double want = std::min(
      p.edge_target_factor * old_m, p.density_target_factor * old_m / old_n * c_n
  );
  const u64 target = want < old_m ? static_cast<u64>(want) : e->m;
  st.target = target;
  if (!(static_cast<double>(c_m) > p.laziness_factor * static_cast<double>(target)) ||
      c_m <= target) {
    return;
  }
  st.applied = 1;
  hipStream_t s = e->stream;
  hipEvent_t ev0, ev1;
  HIP_CHECK(hipEventCreate(&ev0));
  HIP_CHECK(hipEventCreate(&ev1));
  HIP_CHECK(hipEventRecord(ev0, s));
  if (target < 2) { // drop every arc; the arrays keep their size
    HIP_CHECK(hipMemsetAsync(o.d_cxadj, 0, sizeof(u64) * (static_cast<size_t>(c_n) + 1), s));
    o.c_m = 0;
    st.m_after = 0;
    HIP_CHECK(hipEventRecord(ev1, s));
  } else {
    kmp_sparsify::SelectState *d_st = nullptr;
    u32 *d_hist = nullptr, *d_lists = nullptr, *d_tiers = nullptr;
    u64 *d_cnt = nullptr;
    HIP_CHECK(hipMalloc(&d_st, sizeof(kmp_sparsify::SelectState)));
    HIP_CHECK(hipMalloc(
        &d_hist, sizeof(u32) * kmp_sparsify::kSelectPasses * kmp_sparsify::kSelectBins
    ));
    HIP_CHECK(hipMalloc(&d_lists, sizeof(u32) * 2 * c_n));
    HIP_CHECK(hipMalloc(&d_tiers, sizeof(u32) * 2));
    HIP_CHECK(hipMalloc(&d_cnt, sizeof(u64) * (static_cast<size_t>(c_n) + 1)));
    kmp_sparsify::select(o.d_cwgt, c_m, static_cast<u64>(c_m) - target + 1, d_hist, d_st, s);
    kmp_sparsify::View v{};
    v.n = c_n;
    v.xadj = o.d_cxadj;
    v.adjncy = o.d_cadj;
    v.adjwgt = o.d_cwgt;
    v.cnt = d_cnt;
    v.m_list = d_lists;
    v.l_list = d_lists + c_n;
    v.tier_counts = d_tiers;
    v.st = d_st;
    // Measurement switch (tools/sparsify_bench.py kernels --flags): count()
    // stores a byte per arc and fill() reads it instead of evaluating the rule
    // again. Same output; off unless the variable is set.
    uint8_t *d_flags = nullptr;
    if (getenv("KMP_SPARSIFY_FLAGS") != nullptr) {
      HIP_CHECK(hipMalloc(&d_flags, c_m));
    }
    v.flags = d_flags;
    v.target = target;
    v.seed = seed;
    kmp_sparsify::prepare(v, s);
    kmp_sparsify::count(v, s);
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    HIP_CHECK(rocprim::exclusive_scan(
        nullptr, tmp_bytes, d_cnt, d_cnt, u64{0}, static_cast<size_t>(c_n) + 1,
        rocprim::plus<u64>()
    ));
    HIP_CHECK(hipMalloc(&tmp, tmp_bytes > 0 ? tmp_bytes : 1));
    HIP_CHECK(rocprim::exclusive_scan(
        tmp, tmp_bytes, d_cnt, d_cnt, u64{0}, static_cast<size_t>(c_n) + 1,
        rocprim::plus<u64>(), s
    ));
    kmp_sparsify::SelectState h_st{};
    u64 kept = 0;
    HIP_CHECK(hipMemcpyAsync(&h_st, d_st, sizeof(h_st), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&kept, d_cnt + c_n, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (kept > c_m) { // cannot happen; keeps the fill inside its arrays whatever went wrong
      fprintf(stderr, "kaminpar_amd: sparsify: kept %llu of %u arcs\n",
              static_cast<unsigned long long>(kept), c_m);
      abort();
    }
    u32 *d_adj = nullptr;
    i32 *d_wgt = nullptr;
    HIP_CHECK(hipMalloc(&d_adj, sizeof(u32) * (kept > 0 ? kept : 1)));
    HIP_CHECK(hipMalloc(&d_wgt, sizeof(i32) * (kept > 0 ? kept : 1)));
    v.out_adj = d_adj;
    v.out_wgt = d_wgt;
    kmp_sparsify::fill(v, s);
    HIP_CHECK(hipEventRecord(ev1, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (void *q : {(void *)o.d_cxadj, (void *)o.d_cadj, (void *)o.d_cwgt, (void *)d_st,
                    (void *)d_hist, (void *)d_lists, (void *)d_tiers, tmp, (void *)d_flags}) {
      if (q) {
        (void)hipFree(q);
      }
    }
    o.d_cxadj = d_cnt;
    o.d_cadj = d_adj;
    o.d_cwgt = d_wgt;
    o.c_m = static_cast<u32>(kept);
    st.m_after = kept;
    st.threshold = h_st.prefix;
    st.larger = h_st.larger;
    st.equal = h_st.equal;
    st.include = target - h_st.larger;
  }
  HIP_CHECK(hipEventSynchronize(ev1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
  st.pass_ns = static_cast<u64>(static_cast<double>(ms) * 1e6);
  HIP_CHECK(hipEventDestroy(ev0));
  HIP_CHECK(hipEventDestroy(ev1));
}

// kmp_contract_engine (sparsify == nullptr) and kmp_contract_engine_sparsified.
i64 contract_engine_impl(
    kmp_lp_t *e, const u32 *clustering, u32 *mapping_out, const kmp_sparsify_params_t *sparsify,
    u64 seed, kmp_lp_t **coarse_eng_out, kmp_sparsify_stats_t *stats_out
) {
  const bool resident = clustering == nullptr;
  if (resident && e->label_kind != kmp_lp_t::kLabelsClustering) {
    fprintf(stderr, "kaminpar_amd: contract_engine: no resident clustering "
                    "(clustering == NULL needs kmp_lp_cluster first)\n");
    return -1;
  }
  ContractOut o;
  if (contract_core(e, clustering, o) != 0) {
    contract_out_free(o);
    return -1;
  }
  hipStream_t s = e->stream;
  if (sparsify != nullptr) {
    kmp_sparsify_stats_t st;
    sparsify_contract_out(e, o, *sparsify, seed, st);
    if (stats_out != nullptr) {
      *stats_out = st;
    }
  }
  const u32 c_n = o.c_n, c_m = o.c_m;

  // The host form scans the downloaded coarse xadj / vwgt for isolated
  // vertices; the resident form scans on the device (below) and moves neither.
  std::vector<u64> h_cxadj;
  std::vector<i32> h_cvw;
  if (mapping_out != nullptr) {
    HIP_CHECK(hipMemcpyAsync(mapping_out, o.d_map, label_traffic(sizeof(u32) * e->n),
                             hipMemcpyDeviceToHost, s));
  }
  if (!resident) {
    h_cxadj.resize(static_cast<size_t>(c_n) + 1);
    h_cvw.resize(c_n);
    HIP_CHECK(hipMemcpyAsync(h_cxadj.data(), o.d_cxadj, label_traffic(sizeof(u64) * (c_n + 1)),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_cvw.data(), o.d_cvw, label_traffic(sizeof(i32) * c_n),
                             hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));

  kmp_lp_t *e2 = engine_new_shell();
  engine_set_size(e2, c_n, c_m, true, true);
  e2->d_xadj = o.d_cxadj;
  e2->d_adjncy = o.d_cadj;
  e2->d_vwgt = o.d_cvw;
  e2->d_adjwgt = o.d_cwgt;
  engine_alloc_common(e2);
  if (resident) {
    engine_scan_isolated_device(e2);
  } else {
    engine_scan_isolated(e2, h_cxadj.data(), h_cvw.data());
  }
  // the child owns the mapping of its contraction (kmp_lp_project)
  e2->d_parent_map = o.d_map;
  e2->parent_addr = e;
  e2->parent_n = e->n;
  *coarse_eng_out = e2;
  return static_cast<i64>(c_n);
}

} // namespace

i64 kmp_contract_engine(
    kmp_lp_t *e, const u32 *clustering, u32 *mapping_out, kmp_lp_t **coarse_eng_out
) {
  return contract_engine_impl(e, clustering, mapping_out, nullptr, 0, coarse_eng_out, nullptr);
}

kmp_sparsify_params_t kmp_sparsify_params_default(void) {
  kmp_sparsify_params_t p;
  p.density_target_factor = 0.5;
  p.edge_target_factor = 0.5;
  p.laziness_factor = 4.0;
  return p;
}

int kmp_sparsify_params_valid(const kmp_sparsify_params_t *p) {
  return p != nullptr && std::isfinite(p->density_target_factor) &&
         p->density_target_factor > 0 && std::isfinite(p->edge_target_factor) &&
         p->edge_target_factor > 0 && std::isfinite(p->laziness_factor) &&
         p->laziness_factor >= 1;
}

i64 kmp_contract_engine_sparsified(
    kmp_lp_t *e, const u32 *clustering, u32 *mapping_out, const kmp_sparsify_params_t *params,
    u64 seed, kmp_lp_t **coarse_eng_out, kmp_sparsify_stats_t *stats_out
) {
  const kmp_sparsify_params_t p = params != nullptr ? *params : kmp_sparsify_params_default();
  if (!kmp_sparsify_params_valid(&p)) {
    fprintf(stderr, "kaminpar_amd: contract_engine_sparsified: every factor must be finite and "
                    "> 0, and laziness_factor >= 1\n");
    return -1;
  }
  return contract_engine_impl(e, clustering, mapping_out, &p, seed, coarse_eng_out, stats_out);
}

// ==================== resident labels ====================
// Rules: include/kaminpar_lp.h. The kernels are in resident_hip.hip.

int kmp_lp_set_labels(kmp_lp_t *e, u32 k, const u32 *partition) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  for (u32 u = 0; u < e->n; ++u) {
    if (partition[u] >= k) {
      fprintf(stderr, "kaminpar_amd: set_labels: partition[%u] = %u is not below k = %u\n", u,
              partition[u], k);
      return -1;
    }
  }
  HIP_CHECK(hipMemcpyAsync(e->d_labels, partition, label_traffic(sizeof(u32) * e->n),
                           hipMemcpyHostToDevice, e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->label_kind = kmp_lp_t::kLabelsPartition;
  e->label_k = k;
  e->shadows_ok = false;
  return 0;
}

int kmp_lp_get_labels(const kmp_lp_t *e, u32 *out) {
  if (e->label_kind == kmp_lp_t::kLabelsNone) {
    fprintf(stderr, "kaminpar_amd: get_labels: the engine holds no resident labels\n");
    return -1;
  }
  HIP_CHECK(hipMemcpyAsync(out, e->d_labels, label_traffic(sizeof(u32) * e->n),
                           hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  return 0;
}

int kmp_lp_project(kmp_lp_t *coarse, kmp_lp_t *fine) {
  if (coarse->d_parent_map == nullptr || coarse->parent_addr != static_cast<const void *>(fine) ||
      coarse->parent_n != fine->n) {
    fprintf(stderr, "kaminpar_amd: project: the fine engine is not the one the coarse engine "
                    "was contracted from\n");
    return -1;
  }
  if (coarse->label_kind != kmp_lp_t::kLabelsPartition) {
    fprintf(stderr, "kaminpar_amd: project: the coarse engine holds no resident partition\n");
    return -1;
  }
  fine->label_kind = kmp_lp_t::kLabelsNone;
  // Gather from the narrowest array known to equal the coarse d_labels: the
  // shadows after refine / jet / rebalance, d_labels itself otherwise.
  const void *table = coarse->d_labels;
  int label_bytes = 4;
  if (coarse->shadows_ok && coarse->label_k <= 256) {
    table = coarse->d_labels8;
    label_bytes = 1;
  } else if (coarse->shadows_ok && coarse->label_k <= kMaxDenseK) {
    table = coarse->d_labels16;
    label_bytes = 2;
  }
  // The kernel runs on the fine engine's stream: it waits for the coarse
  // stream's work so far, and the coarse stream then waits for the kernel
  // before anything later may overwrite the table.
  HIP_CHECK(hipEventRecord(coarse->sync_ev, coarse->stream));
  HIP_CHECK(hipStreamWaitEvent(fine->stream, coarse->sync_ev, 0));
  kmp_resident::project(coarse->d_parent_map, table, label_bytes, fine->n, fine->d_labels,
                        fine->stream);
  HIP_CHECK(hipEventRecord(fine->sync_ev, fine->stream));
  HIP_CHECK(hipStreamWaitEvent(coarse->stream, fine->sync_ev, 0));
  fine->label_kind = kmp_lp_t::kLabelsPartition;
  fine->label_k = coarse->label_k;
  fine->shadows_ok = false; // d_labels only; the next refine_load_state rebuilds the rest
  return 0;
}

// ==================== V-cycle pieces ====================
// Rules: include/kaminpar_lp.h. The kernels are in vcycle_hip.hip.

static int communities_ok(const kmp_lp_t *e, const char *who) {
  if (e->d_comm == nullptr) {
    fprintf(stderr, "kaminpar_amd: %s: the engine has no communities\n", who);
    return -1;
  }
  if (e->comm_k > KMP_LP_MAX_K) {
    fprintf(stderr, "kaminpar_amd: %s: community ids up to %llu are no partition (k <= %u)\n",
            who, static_cast<unsigned long long>(e->comm_k - 1), static_cast<u32>(KMP_LP_MAX_K));
    return -1;
  }
  return 0;
}

int kmp_lp_restrict(kmp_lp_t *fine, kmp_lp_t *coarse) {
  if (coarse->d_parent_map == nullptr || coarse->parent_addr != static_cast<const void *>(fine) ||
      coarse->parent_n != fine->n) {
    fprintf(stderr, "kaminpar_amd: restrict: the coarse engine was not contracted from the fine "
                    "engine\n");
    return -1;
  }
  if (communities_ok(fine, "restrict") != 0) {
    return -1;
  }
  coarse->label_kind = kmp_lp_t::kLabelsNone;
  // The kernels run on the coarse engine's stream: they wait for the fine
  // stream's work so far (the communities), and the fine stream then waits
  // for them before anything later may replace the communities.
  HIP_CHECK(hipEventRecord(fine->sync_ev, fine->stream));
  HIP_CHECK(hipStreamWaitEvent(coarse->stream, fine->sync_ev, 0));
  kmp_vcycle::restrict_labels(coarse->d_parent_map, fine->d_comm, fine->n, coarse->d_labels,
                              coarse->n, coarse->stream);
  kmp_vcycle::restrict_mismatches(coarse->d_parent_map, fine->d_comm, fine->n, coarse->d_labels,
                                  coarse->n, coarse->d_cut, coarse->stream);
  unsigned long long bad = 0;
  HIP_CHECK(hipMemcpyAsync(&bad, coarse->d_cut, sizeof(bad), hipMemcpyDeviceToHost,
                           coarse->stream));
  HIP_CHECK(hipEventRecord(coarse->sync_ev, coarse->stream));
  HIP_CHECK(hipStreamWaitEvent(fine->stream, coarse->sync_ev, 0));
  HIP_CHECK(hipStreamSynchronize(coarse->stream));
  if (bad != 0) {
    fprintf(stderr, "kaminpar_amd: restrict: %llu fine vertices share a coarse vertex with a "
                    "vertex of another community (the clustering does not respect the "
                    "communities)\n", bad);
    return -1;
  }
  coarse->label_kind = kmp_lp_t::kLabelsPartition;
  coarse->label_k = static_cast<u32>(fine->comm_k);
  coarse->shadows_ok = false; // d_labels only; the next refine_load_state rebuilds the rest
  return 0;
}

int kmp_lp_labels_from_communities(kmp_lp_t *e) {
  if (communities_ok(e, "labels_from_communities") != 0) {
    return -1;
  }
  e->label_kind = kmp_lp_t::kLabelsNone;
  HIP_CHECK(hipMemcpyAsync(e->d_labels, e->d_comm, sizeof(u32) * e->n, hipMemcpyDeviceToDevice,
                           e->stream));
  if (e->n > 0) {
    const u32 threads = 256;
    hipLaunchKernelGGL(k_sync_labels16, dim3(ceil_div(e->n, threads)), dim3(threads), 0, e->stream,
                       e->n, e->d_labels, e->d_labels16, e->d_labels8);
    LAUNCH_CHECK();
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->label_kind = kmp_lp_t::kLabelsPartition;
  e->label_k = static_cast<u32>(e->comm_k);
  e->shadows_ok = e->comm_k <= 65536;
  return 0;
}

i64 kmp_lp_resident_cut(kmp_lp_t *e, u32 k, const i64 *max_block_weights, int32_t *feasible) {
  if (resident_partition_ok(e, k, "resident_cut") != 0) {
    return -1;
  }
  if (feasible != nullptr && max_block_weights == nullptr) {
    fprintf(stderr, "kaminpar_amd: resident_cut: feasibility needs max_block_weights\n");
    return -1;
  }
  HIP_CHECK(hipMemsetAsync(e->d_cut, 0, sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(
      k_edge_cut, dim3(32768), dim3(256), 0, e->stream, e->n, e->d_xadj, e->d_adjncy, e->d_adjwgt,
      e->d_labels, e->d_cut
  );
  LAUNCH_CHECK();
  unsigned long long cut2 = 0;
  std::vector<unsigned long long> w;
  HIP_CHECK(hipMemcpyAsync(&cut2, e->d_cut, sizeof(cut2), hipMemcpyDeviceToHost, e->stream));
  if (feasible != nullptr) { // the block-weight pass runs only where it is asked for
    auto *d_w =
        static_cast<unsigned long long *>(vc_scratch(e, sizeof(unsigned long long) * k));
    w.resize(k);
    kmp_vcycle::block_weights(e->d_labels, e->d_vwgt, e->n, k, d_w, e->stream);
    HIP_CHECK(hipMemcpyAsync(w.data(), d_w, sizeof(unsigned long long) * k, hipMemcpyDeviceToHost,
                             e->stream));
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  if (feasible != nullptr) {
    *feasible = 1;
    for (u32 b = 0; b < k; ++b) {
      if (static_cast<i64>(w[b]) > max_block_weights[b]) {
        *feasible = 0;
        break;
      }
    }
  }
  return static_cast<i64>(cut2 / 2);
}

uint64_t kmp_lp_label_traffic_bytes(void) {
  return g_label_traffic.load(std::memory_order_relaxed);
}

kmp_graph_t *kmp_lp_download_graph(const kmp_lp_t *e) {
  if (e->m > 0xFFFFFFFFull) {
    fprintf(stderr, "kaminpar_amd: kmp_lp_download_graph supports m < 2^32\n");
    return nullptr;
  }
  std::vector<u64> h_xadj64(e->n + 1);
  std::vector<u32> h_xadj(e->n + 1), h_adj(e->m);
  std::vector<i32> h_vw, h_wg;
  HIP_CHECK(
      hipMemcpy(h_xadj64.data(), e->d_xadj, sizeof(u64) * (e->n + 1), hipMemcpyDeviceToHost)
  );
  for (u32 i = 0; i <= e->n; ++i) {
    h_xadj[i] = static_cast<u32>(h_xadj64[i]);
  }
  HIP_CHECK(hipMemcpy(h_adj.data(), e->d_adjncy, sizeof(u32) * e->m, hipMemcpyDeviceToHost));
  if (e->has_vwgt) {
    h_vw.resize(e->n);
    HIP_CHECK(hipMemcpy(h_vw.data(), e->d_vwgt, sizeof(i32) * e->n, hipMemcpyDeviceToHost));
  }
  if (e->has_adjwgt) {
    h_wg.resize(e->m);
    HIP_CHECK(hipMemcpy(h_wg.data(), e->d_adjwgt, sizeof(i32) * e->m, hipMemcpyDeviceToHost));
  }
  return kmp_graph_from_csr(
      e->n, e->m, h_xadj.data(), h_adj.data(), e->has_vwgt ? h_vw.data() : nullptr,
      e->has_adjwgt ? h_wg.data() : nullptr
  );
}

// ==================== engines from edge lists (GPU) ====================
// Driver of kmp_lp_create_from_edges (rule: include/kaminpar_lp.h; kernels:
// edges_hip.hip). Three host reads when n is given: the error counters after
// the pack, the number of collapsed arcs, the isolated scan. An inferred n
// costs one more, before the pack, because the key width depends on n.

extern "C++" {
namespace {

// Device temporaries of one build, with the running and the largest sum of
// their sizes (kmp_edges_stats_t::peak_bytes).
struct EdgeTemps {
  std::vector<std::pair<void *, size_t>> live;
  size_t cur = 0, peak = 0;

  template <typename T>
  T *alloc(size_t count) {
    const size_t bytes = sizeof(T) * count;
    void *p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes > 0 ? bytes : 1));
    live.emplace_back(p, bytes);
    cur += bytes;
    peak = std::max(peak, cur);
    return static_cast<T *>(p);
  }
  void release(const void *p) {
    for (size_t i = 0; i < live.size(); ++i) {
      if (live[i].first == p) {
        HIP_CHECK(hipFree(live[i].first));
        cur -= live[i].second;
        live.erase(live.begin() + static_cast<std::ptrdiff_t>(i));
        return;
      }
    }
  }
  void release_all() {
    for (auto &a : live) {
      HIP_CHECK(hipFree(a.first));
    }
    live.clear();
    cur = 0;
  }
};

u64 event_ns(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  return static_cast<u64>(static_cast<double>(ms) * 1e6);
}

} // namespace
} // extern "C++"

kmp_lp_t *kmp_lp_create_from_edges(
    u32 n, u64 num_pairs, const void *src, const void *dst, const i32 *weights, const i32 *vwgt,
    u32 flags, kmp_edges_stats_t *stats_out
) {
  const u32 known = KMP_EDGES_DEVICE | KMP_EDGES_IDS64 | KMP_EDGES_SUM | KMP_EDGES_SORT64 |
                    KMP_EDGES_IDS_I32;
  if ((flags & ~known) != 0 || ((flags & KMP_EDGES_IDS64) && (flags & KMP_EDGES_IDS_I32))) {
    fprintf(stderr, "kaminpar_amd: create_from_edges: invalid flags 0x%x\n", flags);
    return nullptr;
  }
  if (n == 0 && num_pairs == 0) {
    fprintf(stderr, "kaminpar_amd: create_from_edges: n = 0 and no pairs to infer it from\n");
    return nullptr;
  }
  if (n == 0 && vwgt != nullptr) {
    fprintf(stderr, "kaminpar_amd: create_from_edges: vwgt needs n (its length cannot be "
                    "inferred)\n");
    return nullptr;
  }
  if (2 * num_pairs >= (1ull << 32) || num_pairs >= (1ull << 63)) {
    fprintf(stderr, "kaminpar_amd: create_from_edges: %llu pairs; 2 * pairs must stay below 2^32\n",
            static_cast<unsigned long long>(num_pairs));
    return nullptr;
  }
  if (num_pairs > 0 && (src == nullptr || dst == nullptr)) {
    fprintf(stderr, "kaminpar_amd: create_from_edges: src / dst is NULL\n");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fprintf(stderr, "kaminpar_amd: no HIP device available -- the LP engine requires a GPU\n");
    return nullptr;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const bool on_device = (flags & KMP_EDGES_DEVICE) != 0;
  const bool weighted = weights != nullptr && num_pairs > 0;
  const bool sum = (flags & KMP_EDGES_SUM) != 0;
  const kmp_edges::IdKind kind = (flags & KMP_EDGES_IDS64)    ? kmp_edges::kIdsI64
                                 : (flags & KMP_EDGES_IDS_I32) ? kmp_edges::kIdsI32
                                                               : kmp_edges::kIdsU32;
  const size_t id_bytes = kind == kmp_edges::kIdsI64 ? 8 : 4;
  const hipMemcpyKind to_device = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;

  (void)hipSetDeviceFlags(hipDeviceScheduleSpin); // ignore if context exists
  kmp_lp_t *e = engine_new_shell();
  hipStream_t s = e->stream;
  constexpr int kEvents = 8; // pack, sort, collapse, build: begin / end each
  hipEvent_t ev[kEvents];
  for (hipEvent_t &x : ev) {
    HIP_CHECK(hipEventCreate(&x));
  }
  EdgeTemps tmp;
  // Every error return: nothing stays allocated.
  auto fail = [&]() -> kmp_lp_t * {
    HIP_CHECK(hipStreamSynchronize(s));
    tmp.release_all();
    for (hipEvent_t x : ev) {
      (void)hipEventDestroy(x);
    }
    for (void *p : {(void *)e->d_xadj, (void *)e->d_adjncy, (void *)e->d_adjwgt}) {
      if (p) {
        (void)hipFree(p);
      }
    }
    (void)hipEventDestroy(e->sync_ev);
    (void)hipStreamDestroy(s);
    delete e;
    return nullptr;
  };

  // host pointers: one staged upload, the same path afterwards
  const void *d_src = src, *d_dst = dst;
  const i32 *d_w = weighted ? weights : nullptr;
  void *st_src = nullptr, *st_dst = nullptr;
  i32 *st_w = nullptr;
  if (!on_device && num_pairs > 0) {
    st_src = tmp.alloc<uint8_t>(id_bytes * num_pairs);
    st_dst = tmp.alloc<uint8_t>(id_bytes * num_pairs);
    HIP_CHECK(hipMemcpyAsync(st_src, src, id_bytes * num_pairs, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st_dst, dst, id_bytes * num_pairs, hipMemcpyHostToDevice, s));
    d_src = st_src;
    d_dst = st_dst;
    if (weighted) {
      st_w = tmp.alloc<i32>(num_pairs);
      HIP_CHECK(hipMemcpyAsync(st_w, weights, sizeof(i32) * num_pairs, hipMemcpyHostToDevice, s));
      d_w = st_w;
    }
  }
  u64 *d_cnt = tmp.alloc<u64>(kmp_edges::kNumCounters);
  u32 *d_uniq = tmp.alloc<u32>(1);
  u64 h_cnt[kmp_edges::kNumCounters] = {};
  HIP_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(h_cnt), s));

  if (n == 0) {
    kmp_edges::scan_ids(d_src, d_dst, kind, num_pairs, d_cnt, s);
    HIP_CHECK(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_cnt[kmp_edges::kBadIds] > 0 || h_cnt[kmp_edges::kMaxId] >= 0xFFFFFFFFull) {
      fprintf(stderr, "kaminpar_amd: create_from_edges: %llu pairs with an id that is negative "
                      "or too large (largest id seen: %llu)\n",
              static_cast<unsigned long long>(h_cnt[kmp_edges::kBadIds]),
              static_cast<unsigned long long>(h_cnt[kmp_edges::kMaxId]));
      return fail();
    }
    n = static_cast<u32>(h_cnt[kmp_edges::kMaxId]) + 1;
    HIP_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(h_cnt), s));
  }
  const u32 bits = kmp_edges::key_bits(n);
  const u64 arcs2 = 2 * num_pairs;

  u64 *keys[2] = {nullptr, nullptr};
  i32 *vals[2] = {nullptr, nullptr};
  u64 self_loops = 0;
  u32 m = 0;
  int cur = 0;
  if (num_pairs > 0) {
    keys[0] = tmp.alloc<u64>(arcs2);
    if (weighted) {
      vals[0] = tmp.alloc<i32>(arcs2);
    }
    HIP_CHECK(hipEventRecord(ev[0], s));
    kmp_edges::pack(d_src, d_dst, kind, d_w, num_pairs, n, keys[0], vals[0], d_cnt, s);
    HIP_CHECK(hipEventRecord(ev[1], s));
    HIP_CHECK(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s)); // host read 1: nothing was indexed by an id so far
    if (h_cnt[kmp_edges::kBadIds] > 0) {
      fprintf(stderr, "kaminpar_amd: create_from_edges: %llu pairs with an id that is negative "
                      "or not below n = %u\n",
              static_cast<unsigned long long>(h_cnt[kmp_edges::kBadIds]), n);
      return fail();
    }
    if (h_cnt[kmp_edges::kBadWeights] > 0) {
      fprintf(stderr, "kaminpar_amd: create_from_edges: %llu pairs with a weight <= 0\n",
              static_cast<unsigned long long>(h_cnt[kmp_edges::kBadWeights]));
      return fail();
    }
    self_loops = h_cnt[kmp_edges::kSelfLoops];
    // the staged input is dead: the peak is the sort's, not the sum
    tmp.release(st_src);
    tmp.release(st_dst);
    tmp.release(st_w);

    keys[1] = tmp.alloc<u64>(arcs2);
    if (weighted) {
      vals[1] = tmp.alloc<i32>(arcs2);
    }
    const u32 end_bit = (flags & KMP_EDGES_SORT64) ? 64 : 2 * bits;
    size_t sort_bytes = 0, coll_bytes = 0;
    kmp_edges::sort(nullptr, sort_bytes, keys, vals, arcs2, end_bit, s);
    kmp_edges::collapse(nullptr, coll_bytes, keys[0], vals[0], arcs2, sum, keys[1], vals[1],
                        d_uniq, s);
    void *d_tmp = tmp.alloc<uint8_t>(std::max(sort_bytes, coll_bytes));
    HIP_CHECK(hipEventRecord(ev[2], s));
    cur = kmp_edges::sort(d_tmp, sort_bytes, keys, vals, arcs2, end_bit, s);
    HIP_CHECK(hipEventRecord(ev[3], s));
    // runs of equal keys collapse into the buffer the sort left free
    HIP_CHECK(hipEventRecord(ev[4], s));
    kmp_edges::collapse(d_tmp, coll_bytes, keys[cur], vals[cur], arcs2, sum, keys[cur ^ 1],
                        vals[cur ^ 1], d_uniq, s);
    if (weighted && sum) {
      kmp_edges::check_sums(vals[cur ^ 1], d_uniq, d_cnt, s);
    }
    HIP_CHECK(hipEventRecord(ev[5], s));
    u32 uniq = 0;
    HIP_CHECK(hipMemcpyAsync(&uniq, d_uniq, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s)); // host read 2
    if (h_cnt[kmp_edges::kOverflow] > 0) {
      fprintf(stderr, "kaminpar_amd: create_from_edges: %llu arcs whose summed weight exceeds "
                      "2^31 - 1\n",
              static_cast<unsigned long long>(h_cnt[kmp_edges::kOverflow]));
      return fail();
    }
    // all self-loops share the dropped key, which sorts last: one run
    m = uniq - (self_loops > 0 ? 1u : 0u);
    tmp.release(d_tmp);
    tmp.release(keys[cur]);
    tmp.release(vals[cur]);
  } else {
    for (int i = 0; i < 6; ++i) {
      HIP_CHECK(hipEventRecord(ev[i], s));
    }
  }

  // right-sized arrays of the engine
  const size_t mm = m > 0 ? m : 1;
  HIP_CHECK(hipMalloc(&e->d_xadj, sizeof(u64) * (static_cast<size_t>(n) + 1)));
  HIP_CHECK(hipMalloc(&e->d_adjncy, sizeof(u32) * mm));
  if (weighted) {
    HIP_CHECK(hipMalloc(&e->d_adjwgt, sizeof(i32) * mm));
  }
  size_t scan_bytes = 0;
  kmp_edges::build(nullptr, scan_bytes, nullptr, nullptr, m, n, e->d_xadj, nullptr, nullptr, s);
  void *d_scan = tmp.alloc<uint8_t>(scan_bytes);
  HIP_CHECK(hipEventRecord(ev[6], s));
  kmp_edges::build(d_scan, scan_bytes, keys[cur ^ 1], weighted ? vals[cur ^ 1] : nullptr, m, n,
                   e->d_xadj, e->d_adjncy, e->d_adjwgt, s);
  HIP_CHECK(hipEventRecord(ev[7], s));
  HIP_CHECK(hipStreamSynchronize(s));
  const size_t peak = tmp.peak;
  tmp.release_all(); // before the engine's own buffers: the peak is the sort's

  engine_set_size(e, n, m, vwgt != nullptr, weighted);
  if (e->has_vwgt) {
    HIP_CHECK(hipMalloc(&e->d_vwgt, sizeof(i32) * n));
    HIP_CHECK(hipMemcpyAsync(e->d_vwgt, vwgt, sizeof(i32) * n, to_device, s));
  }
  engine_alloc_common(e);
  engine_scan_isolated_device(e); // host read 3

  if (stats_out != nullptr) {
    kmp_edges_stats_t st;
    memset(&st, 0, sizeof(st));
    st.pairs = num_pairs;
    st.self_loops = self_loops;
    st.arcs = m;
    st.merged_arcs = 2 * (num_pairs - self_loops) - m;
    st.n = n;
    st.isolated = static_cast<u32>(e->isolated.size());
    st.max_degree = e->max_deg;
    st.pack_ns = event_ns(ev[0], ev[1]);
    st.sort_ns = event_ns(ev[2], ev[3]);
    st.build_ns = event_ns(ev[4], ev[5]) + event_ns(ev[6], ev[7]);
    st.total_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                       std::chrono::steady_clock::now() - t0)
                                       .count());
    st.peak_bytes = peak;
    *stats_out = st;
  }
  for (hipEvent_t x : ev) {
    (void)hipEventDestroy(x);
  }
  return e;
}

int kmp_lp_get_labels_device(const kmp_lp_t *e, u32 *dst_device) {
  if (e->label_kind == kmp_lp_t::kLabelsNone) {
    fprintf(stderr, "kaminpar_amd: get_labels_device: the engine holds no resident labels\n");
    return -1;
  }
  HIP_CHECK(hipMemcpyAsync(dst_device, e->d_labels, sizeof(u32) * e->n, hipMemcpyDeviceToDevice,
                           e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
  return 0;
}

// ==================== block subgraph extraction (GPU) ====================
// Driver of kmp_lp_extract_subgraphs (rule: include/kaminpar_lp.h; kernels:
// extract_hip.hip). The partition lives in scratch owned by the call; the
// engine's own label state is not touched.

struct kmp_subgraphs_t {
  u32 n = 0;
  u32 k = 0;
  bool has_vwgt = false, has_adjwgt = false;
  int mp_count = 0;
  u32 *d_nodes = nullptr;     // n
  u64 *d_sub_xadj = nullptr;  // n + 1
  u32 *d_sub_adj = nullptr;   // internal arcs
  i32 *d_sub_adjwgt = nullptr;
  i32 *d_sub_vwgt = nullptr;  // n
  std::vector<u32> node_off;  // k + 1
  std::vector<u64> arc_off;   // k + 1
};

void kmp_subgraphs_free(kmp_subgraphs_t *s) {
  if (!s) {
    return;
  }
  for (void *p : {(void *)s->d_nodes, (void *)s->d_sub_xadj, (void *)s->d_sub_adj,
                  (void *)s->d_sub_adjwgt, (void *)s->d_sub_vwgt}) {
    if (p) {
      (void)hipFree(p);
    }
  }
  delete s;
}

kmp_subgraphs_t *kmp_lp_extract_subgraphs(
    kmp_lp_t *e, u32 k, const u32 *partition, u32 *mapping_out, kmp_extract_stats_t *stats
) {
  if (k < 1 || k > kMaxDenseK) {
    fprintf(stderr, "kaminpar_amd: extract: k = %u is not in 1..%u\n", k, kMaxDenseK);
    return nullptr;
  }
  if (e->m > 0xFFFFFFFFull) {
    fprintf(stderr, "kaminpar_amd: extract supports m < 2^32 arcs\n");
    return nullptr;
  }
  const auto wall0 = std::chrono::steady_clock::now();
  const u32 n = e->n;
  const size_t nn = n > 0 ? n : 1;
  hipStream_t s = e->stream;

  auto *out = new kmp_subgraphs_t();
  out->n = n;
  out->k = k;
  out->has_vwgt = e->has_vwgt;
  out->has_adjwgt = e->has_adjwgt;
  out->mp_count = e->mp_count;
  out->node_off.assign(static_cast<size_t>(k) + 1, 0);
  out->arc_off.assign(static_cast<size_t>(k) + 1, 0);
  HIP_CHECK(hipMalloc(&out->d_sub_xadj, sizeof(u64) * (nn + 1)));
  HIP_CHECK(hipMemsetAsync(out->d_sub_xadj, 0, sizeof(u64) * (nn + 1), s));
  if (n == 0) {
    HIP_CHECK(hipStreamSynchronize(s));
    if (stats) {
      *stats = kmp_extract_stats_t{};
    }
    return out;
  }

  // scratch of the call
  u32 *d_keys[2] = {nullptr, nullptr}, *d_vals[2] = {nullptr, nullptr};
  u32 *d_deg_in = nullptr, *d_pos = nullptr, *d_mapping = nullptr, *d_m_list = nullptr,
      *d_l_list = nullptr, *d_tier = nullptr, *d_node_cnt = nullptr, *d_node_off = nullptr;
  uint16_t *d_lab16 = nullptr;
  uint8_t *d_lab8 = nullptr;
  unsigned long long *d_arc_cnt = nullptr, *d_arcs = nullptr;
  void *sort_tmp = nullptr, *scan_tmp = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (auto &x : ev) {
    HIP_CHECK(hipEventCreate(&x));
  }
  HIP_CHECK(hipMalloc(&d_keys[0], sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_keys[1], sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_vals[0], sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_vals[1], sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_deg_in, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_pos, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_mapping, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_m_list, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_l_list, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_tier, sizeof(u32) * 3));
  HIP_CHECK(hipMalloc(&d_node_cnt, sizeof(u32) * k));
  HIP_CHECK(hipMalloc(&d_node_off, sizeof(u32) * (k + 1)));
  HIP_CHECK(hipMalloc(&d_lab16, sizeof(uint16_t) * n));
  HIP_CHECK(hipMalloc(&d_lab8, n));
  HIP_CHECK(hipMalloc(&d_arc_cnt, sizeof(unsigned long long) * k));
  HIP_CHECK(hipMalloc(&d_arcs, sizeof(unsigned long long)));
  if (e->has_vwgt) {
    HIP_CHECK(hipMalloc(&out->d_sub_vwgt, sizeof(i32) * n));
  }
  auto free_scratch = [&]() {
    for (void *p : {(void *)d_keys[0], (void *)d_keys[1], (void *)d_vals[0], (void *)d_vals[1],
                    (void *)d_deg_in, (void *)d_pos, (void *)d_mapping, (void *)d_m_list,
                    (void *)d_l_list, (void *)d_tier, (void *)d_node_cnt, (void *)d_node_off,
                    (void *)d_lab16, (void *)d_lab8, (void *)d_arc_cnt, (void *)d_arcs, sort_tmp,
                    scan_tmp}) {
      if (p) {
        (void)hipFree(p);
      }
    }
    for (hipEvent_t x : ev) {
      (void)hipEventDestroy(x);
    }
  };

  // the uploaded labels double as the sort keys: after prepare the arc passes
  // read the shadows only
  HIP_CHECK(hipMemcpyAsync(d_keys[0], partition, sizeof(u32) * n, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(d_arcs, 0, sizeof(unsigned long long), s));

  kmp_extract::View v{};
  v.n = n;
  v.k = k;
  v.xadj = e->d_xadj;
  v.adjncy = e->d_adjncy;
  v.adjwgt = e->d_adjwgt;
  v.vwgt = e->d_vwgt;
  v.labels = d_keys[0];
  v.labels16 = d_lab16;
  v.labels8 = d_lab8;
  v.deg_in = d_deg_in;
  v.m_list = d_m_list;
  v.l_list = d_l_list;
  v.tier_counts = d_tier;
  v.node_cnt = d_node_cnt;
  v.arc_cnt = d_arc_cnt;
  v.arcs = d_arcs;
  v.node_off = d_node_off;
  v.pos = d_pos;
  v.mapping = d_mapping;
  v.sub_xadj = out->d_sub_xadj;
  v.sub_vwgt = out->d_sub_vwgt;

  kmp_extract::prepare(v, s);
  u32 tier[3] = {0, 0, 0};
  std::vector<u32> node_cnt(k);
  HIP_CHECK(hipMemcpyAsync(tier, d_tier, sizeof(tier), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(node_cnt.data(), d_node_cnt, sizeof(u32) * k, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (tier[2] > 0) {
    fprintf(stderr, "kaminpar_amd: extract: %u labels are not below k = %u\n", tier[2], k);
    free_scratch();
    kmp_subgraphs_free(out);
    return nullptr;
  }
  for (u32 b = 0; b < k; ++b) {
    out->node_off[b + 1] = out->node_off[b] + node_cnt[b];
  }
  HIP_CHECK(hipMemcpyAsync(d_node_off, out->node_off.data(), sizeof(u32) * (k + 1),
                           hipMemcpyHostToDevice, s));

  // count pass
  HIP_CHECK(hipEventRecord(ev[0], s));
  kmp_extract::count(v, tier[0], tier[1], s);
  HIP_CHECK(hipEventRecord(ev[1], s));

  // order pass: stable sort of (label, id) on ceil_log2(k) key bits
  unsigned key_bits = 1;
  while ((1u << key_bits) < k) {
    ++key_bits;
  }
  kmp_extract::iota(n, d_vals[0], s);
  rocprim::double_buffer<u32> kb(d_keys[0], d_keys[1]);
  rocprim::double_buffer<u32> vb(d_vals[0], d_vals[1]);
  size_t sort_bytes = 0, scan_bytes = 0;
  HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, kb, vb, n, 0, key_bits));
  HIP_CHECK(hipMalloc(&sort_tmp, sort_bytes));
  HIP_CHECK(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, kb, vb, n, 0, key_bits, s));
  v.nodes = vb.current();
  kmp_extract::place(v, kb.current(), s);
  HIP_CHECK(rocprim::exclusive_scan(
      nullptr, scan_bytes, out->d_sub_xadj, out->d_sub_xadj, u64{0}, static_cast<size_t>(n) + 1,
      rocprim::plus<u64>()
  ));
  HIP_CHECK(hipMalloc(&scan_tmp, scan_bytes));
  HIP_CHECK(rocprim::exclusive_scan(
      scan_tmp, scan_bytes, out->d_sub_xadj, out->d_sub_xadj, u64{0}, static_cast<size_t>(n) + 1,
      rocprim::plus<u64>(), s
  ));

  std::vector<unsigned long long> arc_cnt(k);
  u64 m_sub = 0;
  HIP_CHECK(hipMemcpyAsync(arc_cnt.data(), d_arc_cnt, sizeof(unsigned long long) * k,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&m_sub, out->d_sub_xadj + n, sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (u32 b = 0; b < k; ++b) {
    out->arc_off[b + 1] = out->arc_off[b] + arc_cnt[b];
  }
  if (out->arc_off[k] != m_sub || m_sub > e->m) {
    // the fill pass writes at these offsets: never launch it on a mismatch
    fprintf(stderr, "kaminpar_amd: extract: block arc counts (%llu) and row offsets (%llu) "
                    "disagree\n",
            static_cast<unsigned long long>(out->arc_off[k]),
            static_cast<unsigned long long>(m_sub));
    free_scratch();
    kmp_subgraphs_free(out);
    return nullptr;
  }
  HIP_CHECK(hipMalloc(&out->d_sub_adj, sizeof(u32) * (m_sub > 0 ? m_sub : 1)));
  if (e->has_adjwgt) {
    HIP_CHECK(hipMalloc(&out->d_sub_adjwgt, sizeof(i32) * (m_sub > 0 ? m_sub : 1)));
  }
  v.sub_adj = out->d_sub_adj;
  v.sub_adjwgt = out->d_sub_adjwgt;

  // fill pass
  HIP_CHECK(hipEventRecord(ev[2], s));
  kmp_extract::fill(v, tier[0], tier[1], s);
  HIP_CHECK(hipEventRecord(ev[3], s));

  unsigned long long arcs = 0;
  HIP_CHECK(hipMemcpyAsync(&arcs, d_arcs, sizeof(arcs), hipMemcpyDeviceToHost, s));
  if (mapping_out) {
    HIP_CHECK(hipMemcpyAsync(mapping_out, d_mapping, sizeof(u32) * n, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));

  // the handle keeps the sorted ids; everything else of the call goes
  out->d_nodes = vb.current();
  (vb.current() == d_vals[0] ? d_vals[0] : d_vals[1]) = nullptr;
  if (stats) {
    float count_ms = 0, fill_ms = 0;
    HIP_CHECK(hipEventElapsedTime(&count_ms, ev[0], ev[1]));
    HIP_CHECK(hipEventElapsedTime(&fill_ms, ev[2], ev[3]));
    kmp_extract_stats_t st{};
    st.arcs_scanned = arcs;
    st.count_ns = static_cast<u64>(count_ms * 1e6);
    st.fill_ns = static_cast<u64>(fill_ms * 1e6);
    st.total_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                       std::chrono::steady_clock::now() - wall0)
                                       .count());
    *stats = st;
  }
  free_scratch();
  return out;
}

u32 kmp_subgraphs_k(const kmp_subgraphs_t *s) { return s->k; }

int kmp_subgraphs_layout(
    const kmp_subgraphs_t *s, u32 *nodes_out, u32 *node_off_out, u64 *arc_off_out
) {
  if (nodes_out && s->n > 0) {
    HIP_CHECK(hipMemcpy(nodes_out, s->d_nodes, sizeof(u32) * s->n, hipMemcpyDeviceToHost));
  }
  if (node_off_out) {
    memcpy(node_off_out, s->node_off.data(), sizeof(u32) * (s->k + 1));
  }
  if (arc_off_out) {
    memcpy(arc_off_out, s->arc_off.data(), sizeof(u64) * (s->k + 1));
  }
  return 0;
}

kmp_graph_t *kmp_subgraphs_download(const kmp_subgraphs_t *s, u32 b) {
  if (b >= s->k) {
    fprintf(stderr, "kaminpar_amd: subgraphs: block %u is not below k = %u\n", b, s->k);
    return nullptr;
  }
  const u32 first = s->node_off[b];
  const u32 bn = s->node_off[b + 1] - first;
  const u64 base = s->arc_off[b];
  const u64 bm = s->arc_off[b + 1] - base;
  std::vector<u64> x64(static_cast<size_t>(bn) + 1);
  std::vector<u32> x32(static_cast<size_t>(bn) + 1, 0), adj(bm > 0 ? bm : 1);
  std::vector<i32> vw(bn > 0 ? bn : 1), aw(bm > 0 ? bm : 1);
  HIP_CHECK(hipMemcpy(x64.data(), s->d_sub_xadj + first, sizeof(u64) * (bn + 1),
                      hipMemcpyDeviceToHost));
  for (u32 i = 0; i <= bn; ++i) {
    x32[i] = static_cast<u32>(x64[i] - base); // bm <= m < 2^32
  }
  if (bm > 0) {
    HIP_CHECK(hipMemcpy(adj.data(), s->d_sub_adj + base, sizeof(u32) * bm, hipMemcpyDeviceToHost));
    if (s->has_adjwgt) {
      HIP_CHECK(
          hipMemcpy(aw.data(), s->d_sub_adjwgt + base, sizeof(i32) * bm, hipMemcpyDeviceToHost)
      );
    }
  }
  if (bn > 0 && s->has_vwgt) {
    HIP_CHECK(hipMemcpy(vw.data(), s->d_sub_vwgt + first, sizeof(i32) * bn, hipMemcpyDeviceToHost));
  }
  return kmp_graph_from_csr(
      bn, bm, x32.data(), adj.data(), s->has_vwgt ? vw.data() : nullptr,
      s->has_adjwgt ? aw.data() : nullptr
  );
}

kmp_lp_t *kmp_subgraphs_engine(const kmp_subgraphs_t *s, u32 b) {
  if (b >= s->k) {
    fprintf(stderr, "kaminpar_amd: subgraphs: block %u is not below k = %u\n", b, s->k);
    return nullptr;
  }
  const u32 first = s->node_off[b];
  const u32 bn = s->node_off[b + 1] - first;
  const u64 base = s->arc_off[b];
  const u64 bm = s->arc_off[b + 1] - base;
  if (bn == 0) {
    return nullptr; // empty block
  }
  kmp_lp_t *e2 = engine_new_shell();
  engine_set_size(e2, bn, bm, s->has_vwgt, s->has_adjwgt);
  hipStream_t st = e2->stream;

  const size_t mm = bm > 0 ? bm : 1;
  HIP_CHECK(hipMalloc(&e2->d_xadj, sizeof(u64) * (static_cast<size_t>(bn) + 1)));
  HIP_CHECK(hipMalloc(&e2->d_adjncy, sizeof(u32) * mm));
  kmp_extract::rebase_xadj(s->d_sub_xadj, first, base, bn, e2->d_xadj, st);
  if (bm > 0) {
    HIP_CHECK(hipMemcpyAsync(e2->d_adjncy, s->d_sub_adj + base, sizeof(u32) * bm,
                             hipMemcpyDeviceToDevice, st));
  }
  if (s->has_vwgt) {
    HIP_CHECK(hipMalloc(&e2->d_vwgt, sizeof(i32) * bn));
    HIP_CHECK(hipMemcpyAsync(e2->d_vwgt, s->d_sub_vwgt + first, sizeof(i32) * bn,
                             hipMemcpyDeviceToDevice, st));
  }
  if (s->has_adjwgt) {
    HIP_CHECK(hipMalloc(&e2->d_adjwgt, sizeof(i32) * mm));
    if (bm > 0) {
      HIP_CHECK(hipMemcpyAsync(e2->d_adjwgt, s->d_sub_adjwgt + base, sizeof(i32) * bm,
                               hipMemcpyDeviceToDevice, st));
    }
  }
  // host copies for the isolated-vertex scan of the new engine
  std::vector<u64> h_xadj(static_cast<size_t>(bn) + 1);
  std::vector<i32> h_vw;
  HIP_CHECK(hipMemcpyAsync(h_xadj.data(), e2->d_xadj, sizeof(u64) * (bn + 1),
                           hipMemcpyDeviceToHost, st));
  if (s->has_vwgt) {
    h_vw.resize(bn);
    HIP_CHECK(hipMemcpyAsync(h_vw.data(), e2->d_vwgt, sizeof(i32) * bn, hipMemcpyDeviceToHost, st));
  }
  HIP_CHECK(hipStreamSynchronize(st));
  engine_alloc_common(e2);
  engine_scan_isolated(e2, h_xadj.data(), s->has_vwgt ? h_vw.data() : nullptr);
  return e2;
}

// On-GPU degree-bucket rearrangement (the reference's default
// NodeOrdering::DEGREE_BUCKETS preprocessing, graphutils/permutator.cc:36-110;
// bit-identical to the host kmp_rearrange_degree_buckets): rebuilds the
// engine's device CSR in bucket order and writes perm_out[u_old] = u_new.
// Call before any refine/cluster; LP state is reset by the next *_begin.
int kmp_lp_rearrange_degree_buckets(kmp_lp_t *e, u32 *perm_out) {
  e->label_kind = kmp_lp_t::kLabelsNone;
  const u32 n = e->n;
  const u64 m = e->m;
  const u32 threads = 256;
  hipStream_t s = e->stream;
  const u32 rows = 1024;
  const u32 T = (n + 63) >> 6;
  const u32 tpw = (T + rows - 1) / rows;

  u32 *d_perm = nullptr, *d_inv = nullptr, *d_hist = nullptr, *d_off = nullptr;
  u64 *d_nx = nullptr;
  u32 *d_nadj = nullptr;
  i32 *d_nwgt = nullptr, *d_nvw = nullptr;
  HIP_CHECK(hipMalloc(&d_perm, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_inv, sizeof(u32) * n));
  HIP_CHECK(hipMalloc(&d_hist, sizeof(u32) * kDbBuckets * rows));
  HIP_CHECK(hipMalloc(&d_off, sizeof(u32) * kDbBuckets * rows));
  HIP_CHECK(hipMalloc(&d_nx, sizeof(u64) * (n + 1)));
  HIP_CHECK(hipMalloc(&d_nadj, sizeof(u32) * m));
  if (e->has_adjwgt) {
    HIP_CHECK(hipMalloc(&d_nwgt, sizeof(i32) * m));
  }
  if (e->has_vwgt) {
    HIP_CHECK(hipMalloc(&d_nvw, sizeof(i32) * n));
  }

  hipLaunchKernelGGL(
      k_db_hist, dim3(rows / 4), dim3(threads), 0, s, n, rows, tpw, e->d_xadj, d_hist
  );
  LAUNCH_CHECK();
  // exclusive scan of the 33 x rows matrix (single WG; one-time setup cost)
  {
    // reuse k_scan_small's machinery via a plain rocprim scan
    void *tmp = nullptr;
    size_t tb = 0;
    HIP_CHECK(rocprim::exclusive_scan(
        nullptr, tb, d_hist, d_off, 0u, kDbBuckets * rows, rocprim::plus<u32>()
    ));
    HIP_CHECK(hipMalloc(&tmp, tb));
    HIP_CHECK(rocprim::exclusive_scan(
        tmp, tb, d_hist, d_off, 0u, kDbBuckets * rows, rocprim::plus<u32>(), s
    ));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipFree(tmp));
  }
  hipLaunchKernelGGL(
      k_db_scatter, dim3(rows / 4), dim3(threads), 0, s, n, rows, tpw, e->d_xadj, d_off,
      d_perm, d_inv
  );
  LAUNCH_CHECK();
  HIP_CHECK(hipMemsetAsync(d_nx, 0, sizeof(u64), s));
  hipLaunchKernelGGL(
      k_db_degrees, dim3(ceil_div(n, threads)), dim3(threads), 0, s, n, e->d_xadj, d_inv, d_nx
  );
  LAUNCH_CHECK();
  {
    void *tmp = nullptr;
    size_t tb = 0;
    HIP_CHECK(rocprim::inclusive_scan(nullptr, tb, d_nx, d_nx, n + 1, rocprim::plus<u64>()));
    HIP_CHECK(hipMalloc(&tmp, tb));
    HIP_CHECK(rocprim::inclusive_scan(tmp, tb, d_nx, d_nx, n + 1, rocprim::plus<u64>(), s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipFree(tmp));
  }
  hipLaunchKernelGGL(
      k_db_gather, dim3(16384), dim3(threads), 0, s, n, e->d_xadj, e->d_adjncy, e->d_adjwgt,
      e->d_vwgt, d_perm, d_inv, d_nx, d_nadj, d_nwgt, d_nvw
  );
  LAUNCH_CHECK();
  HIP_CHECK(hipMemcpyAsync(perm_out, d_perm, sizeof(u32) * n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));

  // adopt the rearranged CSR
  HIP_CHECK(hipFree(e->d_xadj));
  HIP_CHECK(hipFree(e->d_adjncy));
  e->d_xadj = d_nx;
  e->d_adjncy = d_nadj;
  if (e->has_adjwgt) {
    HIP_CHECK(hipFree(e->d_adjwgt));
    e->d_adjwgt = d_nwgt;
  }
  if (e->has_vwgt) {
    HIP_CHECK(hipFree(e->d_vwgt));
    e->d_vwgt = d_nvw;
  }
  // remap the isolated-vertex list (ids changed)
  for (u32 &u : e->isolated) {
    u = perm_out[u];
  }
  HIP_CHECK(hipFree(d_perm));
  HIP_CHECK(hipFree(d_inv));
  HIP_CHECK(hipFree(d_hist));
  HIP_CHECK(hipFree(d_off));
  return 0;
}

// ==================== C++ RCCL distributed driver ====================
// The per-chunk loop of the sharded multi-GPU refinement, driven from C++
// with RCCL called directly on the engine stream (the python/torch
// orchestration of kaminpar_amd.multi measured a ~0.65 ms/chunk host
// floor; this driver's floor is the per-round convergence readback only).
// Protocol identical to refine_dist_sharded / the 2-rank-sim-verified
// kernels (kaminpar-dist/refinement/lp/lp_refiner.cc:296-333).

#define NCCL_CHECK(cmd)                                                        \
  do {                                                                         \
    ncclResult_t r_ = (cmd);                                                   \
    if (r_ != ncclSuccess) {                                                   \
      fprintf(stderr, "kaminpar_amd: RCCL error %s at %s:%d\n",               \
              ncclGetErrorString(r_), __FILE__, __LINE__);                     \
      return -1;                                                               \
    }                                                                          \
  } while (0)

int kmp_nccl_unique_id(void *out128) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) {
    return -1;
  }
  memcpy(out128, &id, sizeof(id));
  return 0;
}

void *kmp_nccl_comm_init(int world, int rank, const void *id128) {
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t comm = nullptr;
  if (ncclCommInitRank(&comm, world, id, rank) != ncclSuccess) {
    return nullptr;
  }
  return comm;
}

void kmp_nccl_comm_destroy(void *comm) {
  if (comm) {
    (void)ncclCommDestroy(static_cast<ncclComm_t>(comm));
  }
}

i64 kmp_lp_refine_dist(
    kmp_lp_t *e,
    u32 k,
    const i64 *max_block_weights,
    u32 *partition,
    u64 seed,
    int iters,
    void *nccl_comm, // null at world 1
    int rank,
    int world,
    kmp_lp_stats_t *stats
) {
  if (kmp_lp_refine_begin(e, k, max_block_weights, partition, seed) != 0) {
    return -1;
  }
  if (e->coop_nblk < 8 || k > 256) {
    fprintf(stderr, "kaminpar_amd: refine_dist requires the v2 path (k <= 256)\n");
    return -1;
  }
  ncclComm_t comm = static_cast<ncclComm_t>(nccl_comm);
  const u32 threads = 256;
  const u32 cap = e->C / world + 2;      // per-rank proposal capacity
  const u32 seg = cap + 1;               // + trailing count row
  const u32 c_lo = (static_cast<u64>(rank) * k) / world;
  const u32 c_hi = (static_cast<u64>(rank) + 1) * k / world;

  Prop *d_send = nullptr, *d_recv = nullptr;
  long long *d_coll = nullptr; // dep[k+1] | delta[k+1] | meta[2k]
  HIP_CHECK(hipMalloc(&d_send, sizeof(Prop) * seg));
  HIP_CHECK(hipMalloc(&d_recv, sizeof(Prop) * seg * world));
  HIP_CHECK(hipMalloc(&d_coll, sizeof(long long) * (2 * (k + 1) + 2 * k)));
  long long *d_dep_g = d_coll;
  long long *d_delta = d_coll + (k + 1);
  long long *d_meta = d_coll + 2 * (k + 1); // [0..k) cutoffs, [k..2k) arr
  const u32 rows = 1024;
  const u32 cap_total = seg * world; // bound for tpw sizing
  const u32 tpw = (((cap_total + 63) >> 6) + rows - 1) / rows;
  const size_t lds_h = static_cast<size_t>(threads / kWave) * k * sizeof(u32);
  const size_t lds_sc = lds_h + static_cast<size_t>(2 * k) * sizeof(unsigned long long);

  unsigned long long moves_prev = 0;
  for (int iter = 0; iter < iters; ++iter) {
    const u64 iseed = iter_seed_of(e->seed, iter);
    e->ev_used = 0; // per-sweep phase-A event pairs (bench roofline input)
    for (u32 chunk = 0; chunk < kmp::kNumChunks; ++chunk) {
      const u32 lo = chunk * e->C;
      const u32 hi = lo + e->C > e->P ? e->P : lo + e->C;
      if (lo >= hi) {
        continue;
      }
      const u32 span = hi - lo;
      const u32 slo = lo + (static_cast<u64>(rank) * span) / world;
      const u32 shi = lo + ((static_cast<u64>(rank) + 1) * span) / world;

      // phase A on the rank's slice; compact (stable, position order =
      // rank order) into the send buffer; count rides the trailing row.
      // Slots MUST be pre-invalidated here: the memset-free phase A leaves
      // stale proposals in inactive units' slots, which the v2 commit
      // gates by unit_active but a flat compaction cannot.
      HIP_CHECK(hipMemsetAsync(e->d_slots, 0xFF, sizeof(Prop) * (shi - slo), e->stream));
      {
        hipEvent_t a0 = ev_one(e);
        HIP_CHECK(hipEventRecord(a0, e->stream));
      }
      phase_a_v2(e, iter, slo, shi, lo, true);
      {
        hipEvent_t a1 = ev_one(e);
        HIP_CHECK(hipEventRecord(a1, e->stream));
      }
      {
        size_t tb = e->select_temp_bytes;
        HIP_CHECK(rocprim::select(
            e->d_select_temp, tb, e->d_slots, d_send, e->d_prop_count, shi - slo, PropValid(),
            e->stream
        ));
      }
      hipLaunchKernelGGL(k_pack_count, dim3(1), dim3(1), 0, e->stream, e->d_prop_count,
                         d_send + cap);
      LAUNCH_CHECK();

      if (world > 1) {
        NCCL_CHECK(ncclAllGather(d_send, d_recv, static_cast<size_t>(seg) * 4, ncclUint32,
                                 comm, e->stream));
      } else {
        HIP_CHECK(hipMemcpyAsync(d_recv, d_send, sizeof(Prop) * seg, hipMemcpyDeviceToDevice,
                                 e->stream));
      }
      hipLaunchKernelGGL(
          k_compact_gathered, dim3(256), dim3(threads), 0, e->stream, world, cap, d_recv,
          e->d_props, e->d_prop_count
      );
      LAUNCH_CHECK();

      // sort own targets + full-admission dep/arr
      HIP_CHECK(hipMemsetAsync(e->d_dep, 0, sizeof(unsigned long long) * 2 * k, e->stream));
      HIP_CHECK(hipMemsetAsync(d_coll, 0, sizeof(long long) * (k + 1), e->stream));
      hipLaunchKernelGGL(
          k_hist_props, dim3(rows / 4), dim3(threads), lds_h, e->stream, e->d_prop_count, k,
          rows, tpw, c_lo, c_hi, e->d_props, e->d_histT
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_scan_small<true>, dim3(1), dim3(threads), 0, e->stream, k, rows, e->d_histT,
          e->d_offT, e->d_seg_off, e->d_prefix_len, e->d_dep, e->d_changed
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_scatter_props, dim3(rows / 4), dim3(threads), lds_sc, e->stream, e->d_prop_count,
          k, rows, tpw, c_lo, c_hi, e->d_props, e->d_offT, e->d_labels, e->d_s_u, e->d_s_w,
          e->d_s_r, e->d_s_to, e->d_s_b, d_dep_g,
          reinterpret_cast<unsigned long long *>(e->d_dep) + k
      );
      LAUNCH_CHECK();
      if (e->has_vwgt) {
        hipLaunchKernelGGL(
            k_shard_pw, dim3(64), dim3(threads), 0, e->stream, k, c_lo, c_hi, e->d_seg_off,
            e->d_prefix_len, e->d_s_w, e->d_pw
        );
        LAUNCH_CHECK();
      }
      if (world > 1) {
        NCCL_CHECK(ncclAllReduce(d_dep_g, d_dep_g, k + 1, ncclInt64, ncclSum, comm,
                                 e->stream));
      }

      // fixpoint rounds: local cutoffs + allreduced de-admission deltas
      for (;;) {
        hipLaunchKernelGGL(
            k_shard_round, dim3(1), dim3(256), 0, e->stream, k, c_lo, c_hi,
            static_cast<u32>(e->has_vwgt ? 1 : 0), e->d_seg_off, e->d_prefix_len,
            reinterpret_cast<unsigned long long *>(e->d_dep) + k, d_dep_g, e->d_s_w, e->d_s_b,
            e->d_pw, e->d_weights, e->d_maxw, d_delta
        );
        LAUNCH_CHECK();
        if (world > 1) {
          NCCL_CHECK(ncclAllReduce(d_delta, d_delta, k + 1, ncclInt64, ncclSum, comm,
                                   e->stream));
        }
        HIP_CHECK(hipMemcpyAsync(e->h_moves, d_delta + k, sizeof(long long),
                                 hipMemcpyDeviceToHost, e->stream));
        sync_spin(e);
        if (*reinterpret_cast<long long *>(e->h_moves) == 0) {
          break;
        }
        hipLaunchKernelGGL(
            k_vec_sub_i64, dim3(ceil_div(k, threads)), dim3(threads), 0, e->stream, k, d_dep_g,
            d_delta
        );
        LAUNCH_CHECK();
      }

      // exchange cutoffs + admitted arrivals (one summed 2k vector), apply
      HIP_CHECK(hipMemsetAsync(d_meta, 0, sizeof(long long) * 2 * k, e->stream));
      hipLaunchKernelGGL(
          k_shard_finish_meta, dim3(ceil_div(k, 256u)), dim3(256), 0, e->stream, k, c_lo, c_hi,
          e->d_seg_off, e->d_prefix_len,
          reinterpret_cast<unsigned long long *>(e->d_dep) + k, e->d_s_r,
          reinterpret_cast<unsigned long long *>(d_meta), d_meta + k
      );
      LAUNCH_CHECK();
      if (world > 1) {
        NCCL_CHECK(ncclAllReduce(d_meta, d_meta, 2 * k, ncclInt64, ncclSum, comm, e->stream));
      }
      {
        const u32 span2 = cap_total > k ? cap_total : k;
        hipLaunchKernelGGL(
            k_shard_apply, dim3(ceil_div(span2, threads)), dim3(threads), 0, e->stream,
            e->d_prop_count, k, e->d_props,
            reinterpret_cast<const unsigned long long *>(d_meta), d_meta + k, d_dep_g,
            e->d_weights, e->d_labels, e->d_labels16, k <= 256 ? e->d_labels8 : nullptr,
            e->d_admitted_flags, e->d_moves
        );
        LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(
          k_clear_active, dim3(ceil_div(span, threads)), dim3(threads), 0, e->stream, lo, hi,
          e->n, iseed, 0xFFFFFFFFu, e->d_xadj, e->d_active, e->d_unit_active, e->d_arcs
      );
      LAUNCH_CHECK();
      hipLaunchKernelGGL(
          k_activate_props_dev, dim3(2048), dim3(threads), 0, e->stream, e->d_prop_count,
          e->d_admitted_flags, e->d_props, e->d_xadj, e->d_adjncy, e->d_active,
          e->d_unit_active
      );
      LAUNCH_CHECK();
    }
    // early exit: moves counter is bit-identical on every rank
    HIP_CHECK(hipMemcpyAsync(&e->h_moves[1], e->d_moves, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, e->stream));
    sync_spin(e);
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
      e->phase_a_ms += ms;
    }
    if (e->h_moves[1] == moves_prev) {
      break;
    }
    moves_prev = e->h_moves[1];
  }
  // arcs are tallied per position slice: sum over ranks so stats report
  // the whole job (every other counter is already rank-identical)
  if (world > 1) {
    NCCL_CHECK(ncclAllReduce(
        reinterpret_cast<unsigned long long *>(e->d_arcs),
        reinterpret_cast<unsigned long long *>(e->d_arcs), 1, ncclUint64, ncclSum, comm,
        e->stream
    ));
    HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  HIP_CHECK(hipFree(d_send));
  HIP_CHECK(hipFree(d_recv));
  HIP_CHECK(hipFree(d_coll));
  return kmp_lp_refine_end(e, partition, stats);
}

u32 kmp_lp_n(const kmp_lp_t *e) { return e->n; }
u64 kmp_lp_m(const kmp_lp_t *e) { return e->m; }

} // extern "C"
