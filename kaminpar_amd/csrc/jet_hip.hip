// MI355X (gfx950) kernels of the Jet refiner (kmp_lp_jet). Semantics restated
// from kaminpar-shm/refinement/jet/jet_refiner.cc:94-234: a synchronous
// find pass (best adjacent block per unlocked vertex, negative gains admitted
// up to floor(temp * own-connectivity)), an afterburner that re-evaluates
// every candidate assuming its better-ranked neighbours already moved, and
// the execution of the surviving moves.
//
// Kernel design (CDNA4): like the LP refine kernels this is an irregular
// gather workload bounded by 8 B per directed arc in find (4 B adjncy + one
// label-shadow gather) and 12 B per candidate arc in the afterburner (4 B
// adjncy + one 8-byte record gather). Three degree tiers, built once per
// call: deg <= 16 in 16-lane subgroups (gains in registers, shuffles), one
// wavefront per vertex up to deg 2048 with a dense replicated per-wave LDS
// table, one workgroup per vertex beyond. The candidate record carries the
// snapshot label, so the afterburner never reads the label arrays and commits
// surviving moves in place (labels + both shadows + lock byte); block-weight
// deltas go through a per-workgroup LDS histogram and integer global atomics,
// which keeps the result independent of scheduling.

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "jet_hip.h"

namespace kmp_jet {

namespace {

constexpr u32 kWave = 64;
constexpr u32 kThreads = 256;
constexpr u32 kSmallDeg = 16;
constexpr u32 kMidDeg = 2048;
constexpr u32 kNone = 0xFFFFFFFFu;
// Every kernel is grid-stride: 2048 workgroups x 4 wavefronts fill the 256
// CUs (32 wavefronts each) and bound the end-of-kernel counter atomics.
constexpr u32 kMaxGrid = 2048;

#define JET_LAUNCH_CHECK()                                                                         \
  do {                                                                                             \
    hipError_t lerr_ = hipGetLastError();                                                          \
    if (lerr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: launch error %s at %s:%d\n", hipGetErrorString(lerr_),       \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

// Same replication rule as the LP refine M path: lane l adds into replica
// l % R so same-address LDS atomics serialize ~R times less for small k.
__host__ __device__ inline u32 replicas(u32 k) {
  if (k <= 64) {
    return 8;
  }
  if (k <= 256) {
    return 4;
  }
  return 1;
}

// (connectivity desc, block id asc): the reference scans blocks in ascending
// order with a strict >, so the lowest id wins ties.
__device__ inline bool better(i32 g, u32 c, i32 bg, u32 bc) {
  return g > bg || (g == bg && c < bc);
}

// Keep the move iff gain > -floor(temp * own): product in double, compared
// as integers (jet_refiner.cc:118-124).
__device__ inline bool keep_move(i32 gain, i32 own, double temp) {
  const i32 thr = -static_cast<i32>(floor(temp * static_cast<double>(own)));
  return gain > thr;
}

// Block-level sum of up to two counters, then ONE global atomic per counter
// and workgroup: same-address global atomics serialize (~10 ns each), and one
// per wavefront cost more than the S-tier kernels' own work at scale 20.
// Every thread of the block must call this (it synchronizes).
__device__ inline void add_block_totals(
    unsigned long long a, unsigned long long *dst_a, unsigned long long b = 0,
    unsigned long long *dst_b = nullptr
) {
  __shared__ unsigned long long red_a[kThreads / kWave];
  __shared__ unsigned long long red_b[kThreads / kWave];
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, kWave);
    b += __shfl_down(b, off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red_a[threadIdx.x >> 6] = a;
    red_b[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 wv = 1; wv < kThreads / kWave; ++wv) {
      a += red_a[wv];
      b += red_b[wv];
    }
    if (a) {
      atomicAdd(dst_a, a);
    }
    if (dst_b != nullptr && b) {
      atomicAdd(dst_b, b);
    }
  }
}

// ------------------------------------------------------------------ tiers
__global__ void k_jet_tiers(View v) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lane = threadIdx.x & (kWave - 1);
  u32 deg = 0;
  if (u < v.n) {
    deg = static_cast<u32>(v.xadj[u + 1] - v.xadj[u]);
  }
  const bool is_l = deg > kMidDeg;
  const bool is_m = deg > kSmallDeg && !is_l;
  // wave-aggregated append: one atomic per wave and list
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long mm = __ballot(is_m);
  if (mm) {
    const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(mm))) - 1u;
    u32 base = 0;
    if (lane == leader) {
      base = atomicAdd(&v.tier_counts[0], static_cast<u32>(__popcll(mm)));
    }
    base = __shfl(base, leader, kWave);
    if (is_m) {
      v.m_list[base + static_cast<u32>(__popcll(mm & below))] = u;
    }
  }
  const unsigned long long lm = __ballot(is_l);
  if (lm) {
    const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(lm))) - 1u;
    u32 base = 0;
    if (lane == leader) {
      base = atomicAdd(&v.tier_counts[1], static_cast<u32>(__popcll(lm)));
    }
    base = __shfl(base, leader, kWave);
    if (is_l) {
      v.l_list[base + static_cast<u32>(__popcll(lm & below))] = u;
    }
  }
}

// 16-lane row rotations as DPP moves (VALU rate, no LDS traffic): the S-tier
// dedupe needs 45 lane exchanges per vertex, and as ds_bpermute shuffles they
// kept the kernel bound by the LDS pipe. A subgroup is one DPP row, and all
// 16 lanes of a row are active together wherever these are used.
template <int I>
__device__ inline u32 row_ror(u32 x) {
  return static_cast<u32>(
      __builtin_amdgcn_mov_dpp(static_cast<int>(x), 0x120 + I, 0xf, 0xf, false)
  );
}

// Visit the 15 other lanes of the row: sum the weights of equal blocks; the
// lowest slot holding a block owns the sum. The source slot is rotated along,
// so the code does not depend on the rotation's direction.
template <int I>
struct RowDedupe {
  static __device__ inline void run(u32 c, i32 w, u32 slot, i32 &conn, bool &owner) {
    const u32 ci = row_ror<I>(c);
    const i32 wi = static_cast<i32>(row_ror<I>(static_cast<u32>(w)));
    const u32 si = row_ror<I>(slot);
    if (c != kNone && ci == c) {
      conn += wi;
      if (si < slot) {
        owner = false;
      }
    }
    RowDedupe<I + 1>::run(c, w, slot, conn, owner);
  }
};
template <>
struct RowDedupe<16> {
  static __device__ inline void run(u32, i32, u32, i32 &, bool &) {}
};

// One step of the row all-reduce (rotations by 8, 4, 2, 1): own is summed,
// (bg, bc) takes the better pair; the order is total, so all lanes agree.
template <int I>
__device__ inline void row_reduce_step(i32 &own, i32 &bg, u32 &bc) {
  own += static_cast<i32>(row_ror<I>(static_cast<u32>(own)));
  const i32 og = static_cast<i32>(row_ror<I>(static_cast<u32>(bg)));
  const u32 oc = row_ror<I>(bc);
  if (better(og, oc, bg, bc)) {
    bg = og;
    bc = oc;
  }
}

// ------------------------------------------------------------- find, S tier
// Grid-stride over groups of kFindUnroll vertex quads; owns the record of
// EVERY vertex with deg <= 16 (locked, isolated and interior vertices get a
// "no move" record). The row loop is software-pipelined: the xadj reads, then
// the adjncy reads, then the label gathers of all kFindUnroll vertices of a
// subgroup are issued back to back before the first one is consumed, so each
// lane keeps kFindUnroll gathers in flight (one vertex per subgroup and step
// was latency-bound: 0.92 ms per pass at R-MAT scale 23).
constexpr u32 kFindUnroll = 4;

template <typename LT>
__global__ void k_jet_find_s(View v, double temp, const LT *__restrict__ labels_s) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  constexpr u32 kStep = 4 * kFindUnroll;
  unsigned long long arcs = 0;
  for (u64 base = static_cast<u64>(wave_id) * kStep; base < v.n;
       base += static_cast<u64>(num_waves) * kStep) {
    u32 uu[kFindUnroll];
    u64 row[kFindUnroll];
    u32 deg[kFindUnroll];
    bool mine[kFindUnroll];
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      const u64 id = base + j * 4 + sub;
      mine[j] = id < v.n;
      uu[j] = mine[j] ? static_cast<u32>(id) : 0u;
      row[j] = 0;
      deg[j] = 0;
      if (mine[j]) {
        row[j] = v.xadj[uu[j]];
        deg[j] = static_cast<u32>(v.xadj[uu[j] + 1] - row[j]);
      }
      mine[j] = mine[j] && deg[j] <= kSmallDeg; // wide tiers own the rest
    }
    u32 cur[kFindUnroll];
    bool act[kFindUnroll];
    u32 nb[kFindUnroll];
    i32 w[kFindUnroll];
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      cur[j] = 0;
      act[j] = false;
      nb[j] = kNone;
      w[j] = 0;
      if (mine[j]) {
        cur[j] = v.labels[uu[j]];
        act[j] = deg[j] > 0 && !v.lock[uu[j]];
        if (act[j] && slot < deg[j]) {
          nb[j] = __builtin_nontemporal_load(&v.adjncy[row[j] + slot]);
          w[j] = v.adjwgt ? v.adjwgt[row[j] + slot] : 1;
        }
      }
    }
    u32 cc[kFindUnroll];
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      cc[j] = nb[j] != kNone ? static_cast<u32>(labels_s[nb[j]]) : kNone;
    }
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      if (!mine[j]) { // uniform over the subgroup
        continue;
      }
      Rec out{0, static_cast<uint16_t>(cur[j]), static_cast<uint16_t>(cur[j])};
      if (act[j]) {
        const u32 c = cc[j];
        // dedupe within the subgroup: the lowest slot of a block owns its sum
        i32 conn = w[j];
        bool owner = slot < deg[j];
        RowDedupe<1>::run(c, w[j], slot, conn, owner);
        i32 own = (owner && c == cur[j]) ? conn : 0;
        i32 bg = (owner && c != cur[j]) ? conn : 0;
        u32 bc = bg > 0 ? c : kNone;
        row_reduce_step<8>(own, bg, bc);
        row_reduce_step<4>(own, bg, bc);
        row_reduce_step<2>(own, bg, bc);
        row_reduce_step<1>(own, bg, bc);
        if (bg > 0 && keep_move(bg - own, own, temp)) {
          out.gain = bg - own;
          out.next = static_cast<uint16_t>(bc);
        }
        if (slot == 0) {
          arcs += deg[j];
        }
      }
      if (slot == 0) {
        v.rec[uu[j]] = out;
      }
    }
  }
  add_block_totals(arcs, v.arcs);
}

// ------------------------------------------------ find, wave / workgroup tier
// G threads per listed vertex (64: one wavefront, 256: one workgroup) with a
// dense table of k * R counters in LDS. The row loop keeps four adjncy loads
// and four label gathers in flight per lane before the LDS atomics.
template <u32 G>
__device__ inline void group_sync() {
  if constexpr (G == kWave) {
    __threadfence_block(); // table slice is private to this wavefront
  } else {
    __syncthreads();
  }
}

template <u32 G, bool kUnitWeights, typename LT>
__global__ void k_jet_find_w(
    View v, double temp, const LT *__restrict__ labels_s, const u32 *__restrict__ list, u32 count
) {
  extern __shared__ i32 jet_lds[];
  __shared__ i32 red_g[kThreads / kWave];
  __shared__ u32 red_c[kThreads / kWave];
  constexpr u32 kGroups = kThreads / G;
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 R = replicas(v.k);
  const u32 k = v.k;
  i32 *gains = jet_lds + (threadIdx.x / G) * k * R;
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  unsigned long long arcs = 0;

  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    const u32 cur = v.labels[u];
    if (v.lock[u]) { // uniform over the group
      if (t == 0) {
        v.rec[u] = Rec{0, static_cast<uint16_t>(cur), static_cast<uint16_t>(cur)};
      }
      continue;
    }
    for (u32 c = t; c < k * R; c += G) {
      gains[c] = 0;
    }
    group_sync<G>();

    const u32 rep_off = (lane % R) * k;
    for (u32 e0 = t; e0 < deg; e0 += 4 * G) {
      u32 nb[4];
      i32 w[4];
      u32 lab[4];
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        const u32 e = e0 + j * G;
        nb[j] = e < deg ? __builtin_nontemporal_load(&v.adjncy[row + e]) : kNone;
        w[j] = (kUnitWeights || e >= deg) ? 1 : v.adjwgt[row + e];
      }
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        lab[j] = nb[j] != kNone ? static_cast<u32>(labels_s[nb[j]]) : kNone;
      }
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        if (lab[j] != kNone) {
          atomicAdd(&gains[rep_off + lab[j]], w[j]);
        }
      }
    }
    group_sync<G>();

    i32 own = 0;
    for (u32 r = 0; r < R; ++r) {
      own += gains[r * k + cur];
    }
    i32 bg = 0;
    u32 bc = kNone;
    for (u32 c = t; c < k; c += G) {
      i32 g = 0;
      for (u32 r = 0; r < R; ++r) {
        g += gains[r * k + c];
      }
      if (c != cur && g > bg) { // ascending c per lane: strict > keeps the lowest id
        bg = g;
        bc = c;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const i32 og = __shfl_xor(bg, off, kWave);
      const u32 oc = __shfl_xor(bc, off, kWave);
      if (better(og, oc, bg, bc)) {
        bg = og;
        bc = oc;
      }
    }
    if constexpr (G > kWave) {
      if (lane == 0) {
        red_g[threadIdx.x >> 6] = bg;
        red_c[threadIdx.x >> 6] = bc;
      }
      __syncthreads();
      if (t == 0) {
        for (u32 wv = 1; wv < G / kWave; ++wv) {
          if (better(red_g[wv], red_c[wv], bg, bc)) {
            bg = red_g[wv];
            bc = red_c[wv];
          }
        }
      }
    }
    if (t == 0) {
      Rec out{0, static_cast<uint16_t>(cur), static_cast<uint16_t>(cur)};
      if (bg > 0 && keep_move(bg - own, own, temp)) {
        out.gain = bg - own;
        out.next = static_cast<uint16_t>(bc);
      }
      v.rec[u] = out;
      arcs += deg;
    }
    group_sync<G>(); // table (and red_*) reuse across grid-stride iterations
  }
  add_block_totals(arcs, v.arcs);
}

// ------------------------------------------------- afterburner + execution
// A neighbour nb of candidate u is assumed to have moved already iff it is a
// candidate itself and ranks ahead of u: higher gain, ties by lower id
// (jet_refiner.cc:150-176). Contribution +w if its assumed block is u's
// target, -w if it is u's current block.
__device__ inline i32 arc_contribution(const Rec r, u32 u, u32 nb, const Rec rv, i32 w) {
  const bool ahead =
      rv.next != rv.label && (rv.gain > r.gain || (rv.gain == r.gain && nb < u));
  const uint16_t ab = ahead ? rv.next : rv.label;
  return (ab == r.next ? w : 0) - (ab == r.label ? w : 0);
}

// In-place commit of one surviving move (one thread per vertex).
__device__ inline void commit_move(
    const View &v, u32 u, const Rec r, unsigned long long *hist, unsigned long long &moves
) {
  v.labels[u] = r.next;
  v.labels16[u] = r.next;
  v.labels8[u] = static_cast<uint8_t>(r.next);
  const long long uw = v.vwgt ? v.vwgt[u] : 1;
  atomicAdd(&hist[r.label], static_cast<unsigned long long>(-uw));
  atomicAdd(&hist[r.next], static_cast<unsigned long long>(uw));
  moves += 1;
}

__device__ inline void hist_clear(unsigned long long *hist, u32 k) {
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    hist[c] = 0;
  }
  __syncthreads();
}

__device__ inline void hist_flush(const View &v, unsigned long long *hist) {
  __syncthreads();
  for (u32 c = threadIdx.x; c < v.k; c += blockDim.x) {
    if (hist[c]) {
      atomicAdd(reinterpret_cast<unsigned long long *>(&v.weights[c]), hist[c]);
    }
  }
}

__global__ void k_jet_filter_s(View v) {
  extern __shared__ unsigned long long jet_hist[];
  hist_clear(jet_hist, v.k);
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  unsigned long long arcs = 0, moves = 0;
  for (u64 base = static_cast<u64>(wave_id) * 4; base < v.n; base += static_cast<u64>(num_waves) * 4) {
    const u64 u64id = base + sub;
    if (u64id >= v.n) {
      continue;
    }
    const u32 u = static_cast<u32>(u64id);
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    if (deg > kSmallDeg) {
      continue;
    }
    const Rec r = v.rec[u];
    if (r.next == r.label) { // not a candidate: every other lock is cleared
      if (slot == 0) {
        v.lock[u] = 0;
      }
      continue;
    }
    i32 sum = 0;
    if (slot < deg) {
      const u32 nb = __builtin_nontemporal_load(&v.adjncy[row + slot]);
      const Rec rv = v.rec[nb];
      const i32 w = v.adjwgt ? v.adjwgt[row + slot] : 1;
      sum = arc_contribution(r, u, nb, rv, w);
    }
    for (int off = 8; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off, kWave);
    }
    if (slot == 0) {
      const bool locked = sum > 0;
      v.lock[u] = locked ? 1 : 0;
      if (locked) {
        commit_move(v, u, r, jet_hist, moves);
      }
      arcs += deg;
    }
  }
  hist_flush(v, jet_hist);
  add_block_totals(arcs, v.arcs, moves, v.moves);
}

template <u32 G>
__global__ void k_jet_filter_w(View v, const u32 *__restrict__ list, u32 count) {
  extern __shared__ unsigned long long jet_hist[];
  __shared__ i32 red_s[kThreads / kWave];
  hist_clear(jet_hist, v.k);
  constexpr u32 kGroups = kThreads / G;
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  unsigned long long arcs = 0, moves = 0;
  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const Rec r = v.rec[u];
    if (r.next == r.label) { // uniform over the group
      if (t == 0) {
        v.lock[u] = 0;
      }
      continue;
    }
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    i32 sum = 0;
#pragma unroll 4
    for (u32 e = t; e < deg; e += G) {
      const u32 nb = __builtin_nontemporal_load(&v.adjncy[row + e]);
      const Rec rv = v.rec[nb];
      const i32 w = v.adjwgt ? v.adjwgt[row + e] : 1;
      sum += arc_contribution(r, u, nb, rv, w);
    }
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off, kWave);
    }
    if constexpr (G > kWave) {
      if (lane == 0) {
        red_s[threadIdx.x >> 6] = sum;
      }
      __syncthreads();
      if (t == 0) {
        for (u32 wv = 1; wv < G / kWave; ++wv) {
          sum += red_s[wv];
        }
      }
      __syncthreads(); // red_s reuse
    }
    if (t == 0) {
      const bool locked = sum > 0;
      v.lock[u] = locked ? 1 : 0;
      if (locked) {
        commit_move(v, u, r, jet_hist, moves);
      }
      arcs += deg;
    }
  }
  hist_flush(v, jet_hist);
  add_block_totals(arcs, v.arcs, moves, v.moves);
}

// ------------------------------------------------------------------ score
// Edge cut over the same three tiers (twice the cut: every edge is seen from
// both ends). The engine's k_edge_cut walks every row with 16 lanes, which
// serializes on R-MAT hubs (measured 21.7 ms per pass at scale 23, seven
// times find + filter together); here wide rows get a wavefront or a
// workgroup. Integer sums: the result is identical.
template <typename LT>
__global__ void k_jet_cut_s(View v, const LT *__restrict__ labels_s, unsigned long long *cut2) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  unsigned long long local = 0;
  for (u64 base = static_cast<u64>(wave_id) * 4; base < v.n; base += static_cast<u64>(num_waves) * 4) {
    const u64 u = base + sub;
    if (u >= v.n) {
      continue;
    }
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    if (slot < deg && deg <= kSmallDeg) {
      const u32 nb = __builtin_nontemporal_load(&v.adjncy[row + slot]);
      if (labels_s[nb] != labels_s[u]) {
        local += v.adjwgt ? v.adjwgt[row + slot] : 1;
      }
    }
  }
  add_block_totals(local, cut2);
}

template <u32 G, typename LT>
__global__ void k_jet_cut_w(
    View v, const LT *__restrict__ labels_s, const u32 *__restrict__ list, u32 count,
    unsigned long long *cut2
) {
  constexpr u32 kGroups = kThreads / G;
  const u32 t = threadIdx.x % G;
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  unsigned long long local = 0;
  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    const LT lu = labels_s[u];
#pragma unroll 4
    for (u32 e = t; e < deg; e += G) {
      const u32 nb = __builtin_nontemporal_load(&v.adjncy[row + e]);
      if (labels_s[nb] != lu) {
        local += v.adjwgt ? v.adjwgt[row + e] : 1;
      }
    }
  }
  add_block_totals(local, cut2);
}

u32 ceil_div_u32(u64 a, u64 b) { return static_cast<u32>((a + b - 1) / b); }

u32 clamp_grid(u64 want, u32 cap) {
  if (want < 1) {
    return 1;
  }
  return want > cap ? cap : static_cast<u32>(want);
}

template <u32 G, typename LT>
void launch_find_w(
    const View &v, double temp, const LT *shadow, const u32 *list, u32 count, u32 grid,
    hipStream_t stream
) {
  const size_t lds = static_cast<size_t>(kThreads / G) * v.k * replicas(v.k) * sizeof(i32);
  auto *kern = v.adjwgt ? k_jet_find_w<G, false, LT> : k_jet_find_w<G, true, LT>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, v, temp, shadow, list, count);
  JET_LAUNCH_CHECK();
}

template <typename LT>
void find_typed(
    const View &v, double temp, const LT *shadow, u32 m_count, u32 l_count, hipStream_t stream
) {
  const u32 grid_s = clamp_grid(
      ceil_div_u32(ceil_div_u32(v.n, 4 * kFindUnroll), kThreads / kWave), kMaxGrid
  );
  hipLaunchKernelGGL(k_jet_find_s<LT>, dim3(grid_s), dim3(kThreads), 0, stream, v, temp, shadow);
  JET_LAUNCH_CHECK();
  if (m_count > 0) {
    launch_find_w<kWave, LT>(
        v, temp, shadow, v.m_list, m_count, clamp_grid(ceil_div_u32(m_count, 4), kMaxGrid), stream
    );
  }
  if (l_count > 0) {
    launch_find_w<kThreads, LT>(
        v, temp, shadow, v.l_list, l_count, clamp_grid(l_count, kMaxGrid), stream
    );
  }
}

} // namespace

void build_tiers(const View &v, hipStream_t stream) {
  if (hipMemsetAsync(v.tier_counts, 0, sizeof(u32) * 2, stream) != hipSuccess) {
    fprintf(stderr, "kaminpar_amd: jet tier reset failed\n");
    abort();
  }
  hipLaunchKernelGGL(
      k_jet_tiers, dim3(clamp_grid(ceil_div_u32(v.n, kThreads), 0xFFFFFFFFu)), dim3(kThreads), 0,
      stream, v
  );
  JET_LAUNCH_CHECK();
}

void find(const View &v, double temp, u32 m_count, u32 l_count, hipStream_t stream) {
  if (v.k <= 256) {
    find_typed<uint8_t>(v, temp, v.labels8, m_count, l_count, stream);
  } else {
    find_typed<uint16_t>(v, temp, v.labels16, m_count, l_count, stream);
  }
}

namespace {

template <typename LT>
void cut_typed(
    const View &v, const LT *shadow, u32 m_count, u32 l_count, unsigned long long *cut2,
    hipStream_t stream
) {
  const u32 grid_s = clamp_grid(ceil_div_u32(ceil_div_u32(v.n, 4), kThreads / kWave), kMaxGrid);
  hipLaunchKernelGGL(k_jet_cut_s<LT>, dim3(grid_s), dim3(kThreads), 0, stream, v, shadow, cut2);
  JET_LAUNCH_CHECK();
  if (m_count > 0) {
    hipLaunchKernelGGL(
        (k_jet_cut_w<kWave, LT>), dim3(clamp_grid(ceil_div_u32(m_count, 4), kMaxGrid)),
        dim3(kThreads), 0, stream, v, shadow, v.m_list, m_count, cut2
    );
    JET_LAUNCH_CHECK();
  }
  if (l_count > 0) {
    hipLaunchKernelGGL(
        (k_jet_cut_w<kThreads, LT>), dim3(clamp_grid(l_count, kMaxGrid)), dim3(kThreads), 0, stream,
        v, shadow, v.l_list, l_count, cut2
    );
    JET_LAUNCH_CHECK();
  }
}

} // namespace

void edge_cut2(
    const View &v, u32 m_count, u32 l_count, unsigned long long *cut2, hipStream_t stream
) {
  if (hipMemsetAsync(cut2, 0, sizeof(unsigned long long), stream) != hipSuccess) {
    fprintf(stderr, "kaminpar_amd: jet cut reset failed\n");
    abort();
  }
  if (v.k <= 256) {
    cut_typed<uint8_t>(v, v.labels8, m_count, l_count, cut2, stream);
  } else {
    cut_typed<uint16_t>(v, v.labels16, m_count, l_count, cut2, stream);
  }
}

void filter_commit(const View &v, u32 m_count, u32 l_count, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(v.k) * sizeof(unsigned long long);
  const u32 grid_s = clamp_grid(ceil_div_u32(ceil_div_u32(v.n, 4), kThreads / kWave), kMaxGrid);
  hipLaunchKernelGGL(k_jet_filter_s, dim3(grid_s), dim3(kThreads), lds, stream, v);
  JET_LAUNCH_CHECK();
  if (m_count > 0) {
    hipLaunchKernelGGL(
        k_jet_filter_w<kWave>, dim3(clamp_grid(ceil_div_u32(m_count, 4), kMaxGrid)), dim3(kThreads),
        lds, stream, v, v.m_list, m_count
    );
    JET_LAUNCH_CHECK();
  }
  if (l_count > 0) {
    hipLaunchKernelGGL(
        k_jet_filter_w<kThreads>, dim3(clamp_grid(l_count, kMaxGrid)), dim3(kThreads), lds, stream, v,
        v.l_list, l_count
    );
    JET_LAUNCH_CHECK();
  }
}

// ================================================== selection rebalancer
// kmp_lp_rebalance (rule: include/kaminpar_lp.h; the reference's
// OverloadBalancer, overload_balancer.cc:162-271, takes the best relative
// gains of a block from a priority queue until its overload is gone). Here a
// pass is score -> order -> prefix-select -> order -> prefix-admit -> apply
// over a snapshot. The score kernels are find's three tiers restricted to
// the rows of over-cap blocks: a row outside them costs one shadow-label read
// and one LDS read. Candidates are flagged per vertex and compacted by a
// stable select, so the compacted list is in id order and one stable radix
// sort by the packed key yields (block, key desc, id asc).

namespace {

constexpr u64 kKeyMask = (1ull << 53) - 1ull;

#define JET_HIP_CHECK(expr)                                                                        \
  do {                                                                                             \
    hipError_t herr_ = (expr);                                                                     \
    if (herr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: HIP error %s at %s:%d\n", hipGetErrorString(herr_),          \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

// Stages cum (i64) and room into LDS. Room is only ever compared with a
// vertex weight (i32 >= 1), so it is kept saturated to i32.
__device__ inline void rb_stage(u32 k, const Rebal &rb, i64 *cum, i32 *room) {
  for (u32 c = threadIdx.x; c < k; c += blockDim.x) {
    cum[c] = rb.cum[c];
    i64 r = rb.room[c];
    r = r > 0x7FFFFFFFll ? 0x7FFFFFFFll : r;
    r = r < -0x7FFFFFFFll ? -0x7FFFFFFFll : r;
    room[c] = static_cast<i32>(r);
  }
  __syncthreads();
}

// One thread per scored vertex: fallback target, key, record. bg > 0 iff an
// eligible adjacent block (bc) exists.
__device__ inline void rb_emit(
    const View &v, const Rebal &rb, const i64 *cum, const i32 *room, u32 u, u32 cur, i32 vw,
    i32 own, i32 bg, u32 bc
) {
  u32 to = bc;
  i64 gain = static_cast<i64>(bg) - own;
  if (bg <= 0) {
    to = kNone;
    gain = -static_cast<i64>(own);
    if (rb.total_room > 0) {
      const u64 r = kmp::splitmix64((static_cast<u64>(rb.pass) << 32) | u) %
                    static_cast<u64>(rb.total_room);
      u32 lo = 0, hi = v.k - 1; // cum[k - 1] = total_room > r
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (static_cast<u64>(cum[mid]) > r) {
          hi = mid;
        } else {
          lo = mid + 1;
        }
      }
      if (room[lo] >= vw) {
        to = lo;
      }
    }
    if (to == kNone && room[rb.best_target] >= vw) {
      to = rb.best_target;
    }
    if (to == kNone) {
      return;
    }
  }
  i64 key;
  if (gain > 0) {
    const i64 gw = gain * vw;
    key = (gw > 0x7FFFFFFFll ? 0x7FFFFFFFll : gw) << 20;
  } else {
    key = -(((-gain) << 20) / vw);
  }
  rb.key[u] = (static_cast<u64>(cur) << 53) |
              static_cast<u64>(static_cast<i64>(kKeyMask) - (key + (1ll << 52)));
  rb.to[u] = static_cast<uint16_t>(to);
  rb.flag[u] = 1;
}

template <typename LT>
__global__ void k_rb_score_s(View v, Rebal rb, const LT *__restrict__ labels_s) {
  extern __shared__ i64 rb_lds[];
  i64 *cum = rb_lds;
  i32 *room = reinterpret_cast<i32 *>(rb_lds + v.k);
  rb_stage(v.k, rb, cum, room);
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  constexpr u32 kStep = 4 * kFindUnroll;
  unsigned long long arcs = 0;
  for (u64 base = static_cast<u64>(wave_id) * kStep; base < v.n;
       base += static_cast<u64>(num_waves) * kStep) {
    u32 uu[kFindUnroll];
    u64 row[kFindUnroll];
    u32 deg[kFindUnroll];
    u32 cur[kFindUnroll];
    i32 vw[kFindUnroll];
    bool mine[kFindUnroll];
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      const u64 id = base + j * 4 + sub;
      mine[j] = id < v.n;
      uu[j] = mine[j] ? static_cast<u32>(id) : 0u;
      cur[j] = mine[j] ? static_cast<u32>(labels_s[uu[j]]) : 0u;
      // rows outside the source blocks end here, adjacency untouched
      mine[j] = mine[j] && room[cur[j]] < 0;
      vw[j] = 1;
      row[j] = 0;
      deg[j] = 0;
      if (mine[j]) {
        vw[j] = v.vwgt ? v.vwgt[uu[j]] : 1;
        row[j] = v.xadj[uu[j]];
        deg[j] = static_cast<u32>(v.xadj[uu[j] + 1] - row[j]);
      }
      mine[j] = mine[j] && vw[j] > 0 && deg[j] <= kSmallDeg; // wide tiers own the rest
    }
    u32 nb[kFindUnroll];
    i32 w[kFindUnroll];
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      nb[j] = kNone;
      w[j] = 0;
      if (mine[j] && slot < deg[j]) {
        nb[j] = __builtin_nontemporal_load(&v.adjncy[row[j] + slot]);
        w[j] = v.adjwgt ? v.adjwgt[row[j] + slot] : 1;
      }
    }
    u32 cc[kFindUnroll];
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      cc[j] = nb[j] != kNone ? static_cast<u32>(labels_s[nb[j]]) : kNone;
    }
#pragma unroll
    for (u32 j = 0; j < kFindUnroll; ++j) {
      if (!mine[j]) { // uniform over the subgroup
        continue;
      }
      const u32 c = cc[j];
      i32 conn = w[j];
      bool owner = slot < deg[j];
      RowDedupe<1>::run(c, w[j], slot, conn, owner);
      i32 own = (owner && c == cur[j]) ? conn : 0;
      i32 bg = (owner && c != cur[j] && room[c] >= vw[j]) ? conn : 0;
      u32 bc = bg > 0 ? c : kNone;
      row_reduce_step<8>(own, bg, bc);
      row_reduce_step<4>(own, bg, bc);
      row_reduce_step<2>(own, bg, bc);
      row_reduce_step<1>(own, bg, bc);
      if (slot == 0) {
        arcs += deg[j];
        rb_emit(v, rb, cum, room, uu[j], cur[j], vw[j], own, bg, bc);
      }
    }
  }
  add_block_totals(arcs, rb.arcs);
}

template <u32 G, bool kUnitWeights, typename LT>
__global__ void k_rb_score_w(
    View v, Rebal rb, const LT *__restrict__ labels_s, const u32 *__restrict__ list, u32 count
) {
  extern __shared__ i64 rb_lds[];
  __shared__ i32 red_g[kThreads / kWave];
  __shared__ u32 red_c[kThreads / kWave];
  const u32 k = v.k;
  i64 *cum = rb_lds;
  i32 *room = reinterpret_cast<i32 *>(rb_lds + k);
  rb_stage(k, rb, cum, room);
  constexpr u32 kGroups = kThreads / G;
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 R = replicas(k);
  i32 *gains = room + k + (threadIdx.x / G) * k * R;
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  unsigned long long arcs = 0;

  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u32 cur = static_cast<u32>(labels_s[u]);
    if (room[cur] >= 0) { // uniform over the group: not in a source block
      continue;
    }
    const i32 vw = v.vwgt ? v.vwgt[u] : 1;
    if (vw <= 0) {
      continue;
    }
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    for (u32 c = t; c < k * R; c += G) {
      gains[c] = 0;
    }
    group_sync<G>();

    const u32 rep_off = (lane % R) * k;
    for (u32 e0 = t; e0 < deg; e0 += 4 * G) {
      u32 nb[4];
      i32 w[4];
      u32 lab[4];
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        const u32 e = e0 + j * G;
        nb[j] = e < deg ? __builtin_nontemporal_load(&v.adjncy[row + e]) : kNone;
        w[j] = (kUnitWeights || e >= deg) ? 1 : v.adjwgt[row + e];
      }
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        lab[j] = nb[j] != kNone ? static_cast<u32>(labels_s[nb[j]]) : kNone;
      }
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        if (lab[j] != kNone) {
          atomicAdd(&gains[rep_off + lab[j]], w[j]);
        }
      }
    }
    group_sync<G>();

    i32 own = 0;
    for (u32 r = 0; r < R; ++r) {
      own += gains[r * k + cur];
    }
    i32 bg = 0;
    u32 bc = kNone;
    for (u32 c = t; c < k; c += G) {
      i32 g = 0;
      for (u32 r = 0; r < R; ++r) {
        g += gains[r * k + c];
      }
      if (c != cur && g > bg && room[c] >= vw) { // ascending c: strict > keeps the lowest id
        bg = g;
        bc = c;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const i32 og = __shfl_xor(bg, off, kWave);
      const u32 oc = __shfl_xor(bc, off, kWave);
      if (better(og, oc, bg, bc)) {
        bg = og;
        bc = oc;
      }
    }
    if constexpr (G > kWave) {
      if (lane == 0) {
        red_g[threadIdx.x >> 6] = bg;
        red_c[threadIdx.x >> 6] = bc;
      }
      __syncthreads();
      if (t == 0) {
        for (u32 wv = 1; wv < G / kWave; ++wv) {
          if (better(red_g[wv], red_c[wv], bg, bc)) {
            bg = red_g[wv];
            bc = red_c[wv];
          }
        }
      }
    }
    if (t == 0) {
      arcs += deg;
      rb_emit(v, rb, cum, room, u, cur, vw, own, bg, bc);
    }
    group_sync<G>(); // table (and red_*) reuse across grid-stride iterations
  }
  add_block_totals(arcs, rb.arcs);
}

// keys[0][i] of the compacted ids: the per-vertex key as scored, or with the
// target in place of the source block.
__global__ void k_rb_keys(Rebal rb, u32 count, bool by_target) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    const u32 u = rb.ids[0][i];
    const u64 key = rb.key[u];
    rb.keys[0][i] = by_target ? ((static_cast<u64>(rb.to[u]) << 53) | (key & kKeyMask)) : key;
  }
}

__global__ void k_rb_segments(View v, Rebal rb, u32 count) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    rb.seg[i] = static_cast<u32>(rb.keys[1][i] >> 53);
    rb.wt[i] = v.vwgt ? v.vwgt[rb.ids[1][i]] : 1;
  }
}

__global__ void k_rb_select(Rebal rb, u32 count) {
  unsigned long long selected = 0;
  for (u64 i = blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += static_cast<u64>(gridDim.x) * blockDim.x) {
    if (rb.pre[i] < rb.over[rb.seg[i]]) {
      rb.flag[rb.ids[1][i]] = 1;
      selected += 1;
    }
  }
  add_block_totals(selected, rb.selected);
}

__global__ void k_rb_apply(View v, Rebal rb, u32 count) {
  extern __shared__ unsigned long long jet_hist[];
  hist_clear(jet_hist, v.k);
  unsigned long long moves = 0;
  for (u64 i = blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += static_cast<u64>(gridDim.x) * blockDim.x) {
    const u32 to = rb.seg[i];
    if (rb.pre[i] <= rb.room[to]) {
      const u32 u = rb.ids[1][i];
      const u32 from = v.labels[u];
      v.labels[u] = to;
      v.labels16[u] = static_cast<uint16_t>(to);
      v.labels8[u] = static_cast<uint8_t>(to);
      const unsigned long long uw = static_cast<unsigned long long>(rb.wt[i]);
      atomicAdd(&jet_hist[from], static_cast<unsigned long long>(0) - uw);
      atomicAdd(&jet_hist[to], uw);
      moves += 1;
    }
  }
  hist_flush(v, jet_hist);
  add_block_totals(moves, rb.moves);
}

template <u32 G, typename LT>
void launch_score_w(
    const View &v, const Rebal &rb, const LT *shadow, const u32 *list, u32 count, u32 grid,
    hipStream_t stream
) {
  const size_t lds = static_cast<size_t>(v.k) * (sizeof(i64) + sizeof(i32)) +
                     static_cast<size_t>(kThreads / G) * v.k * replicas(v.k) * sizeof(i32);
  auto *kern = v.adjwgt ? k_rb_score_w<G, false, LT> : k_rb_score_w<G, true, LT>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, v, rb, shadow, list, count);
  JET_LAUNCH_CHECK();
}

template <typename LT>
void score_typed(
    const View &v, const Rebal &rb, const LT *shadow, u32 m_count, u32 l_count, hipStream_t stream
) {
  const u32 grid_s = clamp_grid(
      ceil_div_u32(ceil_div_u32(v.n, 4 * kFindUnroll), kThreads / kWave), kMaxGrid
  );
  const size_t lds = static_cast<size_t>(v.k) * (sizeof(i64) + sizeof(i32));
  hipLaunchKernelGGL(k_rb_score_s<LT>, dim3(grid_s), dim3(kThreads), lds, stream, v, rb, shadow);
  JET_LAUNCH_CHECK();
  if (m_count > 0) {
    launch_score_w<kWave, LT>(
        v, rb, shadow, v.m_list, m_count, clamp_grid(ceil_div_u32(m_count, 4), kMaxGrid), stream
    );
  }
  if (l_count > 0) {
    launch_score_w<kThreads, LT>(
        v, rb, shadow, v.l_list, l_count, clamp_grid(l_count, kMaxGrid), stream
    );
  }
}

// Flagged vertices, compacted in id order (rocprim::select is stable).
void compact_flagged(const View &v, const Rebal &rb, hipStream_t stream) {
  size_t tb = rb.temp_bytes;
  JET_HIP_CHECK(rocprim::select(
      rb.temp, tb, rocprim::counting_iterator<u32>(0), rb.flag, rb.ids[0], rb.count, v.n, stream
  ));
}

u32 sort_end_bit(u32 k) {
  u32 bits = 1;
  while ((1u << bits) < k) {
    ++bits;
  }
  return 53 + bits;
}

} // namespace

size_t rebalance_temp_bytes(u32 n) {
  const size_t nn = n > 0 ? n : 1;
  size_t best = 0, tb = 0;
  JET_HIP_CHECK(rocprim::select(
      nullptr, tb, rocprim::counting_iterator<u32>(0), static_cast<uint8_t *>(nullptr),
      static_cast<u32 *>(nullptr), static_cast<u32 *>(nullptr), nn
  ));
  best = tb > best ? tb : best;
  JET_HIP_CHECK(rocprim::radix_sort_pairs(
      nullptr, tb, static_cast<u64 *>(nullptr), static_cast<u64 *>(nullptr),
      static_cast<u32 *>(nullptr), static_cast<u32 *>(nullptr), nn, 0, 64
  ));
  best = tb > best ? tb : best;
  JET_HIP_CHECK(rocprim::exclusive_scan_by_key(
      nullptr, tb, static_cast<u32 *>(nullptr), static_cast<i64 *>(nullptr),
      static_cast<i64 *>(nullptr), static_cast<i64>(0), nn, rocprim::plus<i64>(),
      rocprim::equal_to<u32>()
  ));
  best = tb > best ? tb : best;
  JET_HIP_CHECK(rocprim::inclusive_scan_by_key(
      nullptr, tb, static_cast<u32 *>(nullptr), static_cast<i64 *>(nullptr),
      static_cast<i64 *>(nullptr), nn, rocprim::plus<i64>(), rocprim::equal_to<u32>()
  ));
  best = tb > best ? tb : best;
  return best > 0 ? best : 1;
}

void rebalance_score(
    const View &v, const Rebal &rb, u32 m_count, u32 l_count, hipStream_t stream
) {
  JET_HIP_CHECK(hipMemsetAsync(rb.flag, 0, v.n > 0 ? v.n : 1, stream));
  if (v.k <= 256) {
    score_typed<uint8_t>(v, rb, v.labels8, m_count, l_count, stream);
  } else {
    score_typed<uint16_t>(v, rb, v.labels16, m_count, l_count, stream);
  }
  compact_flagged(v, rb, stream);
}

void rebalance_order(
    const View &v, const Rebal &rb, u32 count, bool by_target, hipStream_t stream
) {
  const u32 grid = ceil_div_u32(count, kThreads);
  hipLaunchKernelGGL(k_rb_keys, dim3(grid), dim3(kThreads), 0, stream, rb, count, by_target);
  JET_LAUNCH_CHECK();
  size_t tb = rb.temp_bytes;
  JET_HIP_CHECK(rocprim::radix_sort_pairs(
      rb.temp, tb, rb.keys[0], rb.keys[1], rb.ids[0], rb.ids[1], count, 0, sort_end_bit(v.k),
      stream
  ));
  hipLaunchKernelGGL(k_rb_segments, dim3(grid), dim3(kThreads), 0, stream, v, rb, count);
  JET_LAUNCH_CHECK();
  tb = rb.temp_bytes;
  if (by_target) {
    JET_HIP_CHECK(rocprim::inclusive_scan_by_key(
        rb.temp, tb, rb.seg, rb.wt, rb.pre, count, rocprim::plus<i64>(), rocprim::equal_to<u32>(),
        stream
    ));
  } else {
    JET_HIP_CHECK(rocprim::exclusive_scan_by_key(
        rb.temp, tb, rb.seg, rb.wt, rb.pre, static_cast<i64>(0), count, rocprim::plus<i64>(),
        rocprim::equal_to<u32>(), stream
    ));
  }
}

void rebalance_select(const View &v, const Rebal &rb, u32 count, hipStream_t stream) {
  JET_HIP_CHECK(hipMemsetAsync(rb.flag, 0, v.n > 0 ? v.n : 1, stream));
  hipLaunchKernelGGL(
      k_rb_select, dim3(clamp_grid(ceil_div_u32(count, kThreads), kMaxGrid)), dim3(kThreads), 0,
      stream, rb, count
  );
  JET_LAUNCH_CHECK();
  compact_flagged(v, rb, stream);
}

void rebalance_apply(const View &v, const Rebal &rb, u32 count, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(v.k) * sizeof(unsigned long long);
  hipLaunchKernelGGL(
      k_rb_apply, dim3(clamp_grid(ceil_div_u32(count, kThreads), kMaxGrid)), dim3(kThreads), lds,
      stream, v, rb, count
  );
  JET_LAUNCH_CHECK();
}

} // namespace kmp_jet
