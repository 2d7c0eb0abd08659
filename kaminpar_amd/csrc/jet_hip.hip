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

#include <hip/hip_runtime.h>

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

} // namespace kmp_jet
