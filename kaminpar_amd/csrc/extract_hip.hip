// MI355X (gfx950) kernels of the block subgraph extraction
// (kmp_lp_extract_subgraphs; rule in include/kaminpar_lp.h). Counterpart of
// graph::extract_subgraphs (kaminpar-shm/graphutils/subgraph_extractor.cc:
// 335-480): all block-induced subgraphs packed into one memory with per-block
// start positions. The reference hands out in-block ranks with a racing
// fetch_add; here the rank is the one a serial run produces (ascending id),
// from a stable sort, so the result is deterministic.
//
// Kernel design (CDNA4): two arc passes, each bound like Jet's find by 8 B per
// directed arc (4 B adjncy + one label-shadow gather); fill adds a mapping
// gather and the stores for internal arcs only. Rows are tiered as in
// jet_hip.hip: deg <= 16 in 16-lane subgroups, one wavefront per vertex up to
// deg 2048, one workgroup per vertex beyond. Every lane keeps four adjncy
// loads and four label gathers in flight before consuming them. Rows are
// compacted in adjacency order with ballots and prefix popcounts (__ballot is
// 64 bits wide), a running offset over 64-arc batches per wavefront and a
// workgroup scan per 256-arc batch: no atomic decides a position. Per-block
// counts go through per-workgroup LDS histograms and one integer global
// atomic per bin and workgroup, so scheduling never shows in the output.

#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include "extract_hip.h"

namespace kmp_extract {

namespace {

constexpr u32 kWave = 64;
constexpr u32 kThreads = 256;
constexpr u32 kSmallDeg = 16;
constexpr u32 kMidDeg = 2048;
constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u32 kMaxGrid = 2048; // grid-stride everywhere (see jet_hip.hip)
constexpr u32 kUnroll = 4;     // loads in flight per lane

#define EXT_LAUNCH_CHECK()                                                                         \
  do {                                                                                             \
    hipError_t lerr_ = hipGetLastError();                                                          \
    if (lerr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: launch error %s at %s:%d\n", hipGetErrorString(lerr_),       \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

u32 ceil_div_u32(u64 a, u64 b) { return static_cast<u32>((a + b - 1) / b); }

u32 clamp_grid(u32 g) { return g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g); }

// Block-level sum, then one global atomic per workgroup. Every thread of the
// block must call this (it synchronizes).
__device__ inline void add_block_total(unsigned long long a, unsigned long long *dst) {
  __shared__ unsigned long long red[kThreads / kWave];
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 wv = 1; wv < kThreads / kWave; ++wv) {
      a += red[wv];
    }
    if (a) {
      atomicAdd(dst, a);
    }
  }
}

// ---------------------------------------------------------------- prepare
__global__ void k_ext_prepare(View v) {
  extern __shared__ u32 ext_hist32[]; // k
  for (u32 c = threadIdx.x; c < v.k; c += kThreads) {
    ext_hist32[c] = 0;
  }
  __syncthreads();
  const u32 lane = threadIdx.x & (kWave - 1);
  const unsigned long long below = (1ull << lane) - 1ull;
  u32 bad = 0;
  for (u64 base = static_cast<u64>(blockIdx.x) * kThreads; base < v.n;
       base += static_cast<u64>(gridDim.x) * kThreads) {
    const u64 id = base + threadIdx.x;
    const u32 u = static_cast<u32>(id);
    u32 deg = 0;
    if (id < v.n) {
      u32 l = v.labels[u];
      if (l >= v.k) { // reported by the driver; keep the tables in bounds
        ++bad;
        l = 0;
      }
      v.labels16[u] = static_cast<uint16_t>(l);
      v.labels8[u] = static_cast<uint8_t>(l);
      atomicAdd(&ext_hist32[l], 1u);
      deg = static_cast<u32>(v.xadj[u + 1] - v.xadj[u]);
    }
    const bool is_l = deg > kMidDeg;
    const bool is_m = deg > kSmallDeg && !is_l;
    // wave-aggregated append: one atomic per wave and list
    const unsigned long long mm = __ballot(is_m);
    if (mm) {
      const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(mm))) - 1u;
      u32 at = 0;
      if (lane == leader) {
        at = atomicAdd(&v.tier_counts[0], static_cast<u32>(__popcll(mm)));
      }
      at = __shfl(at, leader, kWave);
      if (is_m) {
        v.m_list[at + static_cast<u32>(__popcll(mm & below))] = u;
      }
    }
    const unsigned long long lm = __ballot(is_l);
    if (lm) {
      const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(lm))) - 1u;
      u32 at = 0;
      if (lane == leader) {
        at = atomicAdd(&v.tier_counts[1], static_cast<u32>(__popcll(lm)));
      }
      at = __shfl(at, leader, kWave);
      if (is_l) {
        v.l_list[at + static_cast<u32>(__popcll(lm & below))] = u;
      }
    }
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < v.k; c += kThreads) {
    if (ext_hist32[c]) {
      atomicAdd(&v.node_cnt[c], ext_hist32[c]);
    }
  }
  if (bad) {
    atomicAdd(&v.tier_counts[2], bad);
  }
}

// One subgroup step shared by count and fill: the rows of kUnroll vertices
// per 16-lane subgroup, with the xadj reads, then the adjncy reads, then the
// label gathers issued back to back before the first one is consumed.
struct SRows {
  u32 uu[kUnroll];
  u64 row[kUnroll];
  u32 deg[kUnroll];
  bool mine[kUnroll];
  u32 cur[kUnroll];
  u32 nb[kUnroll];
  bool match[kUnroll];
};

template <typename LT>
__device__ inline void s_rows_load(
    const View &v, const LT *__restrict__ labels_s, u64 base, u32 sub, u32 slot, SRows &r
) {
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    const u64 id = base + j * 4 + sub;
    r.mine[j] = id < v.n;
    r.uu[j] = r.mine[j] ? static_cast<u32>(id) : 0u;
    r.row[j] = 0;
    r.deg[j] = 0;
    if (r.mine[j]) {
      r.row[j] = v.xadj[r.uu[j]];
      r.deg[j] = static_cast<u32>(v.xadj[r.uu[j] + 1] - r.row[j]);
    }
    r.mine[j] = r.mine[j] && r.deg[j] <= kSmallDeg; // wide tiers own the rest
  }
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    r.cur[j] = 0;
    r.nb[j] = kNone;
    if (r.mine[j]) {
      r.cur[j] = static_cast<u32>(labels_s[r.uu[j]]);
      if (slot < r.deg[j]) {
        r.nb[j] = __builtin_nontemporal_load(&v.adjncy[r.row[j] + slot]);
      }
    }
  }
  u32 cc[kUnroll];
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    cc[j] = r.nb[j] != kNone ? static_cast<u32>(labels_s[r.nb[j]]) : kNone;
  }
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    r.match[j] = r.nb[j] != kNone && cc[j] == r.cur[j];
  }
}

// ------------------------------------------------------------ count, S tier
template <typename LT>
__global__ void k_ext_count_s(View v, const LT *__restrict__ labels_s) {
  extern __shared__ unsigned long long ext_hist64[]; // k
  for (u32 c = threadIdx.x; c < v.k; c += kThreads) {
    ext_hist64[c] = 0;
  }
  __syncthreads();
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  constexpr u32 kStep = 4 * kUnroll;
  unsigned long long arcs = 0;
  for (u64 base = static_cast<u64>(wave_id) * kStep; base < v.n;
       base += static_cast<u64>(num_waves) * kStep) {
    SRows r;
    s_rows_load(v, labels_s, base, sub, slot, r);
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      const unsigned long long mask = __ballot(r.match[j]);
      const u32 cnt = static_cast<u32>(__popcll((mask >> (sub * 16)) & 0xFFFFull));
      if (r.mine[j] && slot == 0) {
        v.deg_in[r.uu[j]] = cnt;
        if (cnt) {
          atomicAdd(&ext_hist64[r.cur[j]], static_cast<unsigned long long>(cnt));
        }
        arcs += r.deg[j];
      }
    }
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < v.k; c += kThreads) {
    if (ext_hist64[c]) {
      atomicAdd(&v.arc_cnt[c], ext_hist64[c]);
    }
  }
  add_block_total(arcs, v.arcs);
}

// ------------------------------------------- count, wave / workgroup tier
// G threads per listed vertex (64: one wavefront, 256: one workgroup).
template <u32 G, typename LT>
__global__ void k_ext_count_w(
    View v, const LT *__restrict__ labels_s, const u32 *__restrict__ list, u32 count
) {
  extern __shared__ unsigned long long ext_hist64[]; // k
  __shared__ u32 red[kThreads / kWave];
  for (u32 c = threadIdx.x; c < v.k; c += kThreads) {
    ext_hist64[c] = 0;
  }
  __syncthreads();
  constexpr u32 kGroups = kThreads / G;
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  unsigned long long arcs = 0;
  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    const u32 cur = static_cast<u32>(labels_s[u]);
    u32 c = 0;
    for (u32 e0 = t; e0 < deg; e0 += kUnroll * G) {
      u32 nb[kUnroll];
      u32 lab[kUnroll];
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        const u32 e = e0 + j * G;
        nb[j] = e < deg ? __builtin_nontemporal_load(&v.adjncy[row + e]) : kNone;
      }
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        lab[j] = nb[j] != kNone ? static_cast<u32>(labels_s[nb[j]]) : kNone;
      }
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        c += (nb[j] != kNone && lab[j] == cur) ? 1u : 0u;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      c += __shfl_xor(c, off, kWave);
    }
    if constexpr (G > kWave) {
      if (lane == 0) {
        red[threadIdx.x >> 6] = c;
      }
      __syncthreads();
      if (t == 0) {
        for (u32 wv = 1; wv < G / kWave; ++wv) {
          c += red[wv];
        }
      }
    }
    if (t == 0) {
      v.deg_in[u] = c;
      if (c) {
        atomicAdd(&ext_hist64[cur], static_cast<unsigned long long>(c));
      }
      arcs += deg;
    }
    if constexpr (G > kWave) {
      __syncthreads(); // red reuse across grid-stride iterations
    }
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < v.k; c += kThreads) {
    if (ext_hist64[c]) {
      atomicAdd(&v.arc_cnt[c], ext_hist64[c]);
    }
  }
  add_block_total(arcs, v.arcs);
}

// ------------------------------------------------------------------ place
__global__ void k_ext_place(View v, const u32 *__restrict__ keys) {
  for (u64 i = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; i < v.n;
       i += static_cast<u64>(gridDim.x) * kThreads) {
    const u32 u = v.nodes[i];
    const u32 b = keys[i];
    v.pos[u] = static_cast<u32>(i);
    v.mapping[u] = static_cast<u32>(i) - v.node_off[b];
    v.sub_xadj[i] = v.deg_in[u];
    if (v.vwgt) {
      v.sub_vwgt[i] = v.vwgt[u];
    }
    if (i == 0) {
      v.sub_xadj[v.n] = 0;
    }
  }
}

// ------------------------------------------------------------- fill, S tier
template <typename LT>
__global__ void k_ext_fill_s(View v, const LT *__restrict__ labels_s) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  constexpr u32 kStep = 4 * kUnroll;
  unsigned long long arcs = 0;
  for (u64 base = static_cast<u64>(wave_id) * kStep; base < v.n;
       base += static_cast<u64>(num_waves) * kStep) {
    SRows r;
    s_rows_load(v, labels_s, base, sub, slot, r);
    u64 out[kUnroll];
    u32 mp[kUnroll];
    i32 w[kUnroll];
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      out[j] = 0;
      mp[j] = 0;
      w[j] = 1;
      if (r.match[j]) {
        out[j] = v.sub_xadj[v.pos[r.uu[j]]];
        mp[j] = v.mapping[r.nb[j]];
        if (v.adjwgt) {
          w[j] = v.adjwgt[r.row[j] + slot];
        }
      }
    }
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      const unsigned long long mask = __ballot(r.match[j]);
      const u32 sm = static_cast<u32>((mask >> (sub * 16)) & 0xFFFFull);
      if (r.match[j]) {
        const u64 o = out[j] + static_cast<u32>(__popc(sm & ((1u << slot) - 1u)));
        v.sub_adj[o] = mp[j];
        if (v.adjwgt) {
          v.sub_adjwgt[o] = w[j];
        }
      }
      if (r.mine[j] && slot == 0) {
        arcs += r.deg[j];
      }
    }
  }
  add_block_total(arcs, v.arcs);
}

// -------------------------------------------- fill, wave / workgroup tier
// A step covers kUnroll batches of G consecutive arcs. Wavefront tier: the
// write offset runs over the 64-arc batches. Workgroup tier: the per-wave
// counts of all kUnroll batches go through LDS and every thread scans them.
template <u32 G, typename LT>
__global__ void k_ext_fill_w(
    View v, const LT *__restrict__ labels_s, const u32 *__restrict__ list, u32 count
) {
  constexpr u32 kGroups = kThreads / G;
  constexpr u32 kWaves = G / kWave;
  __shared__ u32 s_cnt[kUnroll * (kThreads / kWave)];
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = t >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  unsigned long long arcs = 0;
  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    const u32 cur = static_cast<u32>(labels_s[u]);
    u64 out = v.sub_xadj[v.pos[u]];
    for (u32 e0 = 0; e0 < deg; e0 += kUnroll * G) { // uniform over the group
      u32 nb[kUnroll];
      u32 lab[kUnroll];
      u32 mp[kUnroll];
      i32 w[kUnroll];
      bool match[kUnroll];
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        const u32 e = e0 + j * G + t;
        nb[j] = e < deg ? __builtin_nontemporal_load(&v.adjncy[row + e]) : kNone;
      }
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        lab[j] = nb[j] != kNone ? static_cast<u32>(labels_s[nb[j]]) : kNone;
      }
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        match[j] = nb[j] != kNone && lab[j] == cur;
        mp[j] = 0;
        w[j] = 1;
        if (match[j]) {
          mp[j] = v.mapping[nb[j]];
          if (v.adjwgt) {
            w[j] = v.adjwgt[row + e0 + j * G + t];
          }
        }
      }
      if constexpr (G == kWave) {
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          const unsigned long long mask = __ballot(match[j]);
          if (match[j]) {
            const u64 o = out + static_cast<u32>(__popcll(mask & below));
            v.sub_adj[o] = mp[j];
            if (v.adjwgt) {
              v.sub_adjwgt[o] = w[j];
            }
          }
          out += static_cast<u32>(__popcll(mask));
        }
      } else {
        unsigned long long mask[kUnroll];
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          mask[j] = __ballot(match[j]);
          if (lane == 0) {
            s_cnt[j * kWaves + wv] = static_cast<u32>(__popcll(mask[j]));
          }
        }
        __syncthreads();
        u32 total = 0;
        u32 pre[kUnroll];
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          pre[j] = 0;
        }
#pragma unroll
        for (u32 i = 0; i < kUnroll * kWaves; ++i) {
          const u32 c = s_cnt[i];
#pragma unroll
          for (u32 j = 0; j < kUnroll; ++j) {
            if (i < j * kWaves + wv) {
              pre[j] += c;
            }
          }
          total += c;
        }
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          if (match[j]) {
            const u64 o = out + pre[j] + static_cast<u32>(__popcll(mask[j] & below));
            v.sub_adj[o] = mp[j];
            if (v.adjwgt) {
              v.sub_adjwgt[o] = w[j];
            }
          }
        }
        out += total;
        __syncthreads(); // s_cnt reuse
      }
    }
    if (t == 0) {
      arcs += deg;
    }
  }
  add_block_total(arcs, v.arcs);
}

__global__ void k_ext_rebase(
    const u64 *__restrict__ sub_xadj, u64 first, u64 base, u32 count, u64 *__restrict__ out
) {
  for (u64 i = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; i <= count;
       i += static_cast<u64>(gridDim.x) * kThreads) {
    out[i] = sub_xadj[first + i] - base;
  }
}

__global__ void k_ext_iota(u32 n, u32 *__restrict__ out) {
  for (u64 i = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += static_cast<u64>(gridDim.x) * kThreads) {
    out[i] = static_cast<u32>(i);
  }
}

void reset(void *p, size_t bytes, hipStream_t stream) {
  if (hipMemsetAsync(p, 0, bytes, stream) != hipSuccess) {
    fprintf(stderr, "kaminpar_amd: extract counter reset failed\n");
    abort();
  }
}

template <typename LT>
void count_typed(const View &v, const LT *shadow, u32 m_count, u32 l_count, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(v.k) * sizeof(unsigned long long);
  hipLaunchKernelGGL(
      k_ext_count_s<LT>, dim3(clamp_grid(ceil_div_u32(v.n, 4 * kUnroll * (kThreads / kWave)))),
      dim3(kThreads), lds, stream, v, shadow
  );
  EXT_LAUNCH_CHECK();
  if (m_count > 0) {
    hipLaunchKernelGGL(
        (k_ext_count_w<kWave, LT>), dim3(clamp_grid(ceil_div_u32(m_count, kThreads / kWave))),
        dim3(kThreads), lds, stream, v, shadow, v.m_list, m_count
    );
    EXT_LAUNCH_CHECK();
  }
  if (l_count > 0) {
    hipLaunchKernelGGL(
        (k_ext_count_w<kThreads, LT>), dim3(clamp_grid(l_count)), dim3(kThreads), lds, stream, v,
        shadow, v.l_list, l_count
    );
    EXT_LAUNCH_CHECK();
  }
}

template <typename LT>
void fill_typed(const View &v, const LT *shadow, u32 m_count, u32 l_count, hipStream_t stream) {
  hipLaunchKernelGGL(
      k_ext_fill_s<LT>, dim3(clamp_grid(ceil_div_u32(v.n, 4 * kUnroll * (kThreads / kWave)))),
      dim3(kThreads), 0, stream, v, shadow
  );
  EXT_LAUNCH_CHECK();
  if (m_count > 0) {
    hipLaunchKernelGGL(
        (k_ext_fill_w<kWave, LT>), dim3(clamp_grid(ceil_div_u32(m_count, kThreads / kWave))),
        dim3(kThreads), 0, stream, v, shadow, v.m_list, m_count
    );
    EXT_LAUNCH_CHECK();
  }
  if (l_count > 0) {
    hipLaunchKernelGGL(
        (k_ext_fill_w<kThreads, LT>), dim3(clamp_grid(l_count)), dim3(kThreads), 0, stream, v,
        shadow, v.l_list, l_count
    );
    EXT_LAUNCH_CHECK();
  }
}

} // namespace

void prepare(const View &v, hipStream_t stream) {
  reset(v.tier_counts, sizeof(u32) * 3, stream);
  reset(v.node_cnt, sizeof(u32) * v.k, stream);
  hipLaunchKernelGGL(
      k_ext_prepare, dim3(clamp_grid(ceil_div_u32(v.n, kThreads))), dim3(kThreads),
      static_cast<size_t>(v.k) * sizeof(u32), stream, v
  );
  EXT_LAUNCH_CHECK();
}

void count(const View &v, u32 m_count, u32 l_count, hipStream_t stream) {
  reset(v.arc_cnt, sizeof(unsigned long long) * v.k, stream);
  if (v.k <= 256) {
    count_typed<uint8_t>(v, v.labels8, m_count, l_count, stream);
  } else {
    count_typed<uint16_t>(v, v.labels16, m_count, l_count, stream);
  }
}

void place(const View &v, const u32 *keys, hipStream_t stream) {
  hipLaunchKernelGGL(
      k_ext_place, dim3(clamp_grid(ceil_div_u32(v.n, kThreads))), dim3(kThreads), 0, stream, v,
      keys
  );
  EXT_LAUNCH_CHECK();
}

void fill(const View &v, u32 m_count, u32 l_count, hipStream_t stream) {
  if (v.k <= 256) {
    fill_typed<uint8_t>(v, v.labels8, m_count, l_count, stream);
  } else {
    fill_typed<uint16_t>(v, v.labels16, m_count, l_count, stream);
  }
}

void rebase_xadj(
    const u64 *sub_xadj, u64 first, u64 base, u32 count, u64 *out, hipStream_t stream
) {
  hipLaunchKernelGGL(
      k_ext_rebase, dim3(clamp_grid(ceil_div_u32(static_cast<u64>(count) + 1, kThreads))),
      dim3(kThreads), 0, stream, sub_xadj, first, base, count, out
  );
  EXT_LAUNCH_CHECK();
}

void iota(u32 n, u32 *out, hipStream_t stream) {
  hipLaunchKernelGGL(
      k_ext_iota, dim3(clamp_grid(ceil_div_u32(n, kThreads))), dim3(kThreads), 0, stream, n, out
  );
  EXT_LAUNCH_CHECK();
}

} // namespace kmp_extract
