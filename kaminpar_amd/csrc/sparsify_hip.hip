// MI355X (gfx950) kernels of the threshold edge sparsification of a coarse
// graph (kmp_contract_engine_sparsified; rule in include/kaminpar_lp.h).
// Counterpart of SparsificationClusterCoarsener::
// recontract_with_threshold_sparsification (kaminpar-shm/coarsening/
// sparsification_cluster_coarsener.cc:159-228): keep the arcs heavier than the
// threshold weight T and a hashed sample of the arcs of weight T. The
// reference finds T with a quickselect on the host and recontracts; here T
// comes from a radix select on the device and the existing CSR is compacted.
//
// Kernel design (CDNA4):
//   select   four passes over the weights, most significant byte first. A pass
//            streams the weights (16 B per lane, two loads in flight) and
//            counts the next digit of those that match the digits fixed so far
//            in a per-workgroup LDS histogram, flushed with one global atomic
//            per non-empty bin and workgroup. Coarse weights are small, so in
//            the upper passes a whole wavefront usually holds one digit: it
//            then adds its lane count with a single LDS atomic instead of 64
//            on one address. A one-workgroup pick kernel scans the 256 bins,
//            fixes the digit and narrows the rank, all in device memory.
//   count    kept arcs per row. Rows are tiered as in extract_hip.hip: degree
//            <= 16 in 16-lane subgroups (four rows in flight per subgroup),
//            one wavefront per row up to 2048, one workgroup per row beyond.
//            8 B per arc (adjncy + adjwgt); the hash runs for weight T only.
//   fill     the same traversal; positions inside a row come from ballots and
//            prefix popcounts over the row's own arcs, so rows keep their
//            order and no atomic decides a position. The predicate is
//            evaluated again rather than stored as a byte per arc; View::flags
//            switches the byte form on for measurement (DESIGN.md section 15
//            has the timing of both).

#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include "sparsify_hip.h"

namespace kmp_sparsify {

namespace {

constexpr u32 kWave = 64;
constexpr u32 kThreads = 256;
constexpr u32 kSmallDeg = 16;
constexpr u32 kMidDeg = 2048;
constexpr u32 kMaxGrid = 2048; // grid-stride everywhere (see jet_hip.hip)
constexpr u32 kUnroll = 4;     // loads in flight per lane
constexpr u32 kSelGrid = 1024; // workgroups of a select pass: 256 flushes per bin at most per XCD
constexpr u32 kSelVecs = 2;    // 16-byte loads in flight per lane

static_assert(kSelectBins == kThreads, "one thread per bin in the flush and the pick");

#define SPF_LAUNCH_CHECK()                                                                         \
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

// ----------------------------------------------------------------- select
__global__ void k_sel_init(u64 rank, u32 *__restrict__ hist, SelectState *__restrict__ st) {
  for (u32 i = threadIdx.x; i < kSelectPasses * kSelectBins; i += kThreads) {
    hist[i] = 0;
  }
  if (threadIdx.x == 0) {
    st->prefix = 0;
    st->pad = 0;
    st->rank = rank;
    st->larger = 0;
    st->equal = 0;
  }
}

// One weight per lane into the workgroup's histogram. Called by all lanes of
// a wavefront together.
__device__ inline void sel_add(u32 *s_hist, u32 lane, bool valid, u32 x, u32 prefix, u32 himask,
                               u32 shift) {
  if (valid && ((x ^ prefix) & himask) == 0) {
    const u32 digit = (x >> shift) & (kSelectBins - 1);
    const u32 d0 = __builtin_amdgcn_readfirstlane(digit);
    const unsigned long long act = __ballot(true);
    const unsigned long long same = __ballot(digit == d0);
    if (same == act) {
      if (lane + 1 == static_cast<u32>(__ffsll(static_cast<long long>(act)))) {
        atomicAdd(&s_hist[d0], static_cast<u32>(__popcll(act)));
      }
    } else {
      atomicAdd(&s_hist[digit], 1u);
    }
  }
}

__global__ void k_sel_hist(
    const i32 *__restrict__ w, u32 c_m, u32 shift, const SelectState *__restrict__ st,
    u32 *__restrict__ hist
) {
  __shared__ u32 s_hist[kSelectBins];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const u32 prefix = st->prefix;
  const u32 himask = shift >= 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
  const u32 lane = threadIdx.x & (kWave - 1);
  const u64 nvec = c_m / 4;
  const int4 *__restrict__ w4 = reinterpret_cast<const int4 *>(w);
  constexpr u64 kStep = static_cast<u64>(kSelVecs) * kThreads;
  for (u64 base = static_cast<u64>(blockIdx.x) * kStep; base < nvec;
       base += static_cast<u64>(gridDim.x) * kStep) {
    int4 a[kSelVecs];
    bool ok[kSelVecs];
#pragma unroll
    for (u32 j = 0; j < kSelVecs; ++j) {
      const u64 idx = base + j * kThreads + threadIdx.x;
      ok[j] = idx < nvec;
      a[j] = ok[j] ? w4[idx] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (u32 j = 0; j < kSelVecs; ++j) {
      sel_add(s_hist, lane, ok[j], static_cast<u32>(a[j].x), prefix, himask, shift);
      sel_add(s_hist, lane, ok[j], static_cast<u32>(a[j].y), prefix, himask, shift);
      sel_add(s_hist, lane, ok[j], static_cast<u32>(a[j].z), prefix, himask, shift);
      sel_add(s_hist, lane, ok[j], static_cast<u32>(a[j].w), prefix, himask, shift);
    }
  }
  if (blockIdx.x == 0) { // the c_m % 4 weights behind the last vector
    const u64 idx = nvec * 4 + threadIdx.x;
    const bool ok = idx < c_m;
    sel_add(s_hist, lane, ok, ok ? static_cast<u32>(w[idx]) : 0u, prefix, himask, shift);
  }
  __syncthreads();
  const u32 c = s_hist[threadIdx.x];
  if (c) {
    atomicAdd(&hist[threadIdx.x], c);
  }
}

// One workgroup: the bin that holds the rank-th smallest matching weight.
__global__ void k_sel_pick(const u32 *__restrict__ hist, u32 shift, SelectState *__restrict__ st) {
  __shared__ u64 s_sum[kSelectBins];
  const u32 t = threadIdx.x;
  const u64 c = hist[t];
  s_sum[t] = c;
  __syncthreads();
  for (u32 off = 1; off < kSelectBins; off <<= 1) {
    const u64 add = t >= off ? s_sum[t - off] : 0;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  const u64 incl = s_sum[t];
  const u64 excl = incl - c;
  const u64 total = s_sum[kSelectBins - 1];
  const u64 rank = st->rank;
  __syncthreads(); // every thread has read the rank before one replaces it
  if (excl < rank && rank <= incl) { // exactly one bin: 1 <= rank <= total
    st->prefix |= t << shift;
    st->rank = rank - excl;
    st->larger += total - incl;
    if (shift == 0) {
      st->equal = c;
    }
  }
}

// ------------------------------------------------------------------- rule
struct Rule {
  u32 T;
  u64 equal;
  u64 limit; // include * 2^32
  u64 seed;
};

__device__ inline Rule load_rule(const View &v) {
  Rule r;
  r.T = v.st->prefix;
  r.equal = v.st->equal;
  r.limit = (v.target - v.st->larger) << 32; // 1 <= include <= equal < 2^32
  r.seed = v.seed;
  return r;
}

__device__ inline u64 fmix64(u64 x) { // the Murmur3 finalizer
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

__device__ inline bool keep_arc(const Rule &r, u32 u, u32 nb, i32 w) {
  const u32 x = static_cast<u32>(w); // weights are positive
  if (x != r.T) {
    return x > r.T;
  }
  const u32 lo = u < nb ? u : nb;
  const u32 hi = u < nb ? nb : u;
  const u64 h = fmix64(((static_cast<u64>(hi) << 32) | lo) + r.seed) & 0xFFFFFFFFull;
  return h * r.equal < r.limit;
}

// ---------------------------------------------------------------- prepare
__global__ void k_spf_prepare(View v) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (u64 base = static_cast<u64>(blockIdx.x) * kThreads; base < v.n;
       base += static_cast<u64>(gridDim.x) * kThreads) {
    const u64 id = base + threadIdx.x;
    const u32 u = static_cast<u32>(id);
    u32 deg = 0;
    if (id < v.n) {
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
}

// One subgroup step shared by count and fill: the rows of kUnroll vertices
// per 16-lane subgroup, with the xadj reads, then the adjncy and adjwgt reads
// issued back to back before the first one is consumed.
struct SRows {
  u32 uu[kUnroll];
  u64 row[kUnroll];
  bool mine[kUnroll];
  u32 nb[kUnroll];
  i32 w[kUnroll];
  bool keep[kUnroll];
};

template <bool kFill>
__device__ inline void s_rows_load(const View &v, const Rule &rule, u64 base, u32 sub, u32 slot,
                                   SRows &r) {
  u32 deg[kUnroll];
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    const u64 id = base + j * 4 + sub;
    r.mine[j] = id < v.n;
    r.uu[j] = r.mine[j] ? static_cast<u32>(id) : 0u;
    r.row[j] = 0;
    deg[j] = 0;
    if (r.mine[j]) {
      r.row[j] = v.xadj[r.uu[j]];
      deg[j] = static_cast<u32>(v.xadj[r.uu[j] + 1] - r.row[j]);
    }
    r.mine[j] = r.mine[j] && deg[j] <= kSmallDeg; // wide tiers own the rest
  }
  bool have[kUnroll];
  if (kFill && v.flags != nullptr) {
    uint8_t f[kUnroll];
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      have[j] = r.mine[j] && slot < deg[j];
      f[j] = have[j] ? v.flags[r.row[j] + slot] : uint8_t{0};
    }
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      r.keep[j] = f[j] != 0;
      r.nb[j] = 0;
      r.w[j] = 0;
      if (r.keep[j]) {
        r.nb[j] = __builtin_nontemporal_load(&v.adjncy[r.row[j] + slot]);
        r.w[j] = __builtin_nontemporal_load(&v.adjwgt[r.row[j] + slot]);
      }
    }
    return;
  }
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    have[j] = r.mine[j] && slot < deg[j];
    r.nb[j] = 0;
    r.w[j] = 0;
    if (have[j]) {
      r.nb[j] = __builtin_nontemporal_load(&v.adjncy[r.row[j] + slot]);
      r.w[j] = __builtin_nontemporal_load(&v.adjwgt[r.row[j] + slot]);
    }
  }
#pragma unroll
  for (u32 j = 0; j < kUnroll; ++j) {
    r.keep[j] = have[j] && keep_arc(rule, r.uu[j], r.nb[j], r.w[j]);
    if (!kFill && v.flags != nullptr && have[j]) {
      v.flags[r.row[j] + slot] = r.keep[j] ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------ count, S tier
__global__ void k_spf_count_s(View v) {
  const Rule rule = load_rule(v);
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  constexpr u32 kStep = 4 * kUnroll;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    v.cnt[v.n] = 0;
  }
  for (u64 base = static_cast<u64>(wave_id) * kStep; base < v.n;
       base += static_cast<u64>(num_waves) * kStep) {
    SRows r;
    s_rows_load<false>(v, rule, base, sub, slot, r);
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      const unsigned long long mask = __ballot(r.keep[j]);
      const u32 c = static_cast<u32>(__popcll((mask >> (sub * 16)) & 0xFFFFull));
      if (r.mine[j] && slot == 0) {
        v.cnt[r.uu[j]] = c;
      }
    }
  }
}

// ------------------------------------------- count, wave / workgroup tier
// G threads per listed vertex (64: one wavefront, 256: one workgroup).
template <u32 G>
__global__ void k_spf_count_w(View v, const u32 *__restrict__ list, u32 which) {
  __shared__ u32 red[kThreads / kWave];
  const Rule rule = load_rule(v);
  const u32 count = v.tier_counts[which];
  constexpr u32 kGroups = kThreads / G;
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    u32 c = 0;
    for (u32 e0 = t; e0 < deg; e0 += kUnroll * G) {
      u32 nb[kUnroll];
      i32 w[kUnroll];
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        const u32 e = e0 + j * G;
        nb[j] = 0;
        w[j] = 0;
        if (e < deg) {
          nb[j] = __builtin_nontemporal_load(&v.adjncy[row + e]);
          w[j] = __builtin_nontemporal_load(&v.adjwgt[row + e]);
        }
      }
#pragma unroll
      for (u32 j = 0; j < kUnroll; ++j) {
        const bool k = e0 + j * G < deg && keep_arc(rule, u, nb[j], w[j]);
        if (v.flags != nullptr && e0 + j * G < deg) {
          v.flags[row + e0 + j * G] = k ? 1 : 0;
        }
        c += k ? 1u : 0u;
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
      v.cnt[u] = c;
    }
    if constexpr (G > kWave) {
      __syncthreads(); // red reuse across grid-stride iterations
    }
  }
}

// ------------------------------------------------------------- fill, S tier
__global__ void k_spf_fill_s(View v) {
  const Rule rule = load_rule(v);
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 sub = lane >> 4;
  const u32 slot = lane & 15;
  const u32 wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u32 num_waves = (gridDim.x * blockDim.x) >> 6;
  constexpr u32 kStep = 4 * kUnroll;
  for (u64 base = static_cast<u64>(wave_id) * kStep; base < v.n;
       base += static_cast<u64>(num_waves) * kStep) {
    SRows r;
    s_rows_load<true>(v, rule, base, sub, slot, r);
    u64 out[kUnroll];
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      out[j] = r.keep[j] ? v.cnt[r.uu[j]] : 0;
    }
#pragma unroll
    for (u32 j = 0; j < kUnroll; ++j) {
      const unsigned long long mask = __ballot(r.keep[j]);
      const u32 sm = static_cast<u32>((mask >> (sub * 16)) & 0xFFFFull);
      if (r.keep[j]) {
        const u64 o = out[j] + static_cast<u32>(__popc(sm & ((1u << slot) - 1u)));
        v.out_adj[o] = r.nb[j];
        v.out_wgt[o] = r.w[j];
      }
    }
  }
}

// -------------------------------------------- fill, wave / workgroup tier
// A step covers kUnroll batches of G consecutive arcs. Wavefront tier: the
// write offset runs over the 64-arc batches. Workgroup tier: the per-wave
// counts of all kUnroll batches go through LDS and every thread scans them.
template <u32 G>
__global__ void k_spf_fill_w(View v, const u32 *__restrict__ list, u32 which) {
  constexpr u32 kGroups = kThreads / G;
  constexpr u32 kWaves = G / kWave;
  __shared__ u32 s_cnt[kUnroll * (kThreads / kWave)];
  const Rule rule = load_rule(v);
  const u32 count = v.tier_counts[which];
  const u32 t = threadIdx.x % G;
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wv = t >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const u32 group_id = blockIdx.x * kGroups + threadIdx.x / G;
  const u32 num_groups = gridDim.x * kGroups;
  for (u32 vid = group_id; vid < count; vid += num_groups) {
    const u32 u = list[vid];
    const u64 row = v.xadj[u];
    const u32 deg = static_cast<u32>(v.xadj[u + 1] - row);
    u64 out = v.cnt[u];
    for (u32 e0 = 0; e0 < deg; e0 += kUnroll * G) { // uniform over the group
      u32 nb[kUnroll];
      i32 w[kUnroll];
      bool keep[kUnroll];
      if (v.flags != nullptr) {
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          const u32 e = e0 + j * G + t;
          keep[j] = e < deg && v.flags[row + e] != 0;
        }
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          const u32 e = e0 + j * G + t;
          nb[j] = 0;
          w[j] = 0;
          if (keep[j]) {
            nb[j] = __builtin_nontemporal_load(&v.adjncy[row + e]);
            w[j] = __builtin_nontemporal_load(&v.adjwgt[row + e]);
          }
        }
      } else {
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          const u32 e = e0 + j * G + t;
          nb[j] = 0;
          w[j] = 0;
          if (e < deg) {
            nb[j] = __builtin_nontemporal_load(&v.adjncy[row + e]);
            w[j] = __builtin_nontemporal_load(&v.adjwgt[row + e]);
          }
        }
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          keep[j] = e0 + j * G + t < deg && keep_arc(rule, u, nb[j], w[j]);
        }
      }
      if constexpr (G == kWave) {
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          const unsigned long long mask = __ballot(keep[j]);
          if (keep[j]) {
            const u64 o = out + static_cast<u32>(__popcll(mask & below));
            v.out_adj[o] = nb[j];
            v.out_wgt[o] = w[j];
          }
          out += static_cast<u32>(__popcll(mask));
        }
      } else {
        unsigned long long mask[kUnroll];
#pragma unroll
        for (u32 j = 0; j < kUnroll; ++j) {
          mask[j] = __ballot(keep[j]);
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
          if (keep[j]) {
            const u64 o = out + pre[j] + static_cast<u32>(__popcll(mask[j] & below));
            v.out_adj[o] = nb[j];
            v.out_wgt[o] = w[j];
          }
        }
        out += total;
        __syncthreads(); // s_cnt reuse
      }
    }
  }
}

// The wide tiers read their list length on the device, so that no launch
// waits for a read-back: a grid sized for the worst case a level can have,
// whose spare workgroups find nothing to do.
u32 wave_tier_grid(u32 n) { return clamp_grid(ceil_div_u32(n, 4 * (kThreads / kWave))); }
u32 group_tier_grid(u32 n) {
  const u32 g = ceil_div_u32(n, 16);
  return g < 1 ? 1 : (g > 512 ? 512 : g);
}

} // namespace

void select(const i32 *w, u32 c_m, u64 rank, u32 *hist, SelectState *st, hipStream_t stream) {
  hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(kThreads), 0, stream, rank, hist, st);
  SPF_LAUNCH_CHECK();
  u32 grid = ceil_div_u32(c_m / 4, static_cast<u64>(kSelVecs) * kThreads);
  grid = grid < 1 ? 1 : (grid > kSelGrid ? kSelGrid : grid);
  for (u32 pass = 0; pass < kSelectPasses; ++pass) {
    const u32 shift = 24 - 8 * pass;
    hipLaunchKernelGGL(
        k_sel_hist, dim3(grid), dim3(kThreads), 0, stream, w, c_m, shift, st,
        hist + pass * kSelectBins
    );
    SPF_LAUNCH_CHECK();
    hipLaunchKernelGGL(
        k_sel_pick, dim3(1), dim3(kThreads), 0, stream, hist + pass * kSelectBins, shift, st
    );
    SPF_LAUNCH_CHECK();
  }
}

void prepare(const View &v, hipStream_t stream) {
  if (hipMemsetAsync(v.tier_counts, 0, sizeof(u32) * 2, stream) != hipSuccess) {
    fprintf(stderr, "kaminpar_amd: sparsify counter reset failed\n");
    abort();
  }
  hipLaunchKernelGGL(
      k_spf_prepare, dim3(clamp_grid(ceil_div_u32(v.n, kThreads))), dim3(kThreads), 0, stream, v
  );
  SPF_LAUNCH_CHECK();
}

void count(const View &v, hipStream_t stream) {
  hipLaunchKernelGGL(
      k_spf_count_s, dim3(clamp_grid(ceil_div_u32(v.n, 4 * kUnroll * (kThreads / kWave)))),
      dim3(kThreads), 0, stream, v
  );
  SPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(
      (k_spf_count_w<kWave>), dim3(wave_tier_grid(v.n)), dim3(kThreads), 0, stream, v, v.m_list, 0u
  );
  SPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(
      (k_spf_count_w<kThreads>), dim3(group_tier_grid(v.n)), dim3(kThreads), 0, stream, v,
      v.l_list, 1u
  );
  SPF_LAUNCH_CHECK();
}

void fill(const View &v, hipStream_t stream) {
  hipLaunchKernelGGL(
      k_spf_fill_s, dim3(clamp_grid(ceil_div_u32(v.n, 4 * kUnroll * (kThreads / kWave)))),
      dim3(kThreads), 0, stream, v
  );
  SPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(
      (k_spf_fill_w<kWave>), dim3(wave_tier_grid(v.n)), dim3(kThreads), 0, stream, v, v.m_list, 0u
  );
  SPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(
      (k_spf_fill_w<kThreads>), dim3(group_tier_grid(v.n)), dim3(kThreads), 0, stream, v, v.l_list,
      1u
  );
  SPF_LAUNCH_CHECK();
}

} // namespace kmp_sparsify
