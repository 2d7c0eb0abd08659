// Kernels of the V-cycle (launch interface: vcycle_hip.h):
//   k_restrict        coarse.labels[mapping[u]] = fine.communities[u]
//   k_restrict_check  number of u with coarse.labels[mapping[u]] != communities[u]
//   k_gather          out[i] = src[ids[i]] (communities of the isolated vertices)
//   k_block_weights   block weights of a partition, wave-aggregated atomics
// All are streaming passes with one thread per fine vertex, a capped grid and
// no table sized by k. The drivers are in lp_hip.hip.

#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include "vcycle_hip.h"

namespace kmp_vcycle {

namespace {

constexpr u32 kWave = 64;
constexpr u32 kThreads = 256;
constexpr u32 kMaxGrid = 2048; // memory-bound: cap the grid, stride the rest
constexpr u32 kPerLane = 4;    // vertices per lane per trip

#define VC_HIP_CHECK(expr)                                                                         \
  do {                                                                                             \
    hipError_t herr_ = (expr);                                                                     \
    if (herr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: HIP error %s at %s:%d\n", hipGetErrorString(herr_),          \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

#define VC_LAUNCH_CHECK() VC_HIP_CHECK(hipGetLastError())

// The trip shape of k_project: lane t takes t, t + 256, t + 512, t + 768 of a
// trip's 1024 consecutive vertices, so the loads of the mapping and of the
// communities are coalesced 256-byte wave accesses, all issued before the
// first 4-byte scatter.
__global__ __launch_bounds__(kThreads) void k_restrict(
    const u32 *__restrict__ map, const u32 *__restrict__ comm, u32 n, u32 *__restrict__ coarse,
    u32 coarse_n
) {
  constexpr u64 kTrip = static_cast<u64>(kThreads) * kPerLane;
  const u64 stride = static_cast<u64>(gridDim.x) * kTrip;
  for (u64 base = static_cast<u64>(blockIdx.x) * kTrip; base < n; base += stride) {
    const u64 first = base + threadIdx.x;
    u32 c[kPerLane];
    u32 l[kPerLane];
#pragma unroll
    for (u32 j = 0; j < kPerLane; ++j) {
      const u64 u = first + j * kThreads;
      // past n: a slot no coarse graph has (coarse_n <= n < 2^32 - 1)
      c[j] = u < n ? map[u] : 0xFFFFFFFFu;
      l[j] = u < n ? comm[u] : 0u;
    }
#pragma unroll
    for (u32 j = 0; j < kPerLane; ++j) {
      if (c[j] < coarse_n) { // skips lanes past n and entries outside the coarse graph
        coarse[c[j]] = l[j];
      }
    }
  }
}

// Same trips; the gathers of a trip are in flight together. Each workgroup
// folds its count through shuffles and LDS into one atomic.
__global__ __launch_bounds__(kThreads) void k_restrict_check(
    const u32 *__restrict__ map, const u32 *__restrict__ comm, u32 n,
    const u32 *__restrict__ coarse, u32 coarse_n, unsigned long long *__restrict__ count_out
) {
  __shared__ u32 s_cnt[kThreads / kWave];
  constexpr u64 kTrip = static_cast<u64>(kThreads) * kPerLane;
  const u64 stride = static_cast<u64>(gridDim.x) * kTrip;
  u32 cnt = 0;
  for (u64 base = static_cast<u64>(blockIdx.x) * kTrip; base < n; base += stride) {
    const u64 first = base + threadIdx.x;
    u32 c[kPerLane];
    u32 l[kPerLane];
    u32 got[kPerLane];
    bool valid[kPerLane];
#pragma unroll
    for (u32 j = 0; j < kPerLane; ++j) {
      const u64 u = first + j * kThreads;
      valid[j] = u < n;
      c[j] = valid[j] ? map[u] : 0u;
      l[j] = valid[j] ? comm[u] : 0u;
    }
#pragma unroll
    for (u32 j = 0; j < kPerLane; ++j) {
      got[j] = valid[j] && c[j] < coarse_n ? coarse[c[j]] : l[j];
    }
#pragma unroll
    for (u32 j = 0; j < kPerLane; ++j) {
      // a mapping entry outside the coarse graph counts as a mismatch
      cnt += valid[j] && (c[j] >= coarse_n || got[j] != l[j]) ? 1u : 0u;
    }
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, kWave);
  }
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 w = 1; w < kThreads / kWave; ++w) {
      cnt += s_cnt[w];
    }
    if (cnt > 0) {
      atomicAdd(count_out, static_cast<unsigned long long>(cnt));
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_gather(
    const u32 *__restrict__ ids, u32 count, const u32 *__restrict__ src, u32 *__restrict__ out
) {
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads;
  for (u64 i = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += stride) {
    out[i] = src[ids[i]];
  }
}

// One wave per 64 consecutive vertices per trip. The wave peels its distinct
// labels one at a time: the lowest pending lane names a label, the lanes
// holding it sum their weights through shuffles, lane 0 adds the sum with one
// atomic. A wave of a partition with few blocks issues few atomics, and at
// large k the 64 lanes of a trip cost at most 64 rounds.
__global__ __launch_bounds__(kThreads) void k_block_weights(
    const u32 *__restrict__ labels, const i32 *__restrict__ vwgt, u32 n, u32 k,
    unsigned long long *__restrict__ weights
) {
  const u32 lane = threadIdx.x & (kWave - 1);
  const u64 wave_id = (static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x) / kWave;
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads; // vertices per trip of the grid
  for (u64 base = wave_id * kWave; base < n; base += stride) { // wave-uniform
    const u64 u = base + lane;
    const bool valid = u < n;
    const u32 l = valid ? labels[u] : 0u;
    const unsigned long long w =
        valid ? static_cast<unsigned long long>(vwgt != nullptr ? vwgt[u] : 1) : 0ull;
    bool todo = valid && l < k;
    for (;;) {
      const unsigned long long pending = __ballot(todo);
      if (pending == 0) {
        break;
      }
      const int leader = __ffsll(static_cast<long long>(pending)) - 1;
      const u32 cur = static_cast<u32>(__shfl(static_cast<int>(l), leader, kWave));
      const bool mine = todo && l == cur;
      unsigned long long s = mine ? w : 0ull;
      for (int off = kWave / 2; off > 0; off >>= 1) {
        s += __shfl_down(s, off, kWave);
      }
      if (lane == 0 && s != 0) {
        atomicAdd(&weights[cur], s);
      }
      todo = todo && !mine;
    }
  }
}

u32 capped_grid(u64 items, u64 per_block) {
  const u64 blocks = (items + per_block - 1) / per_block;
  return static_cast<u32>(blocks < kMaxGrid ? (blocks > 0 ? blocks : 1) : kMaxGrid);
}

} // namespace

void restrict_labels(
    const u32 *map, const u32 *comm, u32 n, u32 *coarse, u32 coarse_n, hipStream_t stream
) {
  if (n == 0) {
    return;
  }
  const dim3 grid(capped_grid(n, static_cast<u64>(kThreads) * kPerLane));
  hipLaunchKernelGGL(k_restrict, grid, dim3(kThreads), 0, stream, map, comm, n, coarse,
                     coarse_n);
  VC_LAUNCH_CHECK();
}

void restrict_mismatches(
    const u32 *map, const u32 *comm, u32 n, const u32 *coarse, u32 coarse_n,
    unsigned long long *count_out, hipStream_t stream
) {
  VC_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(unsigned long long), stream));
  if (n == 0) {
    return;
  }
  const dim3 grid(capped_grid(n, static_cast<u64>(kThreads) * kPerLane));
  hipLaunchKernelGGL(k_restrict_check, grid, dim3(kThreads), 0, stream, map, comm, n, coarse,
                     coarse_n, count_out);
  VC_LAUNCH_CHECK();
}

void gather(const u32 *ids, u32 count, const u32 *src, u32 *out, hipStream_t stream) {
  if (count == 0) {
    return;
  }
  hipLaunchKernelGGL(k_gather, dim3(capped_grid(count, kThreads)), dim3(kThreads), 0, stream, ids,
                     count, src, out);
  VC_LAUNCH_CHECK();
}

void block_weights(
    const u32 *labels, const i32 *vwgt, u32 n, u32 k, unsigned long long *weights,
    hipStream_t stream
) {
  VC_HIP_CHECK(hipMemsetAsync(weights, 0, sizeof(unsigned long long) * k, stream));
  if (n == 0) {
    return;
  }
  hipLaunchKernelGGL(k_block_weights, dim3(capped_grid(n, kThreads)), dim3(kThreads), 0, stream,
                     labels, vwgt, n, k, weights);
  VC_LAUNCH_CHECK();
}

} // namespace kmp_vcycle
