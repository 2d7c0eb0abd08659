// Kernels that keep label-shaped arrays on the device between the stages of
// the multilevel chain (launch interface: resident_hip.h):
//   k_project     fine.labels[u] = coarse.labels[mapping[u]]
//   k_iso_flags   degree-0 flags, maximum degree and isolated count of a CSR
//   k_iso_weights node weights of the compacted isolated vertices
// The drivers (kmp_lp_project, kmp_contract_engine) are in lp_hip.hip.

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "resident_hip.h"

namespace kmp_resident {

namespace {

constexpr u32 kWave = 64;
constexpr u32 kThreads = 256;
constexpr u32 kMaxGrid = 2048;  // memory-bound: cap the grid, stride the rest
constexpr u32 kPerLane = 4;     // vertices per lane per trip (k_project)

#define RES_HIP_CHECK(expr)                                                                        \
  do {                                                                                             \
    hipError_t herr_ = (expr);                                                                     \
    if (herr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: HIP error %s at %s:%d\n", hipGetErrorString(herr_),          \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

#define RES_LAUNCH_CHECK() RES_HIP_CHECK(hipGetLastError())

// A trip covers kThreads * kPerLane consecutive vertices per workgroup; lane t
// takes t, t + 256, t + 512, t + 768 of them, so every load of the mapping and
// every store is one coalesced 256-byte wave access. The loop is written in
// three stages over registers so that the kPerLane mapping loads are all
// issued before the first gather and the gathers before the first store; the
// gather table (1, 2 or 4 bytes per coarse vertex) is what the caches hold.
template <typename L>
__global__ __launch_bounds__(kThreads) void k_project(
    const u32 *__restrict__ map, const L *__restrict__ coarse, u32 n, u32 *__restrict__ out
) {
  constexpr u64 kTrip = static_cast<u64>(kThreads) * kPerLane;
  const u64 stride = static_cast<u64>(gridDim.x) * kTrip;
  for (u64 base = static_cast<u64>(blockIdx.x) * kTrip; base < n; base += stride) {
    const u64 first = base + threadIdx.x;
    u32 c[kPerLane];
    u32 l[kPerLane];
    if (base + kTrip <= n) { // full trip: no per-element bounds checks
#pragma unroll
      for (u32 j = 0; j < kPerLane; ++j) {
        c[j] = map[first + j * kThreads];
      }
#pragma unroll
      for (u32 j = 0; j < kPerLane; ++j) {
        l[j] = static_cast<u32>(coarse[c[j]]);
      }
#pragma unroll
      for (u32 j = 0; j < kPerLane; ++j) {
        out[first + j * kThreads] = l[j];
      }
    } else {
#pragma unroll
      for (u32 j = 0; j < kPerLane; ++j) {
        const u64 u = first + j * kThreads;
        c[j] = u < n ? map[u] : 0xFFFFFFFFu;
      }
#pragma unroll
      for (u32 j = 0; j < kPerLane; ++j) {
        l[j] = c[j] != 0xFFFFFFFFu ? static_cast<u32>(coarse[c[j]]) : 0u;
      }
#pragma unroll
      for (u32 j = 0; j < kPerLane; ++j) {
        const u64 u = first + j * kThreads;
        if (u < n) {
          out[u] = l[j];
        }
      }
    }
  }
}

// Grid-stride over the vertices; each workgroup folds its maximum degree and
// isolated count through shuffles and LDS into one atomic each.
__global__ __launch_bounds__(kThreads) void k_iso_flags(
    u32 n, const u64 *__restrict__ xadj, uint8_t *__restrict__ flags, u32 *__restrict__ stats
) {
  __shared__ u32 s_max[kThreads / kWave];
  __shared__ u32 s_cnt[kThreads / kWave];
  u32 maxd = 0, cnt = 0;
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads;
  for (u64 u = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; u < n; u += stride) {
    const u32 deg = static_cast<u32>(xadj[u + 1] - xadj[u]);
    flags[u] = deg == 0 ? 1 : 0;
    maxd = deg > maxd ? deg : maxd;
    cnt += deg == 0 ? 1u : 0u;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const u32 om = __shfl_down(maxd, off, kWave);
    maxd = om > maxd ? om : maxd;
    cnt += __shfl_down(cnt, off, kWave);
  }
  const u32 lane = threadIdx.x & (kWave - 1);
  const u32 wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_max[wave] = maxd;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 w = 1; w < kThreads / kWave; ++w) {
      maxd = s_max[w] > maxd ? s_max[w] : maxd;
      cnt += s_cnt[w];
    }
    if (maxd > 0) {
      atomicMax(&stats[0], maxd);
    }
    if (cnt > 0) {
      atomicAdd(&stats[1], cnt);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_iso_weights(
    const u32 *__restrict__ ids, u32 count, const i32 *__restrict__ vwgt, i32 *__restrict__ out
) {
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i < count) {
    out[i] = vwgt != nullptr ? vwgt[ids[i]] : 1;
  }
}

u32 capped_grid(u64 items, u64 per_block) {
  const u64 blocks = (items + per_block - 1) / per_block;
  return static_cast<u32>(blocks < kMaxGrid ? (blocks > 0 ? blocks : 1) : kMaxGrid);
}

} // namespace

void project(
    const u32 *map, const void *coarse_labels, int label_bytes, u32 n, u32 *out,
    hipStream_t stream
) {
  if (n == 0) {
    return;
  }
  const dim3 grid(capped_grid(n, static_cast<u64>(kThreads) * kPerLane));
  if (label_bytes == 1) {
    hipLaunchKernelGGL(k_project<uint8_t>, grid, dim3(kThreads), 0, stream, map,
                       static_cast<const uint8_t *>(coarse_labels), n, out);
  } else if (label_bytes == 2) {
    hipLaunchKernelGGL(k_project<uint16_t>, grid, dim3(kThreads), 0, stream, map,
                       static_cast<const uint16_t *>(coarse_labels), n, out);
  } else {
    hipLaunchKernelGGL(k_project<u32>, grid, dim3(kThreads), 0, stream, map,
                       static_cast<const u32 *>(coarse_labels), n, out);
  }
  RES_LAUNCH_CHECK();
}

void iso_flags(u32 n, const u64 *xadj, uint8_t *flags, u32 *stats, hipStream_t stream) {
  RES_HIP_CHECK(hipMemsetAsync(stats, 0, sizeof(u32) * 2, stream));
  if (n == 0) {
    return;
  }
  hipLaunchKernelGGL(k_iso_flags, dim3(capped_grid(n, kThreads)), dim3(kThreads), 0, stream, n,
                     xadj, flags, stats);
  RES_LAUNCH_CHECK();
}

void iso_select(
    void *temp, size_t &temp_bytes, const uint8_t *flags, u32 n, u32 *ids_out, u32 *count_out,
    hipStream_t stream
) {
  RES_HIP_CHECK(rocprim::select(
      temp, temp_bytes, rocprim::counting_iterator<u32>(0), flags, ids_out, count_out, n, stream
  ));
}

void iso_weights(const u32 *ids, u32 count, const i32 *vwgt, i32 *out, hipStream_t stream) {
  if (count == 0) {
    return;
  }
  hipLaunchKernelGGL(k_iso_weights, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, ids, count, vwgt, out);
  RES_LAUNCH_CHECK();
}

} // namespace kmp_resident
