// Kernels of the edge-list ingestion (launch interface: edges_hip.h; rule:
// include/kaminpar_lp.h, "engines from edge lists"):
//   k_scan_ids    largest id of the list, for an inferred n
//   k_pack        validation + the two packed 64-bit arc keys of every pair
//   k_check_sums  saturated sums among the collapsed arcs
//   k_build       adjncy / adjwgt and the row-end marks of xadj
// Sorting, collapsing and the closing scan of xadj are rocprim's. No kernel
// here indexes an array by a vertex id before the driver has read the error
// counters: k_scan_ids and k_pack only compare ids, k_build runs after.

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "edges_hip.h"

namespace kmp_edges {

namespace {

using kmp::i64;

constexpr u32 kWave = 64;
constexpr u32 kThreads = 256;
constexpr u32 kMaxGrid = 2048; // memory-bound: cap the grid, stride the rest
constexpr u32 kGroup = 4;      // pairs (pack) or arcs (build) per lane per trip

#define EDGES_HIP_CHECK(expr)                                                                      \
  do {                                                                                             \
    hipError_t herr_ = (expr);                                                                     \
    if (herr_ != hipSuccess) {                                                                     \
      fprintf(stderr, "kaminpar_amd: HIP error %s at %s:%d\n", hipGetErrorString(herr_),          \
              __FILE__, __LINE__);                                                                 \
      abort();                                                                                     \
    }                                                                                              \
  } while (0)

#define EDGES_LAUNCH_CHECK() EDGES_HIP_CHECK(hipGetLastError())

u32 capped_grid(u64 items, u64 per_block) {
  const u64 blocks = (items + per_block - 1) / per_block;
  return static_cast<u32>(blocks < kMaxGrid ? (blocks > 0 ? blocks : 1) : kMaxGrid);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// kGroup consecutive elements from p + base. kVec: p + base is 16-byte
// aligned, so the group is one (4-byte elements) or two (8-byte) 16-byte loads.
template <bool kVec, typename T>
__device__ inline void load_group(const T *__restrict__ p, u64 base, T (&out)[kGroup]) {
  if constexpr (kVec && sizeof(T) == 4) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p + base);
    out[0] = static_cast<T>(v.x);
    out[1] = static_cast<T>(v.y);
    out[2] = static_cast<T>(v.z);
    out[3] = static_cast<T>(v.w);
  } else if constexpr (kVec && sizeof(T) == 8) {
    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p + base);
    const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(p + base + 2);
    out[0] = static_cast<T>(a.x);
    out[1] = static_cast<T>(a.y);
    out[2] = static_cast<T>(b.x);
    out[3] = static_cast<T>(b.y);
  } else {
#pragma unroll
    for (u32 j = 0; j < kGroup; ++j) {
      out[j] = p[base + j];
    }
  }
}

// Whether v is an id at all (non-negative, below 2^32), and its value.
__device__ inline bool id_value(u32 v, u32 &out) {
  out = v;
  return true;
}
__device__ inline bool id_value(i32 v, u32 &out) {
  out = static_cast<u32>(v);
  return v >= 0;
}
__device__ inline bool id_value(i64 v, u32 &out) {
  out = static_cast<u32>(v);
  return v >= 0 && v <= 0xFFFFFFFFll;
}

// Adds the workgroup's nonzero per-lane counts to counters[0 .. kCount):
// through LDS atomics of the lanes that have any, then one global atomic per
// nonzero counter. Every lane of the workgroup calls this once.
template <u32 kCount>
__device__ inline void flush_counts(const u32 (&mine)[kCount], u64 *__restrict__ counters) {
  __shared__ u32 s_cnt[kCount];
  if (threadIdx.x < kCount) {
    s_cnt[threadIdx.x] = 0;
  }
  __syncthreads();
#pragma unroll
  for (u32 c = 0; c < kCount; ++c) {
    if (mine[c] != 0) {
      atomicAdd(&s_cnt[c], mine[c]);
    }
  }
  __syncthreads();
  if (threadIdx.x < kCount && s_cnt[threadIdx.x] != 0) {
    atomicAdd(reinterpret_cast<unsigned long long *>(counters) + threadIdx.x,
              static_cast<unsigned long long>(s_cnt[threadIdx.x]));
  }
}

template <typename IdT, bool kVec>
__global__ __launch_bounds__(kThreads) void k_scan_ids(
    const IdT *__restrict__ src, const IdT *__restrict__ dst, u64 num_pairs,
    u64 *__restrict__ counters
) {
  __shared__ u32 s_max;
  if (threadIdx.x == 0) {
    s_max = 0;
  }
  u32 maxid = 0;
  u32 cnt[1] = {0}; // kBadIds
  auto see = [&](IdT a, IdT b) {
    u32 u, v;
    const bool ok = id_value(a, u) & id_value(b, v);
    if (ok) {
      const u32 hi = u > v ? u : v;
      maxid = hi > maxid ? hi : maxid;
    } else {
      ++cnt[0];
    }
  };
  const u64 groups = num_pairs / kGroup;
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads;
  for (u64 g = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; g < groups; g += stride) {
    IdT a[kGroup], b[kGroup];
    load_group<kVec>(src, g * kGroup, a);
    load_group<kVec>(dst, g * kGroup, b);
#pragma unroll
    for (u32 j = 0; j < kGroup; ++j) {
      see(a[j], b[j]);
    }
  }
  const u64 tail = groups * kGroup + threadIdx.x;
  if (blockIdx.x == 0 && tail < num_pairs) { // fewer than kGroup pairs
    see(src[tail], dst[tail]);
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const u32 om = __shfl_down(maxid, off, kWave);
    maxid = om > maxid ? om : maxid;
  }
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0 && maxid != 0) {
    atomicMax(&s_max, maxid);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_max != 0) {
    atomicMax(reinterpret_cast<unsigned long long *>(counters) + kMaxId,
              static_cast<unsigned long long>(s_max));
  }
  flush_counts<1>(cnt, counters);
}

// One pair: its two keys and whether it counts as bad id / bad weight /
// self-loop. A pair that is any of the three gets the dropped key twice.
struct PackRule {
  u32 n;
  u32 bits;
  u64 dropped; // n << bits

  template <typename IdT>
  __device__ inline void apply(
      IdT a, IdT b, bool weighted, i32 w, u64 &k_uv, u64 &k_vu, i32 &w_out, u32 (&cnt)[3]
  ) const {
    u32 u, v;
    bool ok = id_value(a, u) & id_value(b, v);
    ok = ok && u < n && v < n;
    const bool bad_w = weighted && w <= 0;
    const bool loop = ok && u == v;
    cnt[kBadIds] += ok ? 0u : 1u;
    cnt[kBadWeights] += bad_w ? 1u : 0u;
    cnt[kSelfLoops] += loop ? 1u : 0u;
    if (ok && !loop && !bad_w) {
      k_uv = (static_cast<u64>(u) << bits) | v;
      k_vu = (static_cast<u64>(v) << bits) | u;
      w_out = w;
    } else {
      k_uv = dropped;
      k_vu = dropped;
      w_out = 0;
    }
  }
};

// Lane t of a trip takes the kGroup consecutive pairs of group g: 16 bytes of
// src, dst and weights each (32 for 64-bit ids) in, 64 contiguous bytes of
// keys and 32 of values out, all as 16-byte accesses.
template <typename IdT, bool kVec, bool kWeighted>
__global__ __launch_bounds__(kThreads) void k_pack(
    const IdT *__restrict__ src, const IdT *__restrict__ dst, const i32 *__restrict__ weights,
    u64 num_pairs, PackRule rule, u64 *__restrict__ keys, i32 *__restrict__ vals,
    u64 *__restrict__ counters
) {
  u32 cnt[3] = {0, 0, 0};
  const u64 groups = num_pairs / kGroup;
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads;
  for (u64 g = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; g < groups; g += stride) {
    IdT a[kGroup], b[kGroup];
    i32 w[kGroup] = {1, 1, 1, 1};
    load_group<kVec>(src, g * kGroup, a);
    load_group<kVec>(dst, g * kGroup, b);
    if constexpr (kWeighted) {
      load_group<kVec>(weights, g * kGroup, w);
    }
    u64 k0[kGroup], k1[kGroup];
    i32 wo[kGroup];
#pragma unroll
    for (u32 j = 0; j < kGroup; ++j) {
      rule.apply(a[j], b[j], kWeighted, w[j], k0[j], k1[j], wo[j], cnt);
    }
    ulonglong2 *kout = reinterpret_cast<ulonglong2 *>(keys + 2 * kGroup * g);
#pragma unroll
    for (u32 j = 0; j < kGroup; ++j) {
      kout[j] = make_ulonglong2(k0[j], k1[j]);
    }
    if constexpr (kWeighted) {
      int4 *vout = reinterpret_cast<int4 *>(vals + 2 * kGroup * g);
      vout[0] = make_int4(wo[0], wo[0], wo[1], wo[1]);
      vout[1] = make_int4(wo[2], wo[2], wo[3], wo[3]);
    }
  }
  const u64 tail = groups * kGroup + threadIdx.x;
  if (blockIdx.x == 0 && tail < num_pairs) { // fewer than kGroup pairs
    u64 k0, k1;
    i32 wo;
    rule.apply(src[tail], dst[tail], kWeighted, kWeighted ? weights[tail] : 1, k0, k1, wo, cnt);
    keys[2 * tail] = k0;
    keys[2 * tail + 1] = k1;
    if constexpr (kWeighted) {
      vals[2 * tail] = wo;
      vals[2 * tail + 1] = wo;
    }
  }
  flush_counts<3>(cnt, counters);
}

__global__ __launch_bounds__(kThreads) void k_check_sums(
    const u32 *__restrict__ uvals, const u32 *__restrict__ d_count, u64 *__restrict__ counters
) {
  const u64 count = *d_count;
  u32 cnt[1] = {0};
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads;
  for (u64 i = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += stride) {
    cnt[0] += uvals[i] == kSumSaturated ? 1u : 0u;
  }
  flush_counts<1>(cnt, counters + kOverflow);
}

// Lane t of a trip takes the arcs 4g .. 4g + 3 and reads one key beyond them:
// an arc is the last of its row iff the next key has another row (or there is
// no next arc). Rows are below n, so xadj[row + 1] is in range.
template <bool kWeighted>
__global__ __launch_bounds__(kThreads) void k_build(
    const u64 *__restrict__ ukeys, const i32 *__restrict__ uvals, u32 m, u32 bits,
    u64 *__restrict__ xadj, u32 *__restrict__ adjncy, i32 *__restrict__ adjwgt
) {
  const u64 mask = (1ull << bits) - 1;
  const u64 groups = (static_cast<u64>(m) + kGroup - 1) / kGroup;
  const u64 stride = static_cast<u64>(gridDim.x) * kThreads;
  for (u64 g = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x; g < groups; g += stride) {
    const u64 base = g * kGroup;
    if (base + kGroup <= m) {
      u64 k[kGroup + 1];
      const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(ukeys + base);
      const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(ukeys + base + 2);
      k[0] = a.x;
      k[1] = a.y;
      k[2] = b.x;
      k[3] = b.y;
      k[4] = base + kGroup < m ? ukeys[base + kGroup] : ~0ull;
      *reinterpret_cast<uint4 *>(adjncy + base) =
          make_uint4(static_cast<u32>(k[0] & mask), static_cast<u32>(k[1] & mask),
                     static_cast<u32>(k[2] & mask), static_cast<u32>(k[3] & mask));
      if constexpr (kWeighted) {
        *reinterpret_cast<int4 *>(adjwgt + base) = *reinterpret_cast<const int4 *>(uvals + base);
      }
#pragma unroll
      for (u32 j = 0; j < kGroup; ++j) {
        const u64 row = k[j] >> bits;
        if ((k[j + 1] >> bits) != row) {
          xadj[row + 1] = base + j + 1;
        }
      }
    } else {
      for (u64 i = base; i < m; ++i) {
        const u64 key = ukeys[i];
        const u64 next = i + 1 < m ? ukeys[i + 1] : ~0ull;
        adjncy[i] = static_cast<u32>(key & mask);
        if constexpr (kWeighted) {
          adjwgt[i] = uvals[i];
        }
        const u64 row = key >> bits;
        if ((next >> bits) != row) {
          xadj[row + 1] = i + 1;
        }
      }
    }
  }
}

// min(a + b, kSumSaturated) with the addition in 64 bits: associative and
// commutative on [0, kSumSaturated], so the reduction's grouping cannot show.
struct SaturatedSum {
  __host__ __device__ inline u32 operator()(u32 a, u32 b) const {
    const u64 s = static_cast<u64>(a) + b;
    return s > kSumSaturated ? kSumSaturated : static_cast<u32>(s);
  }
};

template <typename IdT>
void launch_scan_ids(
    const void *src, const void *dst, u64 num_pairs, u64 *counters, hipStream_t stream
) {
  const dim3 grid(capped_grid(num_pairs, static_cast<u64>(kThreads) * kGroup));
  const IdT *s = static_cast<const IdT *>(src), *d = static_cast<const IdT *>(dst);
  if (aligned16(src) && aligned16(dst)) {
    hipLaunchKernelGGL((k_scan_ids<IdT, true>), grid, dim3(kThreads), 0, stream, s, d, num_pairs,
                       counters);
  } else {
    hipLaunchKernelGGL((k_scan_ids<IdT, false>), grid, dim3(kThreads), 0, stream, s, d, num_pairs,
                       counters);
  }
  EDGES_LAUNCH_CHECK();
}

template <typename IdT, bool kWeighted>
void launch_pack(
    const void *src, const void *dst, const i32 *weights, u64 num_pairs, const PackRule &rule,
    u64 *keys, i32 *vals, u64 *counters, hipStream_t stream
) {
  const dim3 grid(capped_grid(num_pairs, static_cast<u64>(kThreads) * kGroup));
  const IdT *s = static_cast<const IdT *>(src), *d = static_cast<const IdT *>(dst);
  if (aligned16(src) && aligned16(dst) && aligned16(weights)) {
    hipLaunchKernelGGL((k_pack<IdT, true, kWeighted>), grid, dim3(kThreads), 0, stream, s, d,
                       weights, num_pairs, rule, keys, vals, counters);
  } else {
    hipLaunchKernelGGL((k_pack<IdT, false, kWeighted>), grid, dim3(kThreads), 0, stream, s, d,
                       weights, num_pairs, rule, keys, vals, counters);
  }
  EDGES_LAUNCH_CHECK();
}

template <typename IdT>
void launch_pack_w(
    const void *src, const void *dst, const i32 *weights, u64 num_pairs, const PackRule &rule,
    u64 *keys, i32 *vals, u64 *counters, hipStream_t stream
) {
  if (weights != nullptr) {
    launch_pack<IdT, true>(src, dst, weights, num_pairs, rule, keys, vals, counters, stream);
  } else {
    launch_pack<IdT, false>(src, dst, weights, num_pairs, rule, keys, vals, counters, stream);
  }
}

} // namespace

void scan_ids(
    const void *src, const void *dst, IdKind kind, u64 num_pairs, u64 *counters,
    hipStream_t stream
) {
  if (num_pairs == 0) {
    return;
  }
  if (kind == kIdsI64) {
    launch_scan_ids<i64>(src, dst, num_pairs, counters, stream);
  } else if (kind == kIdsI32) {
    launch_scan_ids<i32>(src, dst, num_pairs, counters, stream);
  } else {
    launch_scan_ids<u32>(src, dst, num_pairs, counters, stream);
  }
}

void pack(
    const void *src, const void *dst, IdKind kind, const i32 *weights, u64 num_pairs, u32 n,
    u64 *keys, i32 *vals, u64 *counters, hipStream_t stream
) {
  if (num_pairs == 0) {
    return;
  }
  PackRule rule;
  rule.n = n;
  rule.bits = key_bits(n);
  rule.dropped = static_cast<u64>(n) << rule.bits;
  if (kind == kIdsI64) {
    launch_pack_w<i64>(src, dst, weights, num_pairs, rule, keys, vals, counters, stream);
  } else if (kind == kIdsI32) {
    launch_pack_w<i32>(src, dst, weights, num_pairs, rule, keys, vals, counters, stream);
  } else {
    launch_pack_w<u32>(src, dst, weights, num_pairs, rule, keys, vals, counters, stream);
  }
}

int sort(
    void *temp, size_t &temp_bytes, u64 *keys[2], i32 *vals[2], u64 count, u32 end_bit,
    hipStream_t stream
) {
  rocprim::double_buffer<u64> kb(keys[0], keys[1]);
  if (vals[0] != nullptr) {
    rocprim::double_buffer<i32> vb(vals[0], vals[1]);
    EDGES_HIP_CHECK(rocprim::radix_sort_pairs(temp, temp_bytes, kb, vb, count, 0, end_bit, stream));
    if ((kb.current() == keys[0]) != (vb.current() == vals[0])) {
      fprintf(stderr, "kaminpar_amd: edges: sorted keys and values ended in different buffers\n");
      abort();
    }
  } else {
    EDGES_HIP_CHECK(rocprim::radix_sort_keys(temp, temp_bytes, kb, count, 0, end_bit, stream));
  }
  return kb.current() == keys[0] ? 0 : 1;
}

void collapse(
    void *temp, size_t &temp_bytes, const u64 *keys, const i32 *vals, u64 count, bool sum,
    u64 *ukeys, i32 *uvals, u32 *d_count, hipStream_t stream
) {
  if (vals == nullptr) {
    EDGES_HIP_CHECK(rocprim::unique(
        temp, temp_bytes, keys, ukeys, d_count, count, rocprim::equal_to<u64>(), stream
    ));
  } else if (sum) {
    EDGES_HIP_CHECK(rocprim::reduce_by_key(
        temp, temp_bytes, keys, reinterpret_cast<const u32 *>(vals), count, ukeys,
        reinterpret_cast<u32 *>(uvals), d_count, SaturatedSum(), rocprim::equal_to<u64>(), stream
    ));
  } else {
    EDGES_HIP_CHECK(rocprim::reduce_by_key(
        temp, temp_bytes, keys, vals, count, ukeys, uvals, d_count, rocprim::maximum<i32>(),
        rocprim::equal_to<u64>(), stream
    ));
  }
}

void check_sums(const i32 *uvals, const u32 *d_count, u64 *counters, hipStream_t stream) {
  // the count is on the device: a capped grid strides over whatever it is
  hipLaunchKernelGGL(k_check_sums, dim3(kMaxGrid), dim3(kThreads), 0, stream,
                     reinterpret_cast<const u32 *>(uvals), d_count, counters);
  EDGES_LAUNCH_CHECK();
}

void build(
    void *temp, size_t &temp_bytes, const u64 *ukeys, const i32 *uvals, u32 m, u32 n, u64 *xadj,
    u32 *adjncy, i32 *adjwgt, hipStream_t stream
) {
  const size_t rows = static_cast<size_t>(n) + 1;
  if (temp == nullptr) {
    EDGES_HIP_CHECK(rocprim::inclusive_scan(
        nullptr, temp_bytes, xadj, xadj, rows, rocprim::maximum<u64>(), stream
    ));
    return;
  }
  EDGES_HIP_CHECK(hipMemsetAsync(xadj, 0, sizeof(u64) * rows, stream));
  if (m > 0) {
    const dim3 grid(capped_grid(m, static_cast<u64>(kThreads) * kGroup));
    if (uvals != nullptr) {
      hipLaunchKernelGGL(k_build<true>, grid, dim3(kThreads), 0, stream, ukeys, uvals, m,
                         key_bits(n), xadj, adjncy, adjwgt);
    } else {
      hipLaunchKernelGGL(k_build<false>, grid, dim3(kThreads), 0, stream, ukeys, uvals, m,
                         key_bits(n), xadj, adjncy, adjwgt);
    }
    EDGES_LAUNCH_CHECK();
  }
  EDGES_HIP_CHECK(rocprim::inclusive_scan(
      temp, temp_bytes, xadj, xadj, rows, rocprim::maximum<u64>(), stream
  ));
}

} // namespace kmp_edges
