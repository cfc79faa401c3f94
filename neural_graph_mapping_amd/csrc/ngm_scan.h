// Prefix sums over arrays in device memory, written once for the evaluation-side kernels (marching cubes, the surface sampler,
// the nearest-point grid, subdivision, the kNN grids): a wave scan by lane shifts, a workgroup scan on top of it (the waves'
// totals through LDS, added in wave order), one workgroup scanning an array in rounds, and the three-pass device-wide scan.
// Sums are formed in a fixed order, no atomics: integer results do not depend on it, fp64 results are reproducible.
// (The DPP segmented scans of the render kernels are ngm_device.h's.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

// inclusive scan over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
  return v;
}

// exclusive scan over a workgroup of THREADS threads, every one of which calls it; *total = the workgroup's sum, in every
// thread.  wave_totals: THREADS / 64 words of LDS, not to be written again before the workgroup's next barrier
template <typename T, int THREADS>
__device__ __forceinline__ T block_exclusive_scan(T v, T* wave_totals, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_inclusive_scan(v, lane);
  if (lane == 63) wave_totals[wave] = inc;
  __syncthreads();
  T off = inc - v, sum = T(0);
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) { const T t = wave_totals[w]; if (w < wave) off += t; sum += t; }
  *total = sum;
  return off;
}

// exclusive scan of arr[0 .. n) in place by ONE workgroup of 1024 threads, every one of which calls it: rounds of 1024
// consecutive elements, the sum of the rounds before carried in a register.  write_total: arr[n] = the total.  Threads that
// read elements other than their own afterwards put a __threadfence() and a barrier in between.
template <typename T>
__device__ __forceinline__ void workgroup_scan_inplace(T* arr, int64_t n, bool write_total) {
  __shared__ T wave_totals[16];
  T carry = T(0);
  for (int64_t b0 = 0; b0 < n; b0 += 1024) {
    const int64_t i = b0 + threadIdx.x;
    const T v = i < n ? arr[i] : T(0);
    T total;
    const T off = block_exclusive_scan<T, 1024>(v, wave_totals, &total);
    if (i < n) arr[i] = carry + off;
    carry += total;
    __syncthreads();                                       // wave_totals is rewritten by the next round
  }
  if (write_total && threadIdx.x == 0) arr[n] = carry;
}

// ---- device-wide scan, in place ---------------------------------------------------------------------------------------
// Three passes over chunks of SCAN_CHUNK<PER> elements, one workgroup of SCAN_T threads per chunk: (1) k_scan_reduce, the
// chunks' sums; (2) k_scan_chunks, ONE workgroup scans those sums; (3) k_scan_apply, PER contiguous elements per thread:
// thread-local scan, workgroup scan of the threads' sums, + the chunk's offset, written back over the input.  Every element
// is read twice and written once.  The length is *n_dev where the host only knows its bound n_max (a grid's cell count): the
// launch covers n_max, chunks past the length do nothing.  An exclusive scan also leaves a[n] = total (a[0] = 0 for n == 0),
// so `a` has n + 1 elements.  `a` is 256-byte aligned (WsArena::take) and a chunk starts at a multiple of 256 * PER elements:
// a chunk that lies inside the length moves as 16-byte vectors, the last one as guarded scalars.  The kernels are static: every
// translation unit that includes this launches its own instances.
constexpr int SCAN_T = 256;
template <int PER> constexpr int SCAN_CHUNK = SCAN_T * PER;
template <typename T> struct alignas(16) ScanVec { T e[16 / sizeof(T)]; };

__device__ __forceinline__ int64_t scan_length(const int* n_dev, int64_t n_max) { return n_dev ? (int64_t)*n_dev : n_max; }

// the thread's j'th vector of the chunk at `base`.  STRIPED: consecutive threads take consecutive vectors, a wave reads 1 KB
// at once (the sums, whose order is free); otherwise a thread's vectors are consecutive (the scan)
template <typename T, int PER, bool STRIPED>
__device__ __forceinline__ int64_t scan_vec_index(int64_t base, int j) {
  constexpr int W = 16 / sizeof(T);
  return base + (STRIPED ? (int64_t)j * SCAN_T + threadIdx.x : (int64_t)threadIdx.x * (PER / W) + j) * W;
}
template <typename T, int PER, bool STRIPED>
__device__ __forceinline__ void scan_load(const T* a, int64_t base, int64_t n, T (&v)[PER]) {
  constexpr int W = 16 / sizeof(T);
  static_assert(PER % W == 0, "whole 16-byte vectors per thread");
  const bool full = base + SCAN_CHUNK<PER> <= n;
#pragma unroll
  for (int j = 0; j < PER / W; ++j) {
    const int64_t i = scan_vec_index<T, PER, STRIPED>(base, j);
    if (full) {
      const ScanVec<T> x = *reinterpret_cast<const ScanVec<T>*>(a + i);
#pragma unroll
      for (int k = 0; k < W; ++k) v[j * W + k] = x.e[k];
    } else {
#pragma unroll
      for (int k = 0; k < W; ++k) v[j * W + k] = (i + k < n) ? a[i + k] : T(0);
    }
  }
}
template <typename T, int PER>
__device__ __forceinline__ void scan_store(T* a, int64_t base, int64_t n, const T (&v)[PER]) {
  constexpr int W = 16 / sizeof(T);
  const bool full = base + SCAN_CHUNK<PER> <= n;
#pragma unroll
  for (int j = 0; j < PER / W; ++j) {
    const int64_t i = scan_vec_index<T, PER, false>(base, j);
    if (full) {
      ScanVec<T> x;
#pragma unroll
      for (int k = 0; k < W; ++k) x.e[k] = v[j * W + k];
      *reinterpret_cast<ScanVec<T>*>(a + i) = x;
    } else {
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (i + k < n) a[i + k] = v[j * W + k];
    }
  }
}

template <typename T, int PER>
static __global__ __launch_bounds__(SCAN_T) void k_scan_reduce(const T* __restrict__ a, const int* __restrict__ n_dev,
                                                               int64_t n_max, T* __restrict__ partial) {
  __shared__ T wave_totals[SCAN_T / 64];
  const int64_t n = scan_length(n_dev, n_max), base = (int64_t)blockIdx.x * SCAN_CHUNK<PER>;
  if (base >= n) return;
  T v[PER];
  scan_load<T, PER, true>(a, base, n, v);
  T s = T(0);
#pragma unroll
  for (int i = 0; i < PER; ++i) s += v[i];
  T total;
  (void)block_exclusive_scan<T, SCAN_T>(s, wave_totals, &total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

template <typename T>
static __global__ __launch_bounds__(1024) void k_scan_chunks(T* partial, const int* n_dev, int64_t n_max, int chunk) {
  workgroup_scan_inplace(partial, (scan_length(n_dev, n_max) + chunk - 1) / chunk, false);
}

template <typename T, int PER, bool INCLUSIVE>
static __global__ __launch_bounds__(SCAN_T) void k_scan_apply(T* __restrict__ a, const int* __restrict__ n_dev, int64_t n_max,
                                                              const T* __restrict__ partial) {
  __shared__ T wave_totals[SCAN_T / 64];
  const int64_t n = scan_length(n_dev, n_max), base = (int64_t)blockIdx.x * SCAN_CHUNK<PER>;
  if (base >= n) {
    if (!INCLUSIVE && n == 0 && blockIdx.x == 0 && threadIdx.x == 0) a[0] = T(0);
    return;
  }
  T v[PER];
  scan_load<T, PER, false>(a, base, n, v);
  T s = T(0);
#pragma unroll
  for (int i = 0; i < PER; ++i) s += v[i];
  T total;
  T run = partial[blockIdx.x] + block_exclusive_scan<T, SCAN_T>(s, wave_totals, &total);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const T x = v[i];
    if (INCLUSIVE) { run += x; v[i] = run; }
    else { v[i] = run; run += x; }
  }
  scan_store<T, PER>(a, base, n, v);
  // the thread that holds element n - 1 (zeros behind it): its running sum is the total
  const int64_t i0 = base + (int64_t)threadIdx.x * PER;
  if (!INCLUSIVE && i0 < n && n <= i0 + PER) a[n] = run;
}

// chunk sums a scan of up to n_max elements needs (`partial`)
template <int PER>
static inline int64_t scan_partial_count(int64_t n_max) {
  return std::max<int64_t>((n_max + SCAN_CHUNK<PER> - 1) / SCAN_CHUNK<PER>, 1);
}
template <typename T, int PER, bool INCLUSIVE>
static void launch_scan(T* a, const int* n_dev, int64_t n_max, T* partial, hipStream_t st) {
  const dim3 nb((unsigned)scan_partial_count<PER>(n_max));
  hipLaunchKernelGGL((k_scan_reduce<T, PER>), nb, dim3(SCAN_T), 0, st, a, n_dev, n_max, partial);
  hipLaunchKernelGGL(k_scan_chunks<T>, dim3(1), dim3(1024), 0, st, partial, n_dev, n_max, SCAN_CHUNK<PER>);
  hipLaunchKernelGGL((k_scan_apply<T, PER, INCLUSIVE>), nb, dim3(SCAN_T), 0, st, a, n_dev, n_max, partial);
}
