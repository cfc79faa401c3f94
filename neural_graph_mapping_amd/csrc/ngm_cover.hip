// Cover a keyframe's depth with new fields (ngm_cover_depth; the contract is the comment above it in include/ngm_hip.h):
// NeuralGraphMap._extend_global_map_dict (run_mapping.py:265-345) up to the positions of the new fields, in fp32, in the
// reference's order of operations.  The host clears the workspace's tables and counters (one memset), then five launches:
//   k_cover_bin     one thread per active field: its row goes into `bins`, an open-addressing table of row numbers probed from
//                   the hash of the field's cell (the cell of THIS call: edge `cell`, shifted by `shift`).  Fields of one cell,
//                   and fields whose hashes collide, sit in one unbroken run.
//   k_cover_pixels  one thread per pixel: back-project, transform, cell.  Covered iff a field centre lies within r: r < cell, so
//                   such a centre is in one of the 27 cells around the pixel's (while |index| < 2^16; beyond, where fp32 cell
//                   coordinates get coarse, every active field is tried), and each of those cells' runs in `bins` is walked with
//                   the exact test -- a hash collision only adds a candidate that fails it.  The key of an uncovered pixel is
//                   deduplicated in the wave (neighbouring pixels share a cell), then in a 512-slot LDS set per workgroup; only
//                   the thread that put a key into the LDS set inserts it into the global set `cells` (64-bit compare-and-swap).
//                   Pixel counts: one ballot per wave, one atomic per workgroup.
//   k_cover_occupy  one thread per active field: if its cell is in `cells`, bit 63 of that slot is set (occupied).
//   k_cover_compact one thread per slot of `cells`: keys without bit 63 are counted and, while they fit, appended to `list`
//                   (wave-aggregated: one atomic per wave).  The order of `list` depends on scheduling; nothing else does.
//   k_cover_emit    status and counts; with status 0 one thread per listed key counts the keys below its own -- its rank, the
//                   keys are distinct -- and writes the cell centre at that row: ascending (i, j, k), bitwise repeatable.
// Integer atomics only; `any`, set union and rank are independent of arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ngm_hip.h"
#include "ngm_workspace.h"

#pragma clang fp contract(off)

#define CV_T 256                          // threads per workgroup (4 waves)
#define CV_LDS_SLOTS 512                  // per-workgroup set: at most CV_T distinct keys, load <= 1/2
#define CV_BIAS 1048576                   // 2^20: indices in (-2^20, 2^20) pack into 21 bits each, never 0
#define CV_NEAR 65536.0f                  // |cell coordinate| below which the 27-cell search is exact (see cover_covered)
#define CV_OCCUPIED 0x8000000000000000ull
#define CV_CTR 8                          // counters: survivors, range flag, uncovered valid pixels, valid pixels, global insertions

typedef unsigned long long u64;

struct CoverWs {
  u64* cells;                             // [slots] 0 = empty, else key | CV_OCCUPIED
  uint32_t* bins;                         // [bin_slots] 0 = empty, else row + 1
  u64* list;                              // [max_new] surviving keys, unordered
  int32_t* ctr;                           // [CV_CTR]
  int64_t slots, bin_slots;
};

__device__ __forceinline__ bool cv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ u64 cv_mix(u64 k) {                               // murmur3's 64-bit finaliser
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}
__device__ __forceinline__ u64 cv_pack(int i, int j, int k) {
  return ((u64)(uint32_t)(i + CV_BIAS) << 42) | ((u64)(uint32_t)(j + CV_BIAS) << 21) | (u64)(uint32_t)(k + CV_BIAS);
}
__device__ __forceinline__ bool cv_in_range(float f) { return f > -(float)CV_BIAS && f < (float)CV_BIAS; }   // false for NaN

// floor((v + shift) / cell) per axis, as floats
__device__ __forceinline__ void cv_cell(const float p[3], const float sh[3], float cell, float f[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) f[a] = floorf((p[a] + sh[a]) / cell);
}

// row of active field a, or -1 where the entry is skipped
__device__ __forceinline__ int cv_row(const ngm_cover_depth_args& a, int n) {
  if (!a.field_ids) return n;
  const int64_t id = a.field_ids[n];
  return (id < 0 || id >= (int64_t)a.rows) ? -1 : (int)id;
}

__device__ __forceinline__ bool cv_within(const float* __restrict__ pos, int row, const float p[3], float r2) {
  const float dx = p[0] - pos[3 * (int64_t)row], dy = p[1] - pos[3 * (int64_t)row + 1], dz = p[2] - pos[3 * (int64_t)row + 2];
  return dx * dx + dy * dy + dz * dz < r2;                                    // NaN: not covered
}

__global__ __launch_bounds__(CV_T) void k_cover_bin(ngm_cover_depth_args a, CoverWs w) {
  const int n = blockIdx.x * CV_T + threadIdx.x;
  if (n >= a.num_active) return;
  const int row = cv_row(a, n);
  if (row < 0) return;
  const float sh[3] = {a.shift[0], a.shift[1], a.shift[2]};
  const float c[3] = {a.field_positions[3 * (int64_t)row], a.field_positions[3 * (int64_t)row + 1], a.field_positions[3 * (int64_t)row + 2]};
  float f[3];
  cv_cell(c, sh, a.cell, f);
  if (!(cv_in_range(f[0]) && cv_in_range(f[1]) && cv_in_range(f[2]))) return;   // no pixel searched by cell can be within r of it
  const u64 mask = (u64)w.bin_slots - 1;
  u64 h = cv_mix(cv_pack((int)f[0], (int)f[1], (int)f[2])) & mask;
  for (int64_t t = 0; t < w.bin_slots; ++t) {                                 // bin_slots >= 4 num_active: an empty slot exists
    if (atomicCAS(&w.bins[h], 0u, (uint32_t)row + 1u) == 0u) break;
    h = (h + 1) & mask;
  }
}

// Some active centre within r of p?  A centre within r has |u_p - u_c| <= r / cell = 0.866 per axis in exact arithmetic; the
// computed cell coordinates carry two roundings each (the add, the divide), at most 2^-7 below |u| = 2^16, so the computed
// ones differ by less than 1 and their floors by at most 1.  Beyond that bound every active field is tried.
__device__ bool cover_covered(const ngm_cover_depth_args& a, const CoverWs& w, const float p[3], const float f[3], float r2) {
  const float* __restrict__ pos = a.field_positions;
  if (fabsf(f[0]) < CV_NEAR && fabsf(f[1]) < CV_NEAR && fabsf(f[2]) < CV_NEAR) {
    const int ci = (int)f[0], cj = (int)f[1], ck = (int)f[2];
    const u64 mask = (u64)w.bin_slots - 1;
    for (int d = 0; d < 27; ++d) {
      u64 h = cv_mix(cv_pack(ci + d / 9 - 1, cj + (d / 3) % 3 - 1, ck + d % 3 - 1)) & mask;
      for (int64_t t = 0; t < w.bin_slots; ++t) {
        const uint32_t e = w.bins[h];
        if (e == 0u) break;
        if (cv_within(pos, (int)(e - 1u), p, r2)) return true;
        h = (h + 1) & mask;
      }
    }
    return false;
  }
  for (int n = 0; n < a.num_active; ++n) {
    const int row = cv_row(a, n);
    if (row >= 0 && cv_within(pos, row, p, r2)) return true;
  }
  return false;
}

__global__ __launch_bounds__(CV_T) void k_cover_pixels(ngm_cover_depth_args a, CoverWs w) {
  __shared__ u64 lset[CV_LDS_SLOTS];
  __shared__ int lcnt[4];                                                    // valid, uncovered valid, global insertions, range flag
  for (int i = threadIdx.x; i < CV_LDS_SLOTS; i += CV_T) lset[i] = 0ull;
  if (threadIdx.x < 4) lcnt[threadIdx.x] = 0;
  __syncthreads();

  const int64_t hw = (int64_t)a.height * a.width;
  const int64_t pix = (int64_t)blockIdx.x * CV_T + threadIdx.x;
  bool valid = false, want = false, out_of_range = false;
  u64 key = 0ull;
  if (pix < hw) {
    const float d = a.depth[pix * a.pixel_stride];
    if (cv_finite(d) && d != 0.0f) {
      const int i = (int)(pix / a.width), j = (int)(pix % a.width);
      const float x = ((float)j - a.cx) * d / a.fx;
      const float y = -((float)i - a.cy) * d / a.fy;
      const float z = -d;
      const float* __restrict__ T = a.c2w;
      float p[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) p[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
      if (cv_finite(p[0]) && cv_finite(p[1]) && cv_finite(p[2])) {
        valid = true;
        const float sh[3] = {a.shift[0], a.shift[1], a.shift[2]};
        float f[3];
        cv_cell(p, sh, a.cell, f);
        const bool covered = a.num_active > 0 && cover_covered(a, w, p, f, a.radius * a.radius);
        if (!covered) {
          want = true;
          if (cv_in_range(f[0]) && cv_in_range(f[1]) && cv_in_range(f[2])) key = cv_pack((int)f[0], (int)f[1], (int)f[2]);
          else out_of_range = true;
        }
      }
    }
  }

  const int lane = threadIdx.x & 63;
  const u64 bv = __ballot(valid), bw = __ballot(want), bo = __ballot(out_of_range);
  if (lane == 0) {
    if (bv) atomicAdd(&lcnt[0], __popcll(bv));
    if (bw) atomicAdd(&lcnt[1], __popcll(bw));
    if (bo) atomicOr(&lcnt[3], 1);
  }

  // one lane per distinct key of the wave goes on
  bool pending = want && !out_of_range, leader = false;
  for (int it = 0; it < 64; ++it) {
    const u64 b = __ballot(pending);
    if (b == 0ull) break;
    const int first = __ffsll((long long)b) - 1;
    const uint32_t lo = __shfl((uint32_t)key, first, 64), hi = __shfl((uint32_t)(key >> 32), first, 64);
    if (pending && key == (((u64)hi << 32) | lo)) {
      pending = false;
      leader = lane == first;
    }
  }
  // one thread per distinct key of the workgroup goes on: the one whose compare-and-swap found the LDS slot empty
  if (leader) {
    bool fresh = false;
    uint32_t h = (uint32_t)cv_mix(key) & (CV_LDS_SLOTS - 1);
    for (int t = 0; t < CV_LDS_SLOTS; ++t) {
      const u64 old = atomicCAS(&lset[h], 0ull, key);
      if (old == 0ull) { fresh = true; break; }
      if (old == key) break;
      h = (h + 1) & (CV_LDS_SLOTS - 1);
    }
    if (fresh) {
      atomicAdd(&lcnt[2], 1);
      const u64 mask = (u64)w.slots - 1;
      u64 g = cv_mix(key) & mask;
      for (int64_t t = 0; t < w.slots; ++t) {                                 // slots >= 2 H W: an empty slot exists
        const u64 old = atomicCAS(&w.cells[g], 0ull, key);
        if (old == 0ull || old == key) break;
        g = (g + 1) & mask;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (lcnt[0]) atomicAdd(&w.ctr[3], lcnt[0]);
    if (lcnt[1]) atomicAdd(&w.ctr[2], lcnt[1]);
    if (lcnt[2]) atomicAdd(&w.ctr[4], lcnt[2]);
    if (lcnt[3]) atomicOr(&w.ctr[1], 1);
  }
}

__global__ __launch_bounds__(CV_T) void k_cover_occupy(ngm_cover_depth_args a, CoverWs w) {
  const int n = blockIdx.x * CV_T + threadIdx.x;
  if (n >= a.num_active) return;
  const int row = cv_row(a, n);
  if (row < 0) return;
  const float sh[3] = {a.shift[0], a.shift[1], a.shift[2]};
  const float c[3] = {a.field_positions[3 * (int64_t)row], a.field_positions[3 * (int64_t)row + 1], a.field_positions[3 * (int64_t)row + 2]};
  float f[3];
  cv_cell(c, sh, a.cell, f);
  if (!(cv_in_range(f[0]) && cv_in_range(f[1]) && cv_in_range(f[2]))) return;   // no wanted cell has such an index
  const u64 key = cv_pack((int)f[0], (int)f[1], (int)f[2]);
  const u64 mask = (u64)w.slots - 1;
  u64 g = cv_mix(key) & mask;
  for (int64_t t = 0; t < w.slots; ++t) {
    const u64 v = w.cells[g];                                                 // keys no longer change: k_cover_pixels is complete
    if (v == 0ull) break;
    if ((v & ~CV_OCCUPIED) == key) { atomicOr(&w.cells[g], CV_OCCUPIED); break; }
    g = (g + 1) & mask;
  }
}

__global__ __launch_bounds__(CV_T) void k_cover_compact(ngm_cover_depth_args a, CoverWs w) {
  const int64_t s = (int64_t)blockIdx.x * CV_T + threadIdx.x;
  const u64 v = s < w.slots ? w.cells[s] : 0ull;
  const bool keep = v != 0ull && !(v & CV_OCCUPIED);
  const u64 b = __ballot(keep);
  if (b == 0ull) return;
  const int lane = threadIdx.x & 63, first = __ffsll((long long)b) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(&w.ctr[0], __popcll(b));
  base = __shfl(base, first, 64);
  const int at = base + __popcll(b & ((1ull << lane) - 1ull));
  if (keep && at < a.max_new) w.list[at] = v;
}

__global__ __launch_bounds__(CV_T) void k_cover_emit(ngm_cover_depth_args a, CoverWs w) {
  __shared__ u64 tile[CV_T];
  const int n = w.ctr[0];
  const int status = w.ctr[1] ? 2 : (n > a.max_new ? 1 : 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.counts[0] = status == 2 ? 0 : n;
    a.counts[1] = status;
    a.counts[2] = w.ctr[2];
    a.counts[3] = w.ctr[3];
  }
  if (status != 0 || (int64_t)blockIdx.x * CV_T >= n) return;                 // uniform over the workgroup
  const int me = blockIdx.x * CV_T + threadIdx.x;
  const u64 key = me < n ? w.list[me] : 0ull;
  int rank = 0;
  for (int base = 0; base < n; base += CV_T) {
    __syncthreads();
    tile[threadIdx.x] = base + (int)threadIdx.x < n ? w.list[base + threadIdx.x] : ~0ull;
    __syncthreads();
    const int m = n - base < CV_T ? n - base : CV_T;
    for (int t = 0; t < m; ++t) rank += tile[t] < key ? 1 : 0;
  }
  if (me >= n) return;
  const float ijk[3] = {(float)((int)(key >> 42) - CV_BIAS), (float)((int)((key >> 21) & 0x1fffffu) - CV_BIAS),
                        (float)((int)(key & 0x1fffffu) - CV_BIAS)};
#pragma unroll
  for (int c = 0; c < 3; ++c) a.new_positions[3 * (int64_t)rank + c] = ((ijk[c] - a.shift[c]) + 0.5f) * a.cell;
}

// ------------------------------------------------------------------------------------------------ host
static int64_t cv_pow2_at_least(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
static void cover_layout(CoverWs& w, int64_t hw, int num_active, int max_new, WsArena& ws) {
  w.slots = cv_pow2_at_least(2 * hw < CV_T ? CV_T : 2 * hw);            // a multiple of CV_T: k_cover_compact's grid
  w.bin_slots = cv_pow2_at_least(4 * (int64_t)num_active < 64 ? 64 : 4 * (int64_t)num_active);
  w.cells = ws.take<u64>(w.slots);
  w.bins = ws.take<uint32_t>(w.bin_slots);
  w.ctr = ws.take<int32_t>(CV_CTR);
  w.list = ws.take<u64>(max_new);
}
int64_t ngm_cover_bytes(int H, int W, int num_active, int max_new) {
  CoverWs w = {};
  WsArena ws;
  cover_layout(w, (int64_t)H * W, num_active, max_new, ws);
  return ws.bytes();
}
// the first word of the counter region, for measurements: [4] = insertions into the global set of the last call
const int32_t* ngm_cover_counters(int H, int W, int num_active, int max_new, void* workspace) {
  CoverWs w = {};
  WsArena ws(workspace);
  cover_layout(w, (int64_t)H * W, num_active, max_new, ws);
  return w.ctr;
}
int ngm_launch_cover(const ngm_cover_depth_args& a, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  CoverWs w = {};
  WsArena ws(workspace);
  const int64_t hw = (int64_t)a.height * a.width;
  cover_layout(w, hw, a.num_active, a.max_new, ws);
  if (!ws.covers(workspace_bytes)) return 1;
  // cells, bins and the counters are adjacent regions of the walk: one clear
  hipMemsetAsync(w.cells, 0, (size_t)((char*)(w.ctr + CV_CTR) - (char*)w.cells), st);
  const unsigned field_blocks = (unsigned)((a.num_active + CV_T - 1) / CV_T);
  if (a.num_active > 0) hipLaunchKernelGGL(k_cover_bin, dim3(field_blocks), dim3(CV_T), 0, st, a, w);
  if (hw > 0) hipLaunchKernelGGL(k_cover_pixels, dim3((unsigned)((hw + CV_T - 1) / CV_T)), dim3(CV_T), 0, st, a, w);
  if (a.num_active > 0 && hw > 0) hipLaunchKernelGGL(k_cover_occupy, dim3(field_blocks), dim3(CV_T), 0, st, a, w);
  if (hw > 0) hipLaunchKernelGGL(k_cover_compact, dim3((unsigned)(w.slots / CV_T)), dim3(CV_T), 0, st, a, w);
  hipLaunchKernelGGL(k_cover_emit, dim3((unsigned)((a.max_new + CV_T - 1) / CV_T)), dim3(CV_T), 0, st, a, w);
  return 0;
}
