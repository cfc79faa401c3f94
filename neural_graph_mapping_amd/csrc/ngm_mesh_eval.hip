// Scoring a mesh on the device: the two device parts of evaluation._evaluate_postprocessed_meshes (evaluation.py:163-208).
//   surface sampler (evaluation.py:190-191, trimesh.sample.sample_surface restated from its public definition: a face with
//   probability proportional to its area, then a uniform point in it)
//     k_face_area       : fp32 triangle area per face, stored as fp64; 0 for a face with a non-finite vertex or an index
//                         outside [0, V)
//     k_scan_*          : inclusive fp64 scan over the faces, the three passes of ngm_scan.h (chunk sums, one workgroup over the
//                         chunk sums with a carry, chunks again): GT meshes have millions of faces
//     k_surface_sample  : one thread per sample: Philox block `sample index` of stream MESH_STREAM_SURFACE, words 0 and 1 a
//                         53-bit uniform that picks the face by binary search in the scan, words 2 and 3 the point in it
//   exact nearest point between two clouds (evaluation.py:75-130: scipy.spatial.KDTree build + query)
//     k_np_bbox / k_np_header : bounding box of the finite references -> uniform grid of cubic cells, a few points per occupied
//                         cell, no more than max_cells of them; the header stays in device memory (NpGridHdr, like KnnGridHdr)
//     k_np_clear / k_np_count / k_scan_* / k_np_fill : count -> exclusive scan -> cell-sorted float4 copy (x, y, z, index)
//     k_np_query        : one thread per query: Chebyshev rings around the query's (clamped) cell until the best distance found
//                         is within the gap to every face of the visited block that still has cells behind it
//   subdivision to a maximum edge length (mesh_culling.py:260-261: trimesh's subdivide_to_size), at the end of the file
//     k_sub_level / k_scan_* / k_sub_totals : level, children and new vertices per face, two exclusive int64 scans, three totals
//     k_sub_copy / k_sub_verts / k_sub_faces : one thread per output element, its parent by binary search in the scans
// No size is read back to the host; nothing here returns a status from the device.  Plain C++ and vector stores only; every
// index that reaches memory is checked (face indices against V) or clamped (cell indices).
#include "ngm_device.h"
#include "ngm_launch.h"
#include "ngm_scan.h"
#include "ngm_workspace.h"

#include <algorithm>

#pragma clang fp contract(off)

constexpr uint32_t MESH_STREAM_SURFACE = 0x54470006u;      // next to the TSMV_STREAM_* ids of ngm_target.hip

__device__ __forceinline__ bool me_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the device-wide scans of ngm_scan.h, 2048-element chunks: fp64 areas (inclusive), int cell counts, int64 child counts
constexpr int ME_SCAN_PER = 8;

// ---- surface sampler --------------------------------------------------------------------------------------------------
struct SurfArgs {
  const float* verts; const int64_t* faces;
  int64_t V; int F; int N;
  uint64_t seed;
  double* cum;          // (F) areas, then their inclusive scan
  float* points; int64_t* face_ids;
};

// the three corners of face f; false when an index is outside [0, V) or a coordinate is not finite
__device__ __forceinline__ bool surf_face(const SurfArgs& a, int f, float (&p)[3][3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t i = a.faces[3 * (int64_t)f + k];
    if (i < 0 || i >= a.V) { ok = false; p[k][0] = p[k][1] = p[k][2] = 0.f; continue; }
#pragma unroll
    for (int d = 0; d < 3; ++d) { p[k][d] = a.verts[3 * i + d]; ok = ok && me_finite(p[k][d]); }
  }
  return ok;
}
// fp32: 0.5 |(v1 - v0) x (v2 - v0)|, every product and sum rounded on its own (tests/_mesh_metrics_host.py restates it)
__device__ __forceinline__ float surf_area(const float (&p)[3][3]) {
  const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
  const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const float ar = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
  return me_finite(ar) ? ar : 0.f;
}

__global__ __launch_bounds__(256) void k_face_area(SurfArgs a) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.F) return;
  float p[3][3];
  a.cum[f] = surf_face(a, f, p) ? (double)surf_area(p) : 0.0;
}

__global__ __launch_bounds__(256) void k_surface_sample(SurfArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  const float qnan = __int_as_float(0x7fc00000);
  float out[3] = {qnan, qnan, qnan};
  int64_t fid = -1;
  const double total = a.cum[a.F - 1];
  if (total > 0.0 && total < (double)INFINITY) {
    uint32_t q[4];
    philox_block(a.seed, 0ull, (uint64_t)i, MESH_STREAM_SURFACE, q);
    // 53 bits: a 24-bit draw would quantise a mesh of millions of faces
    const double u53 = (double)(((uint64_t)(q[0] >> 5) << 26) | (uint64_t)(q[1] >> 6)) * (1.0 / 9007199254740992.0);
    const double target = u53 * total;
    int lo = 0, hi = a.F;                                   // first k with cum[k] > target (F: none)
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (a.cum[mid] > target) hi = mid; else lo = mid + 1; }
    int k = min(lo, a.F - 1);
    // cum[k - 1] <= target < cum[k] makes face k one of positive area.  A parallel fp64 scan may be off by an ulp between
    // neighbouring elements, and u53 * total may round up to total: where the face found has no area after all, the next
    // one that has (forwards, then backwards) is the face the draw belongs to
    float p[3][3];
    bool ok = surf_face(a, k, p) && surf_area(p) > 0.f;
    for (int j = k + 1; !ok && j < a.F; ++j) { ok = surf_face(a, j, p) && surf_area(p) > 0.f; if (ok) k = j; }
    for (int j = k - 1; !ok && j >= 0; --j) { ok = surf_face(a, j, p) && surf_area(p) > 0.f; if (ok) k = j; }
    if (ok) {
      float u = philox_word_uniform(q[2]), v = philox_word_uniform(q[3]);
      if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
#pragma unroll
      for (int d = 0; d < 3; ++d) out[d] = (p[0][d] + u * (p[1][d] - p[0][d])) + v * (p[2][d] - p[0][d]);
      fid = k;
    }
  }
  a.points[3 * (int64_t)i] = out[0]; a.points[3 * (int64_t)i + 1] = out[1]; a.points[3 * (int64_t)i + 2] = out[2];
  a.face_ids[i] = fid;
}

// workspace: the areas / their scan, the scan's chunk sums
static void surf_layout(int64_t F, double** cum, double** partial, WsArena& ws) {
  *cum = ws.take<double>(F);
  *partial = ws.take<double>(scan_partial_count<ME_SCAN_PER>(F) + 1);
}
int64_t ngm_surface_sample_bytes(int64_t num_faces) {
  double *cum, *partial;
  return ws_bytes(surf_layout, num_faces, &cum, &partial);
}
int ngm_launch_surface_sample(const float* verts, int64_t V, const int64_t* faces, int64_t F, int64_t N, uint64_t seed, float* points,
                              int64_t* face_ids, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  SurfArgs a = {};
  a.verts = verts; a.faces = faces; a.V = V; a.F = (int)F; a.N = (int)N; a.seed = seed; a.points = points; a.face_ids = face_ids;
  double* partial;
  WsArena ws(workspace);
  surf_layout(F, &a.cum, &partial, ws);
  if (!ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_face_area, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, a);
  launch_scan<double, ME_SCAN_PER, true>(a.cum, nullptr, F, partial, st);
  hipLaunchKernelGGL(k_surface_sample, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a);
  return 0;
}

// ---- exact nearest point ----------------------------------------------------------------------------------------------
struct NpGridHdr { float x0, y0, z0, c, inv_c; int nx, ny, nz, ncells, valid, nmax, pad; };
constexpr int NP_BBOX_BLOCKS = 1024;
struct NpArgs {
  const float* refs; const float* queries;
  int M, N;
  float* dist; int64_t* index;
  NpGridHdr* hdr;
  float* part;          // (NP_BBOX_BLOCKS, 6) per-workgroup bounding boxes
  int* cell_start;      // (max_cells + 1) counts, then their exclusive prefix
  int* cell_fill;       // (max_cells) fill cursors
  int* scan_part;       // chunk sums of the scan
  float4* sorted;       // (M) finite references grouped by cell: (x, y, z, original index as int bits)
  int max_cells, bbox_blocks;
};

__global__ __launch_bounds__(256) void k_np_bbox(NpArgs a) {
  __shared__ float red[6][256];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.M; i += (int64_t)gridDim.x * 256) {
    const float x = a.refs[3 * i], y = a.refs[3 * i + 1], z = a.refs[3 * i + 2];
    if (!(me_finite(x) && me_finite(y) && me_finite(z))) continue;           // a non-finite reference is nobody's neighbour
    lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
    lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
    lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
  }
  const int t = threadIdx.x;
#pragma unroll
  for (int d = 0; d < 3; ++d) { red[d][t] = lo[d]; red[3 + d][t] = hi[d]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int d = 0; d < 3; ++d) { red[d][t] = fminf(red[d][t], red[d][t + s]); red[3 + d][t] = fmaxf(red[3 + d][t], red[3 + d][t + s]); }
    __syncthreads();
  }
  if (t < 6) a.part[6 * blockIdx.x + t] = red[t][0];
}

// One workgroup: the boxes of k_np_bbox -> the grid.  Cubic cells sized for a few points per OCCUPIED cell: 2 M cells over
// the box's volume when it has three extents (the clouds are samples of surfaces: a cell the surface crosses then holds
// about half a dozen), M / 4 over its area / length when it has two / one; coarsened by 2^(1/3) per step until the
// grid fits max_cells.  A box the arithmetic cannot grid (an extent that overflows fp32) becomes one cell: brute force.
__global__ __launch_bounds__(256) void k_np_header(NpArgs a) {
  __shared__ float red[6][256];
  const int t = threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = t; b < a.bbox_blocks; b += 256)
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], a.part[6 * b + d]); hi[d] = fmaxf(hi[d], a.part[6 * b + 3 + d]); }
#pragma unroll
  for (int d = 0; d < 3; ++d) { red[d][t] = lo[d]; red[3 + d][t] = hi[d]; }
  __syncthreads();
  if (t != 0) return;
  float L[3], U[3], ext[3];
  bool valid = true, gridable = true;
  for (int d = 0; d < 3; ++d) {
    L[d] = red[d][0]; U[d] = red[3 + d][0];
    for (int j = 1; j < 256; ++j) { L[d] = fminf(L[d], red[d][j]); U[d] = fmaxf(U[d], red[3 + d][j]); }
    valid = valid && (L[d] <= U[d]);
  }
  NpGridHdr h = {};
  h.nx = h.ny = h.nz = 1; h.ncells = 1; h.nmax = 1; h.c = 1.f; h.inv_c = 0.f;
  if (valid) {
    int k = 0;
    double vol = 1.0;
    for (int d = 0; d < 3; ++d) {
      ext[d] = U[d] - L[d];
      if (!me_finite(ext[d])) gridable = false;
      if (ext[d] > 0.f) { ++k; vol *= (double)ext[d]; }
    }
    h.x0 = L[0]; h.y0 = L[1]; h.z0 = L[2];
    if (gridable && k > 0) {
      double want = (k == 3) ? 2.0 * (double)a.M : fmax(0.25 * (double)a.M, 1.0);
      want = fmin(want, (double)a.max_cells);
      float c = (float)pow(vol / want, 1.0 / (double)k);
      if (!(c > 0.f) || !me_finite(c)) c = fmaxf(fmaxf(ext[0], ext[1]), ext[2]);
      int n[3] = {1, 1, 1};
      bool fits = false;
      for (int it = 0; it < 400 && !fits; ++it) {
        double cells = 1.0;
        for (int d = 0; d < 3; ++d) {
          const float e = ext[d] / c;
          n[d] = (e < 1.0e6f) ? (int)e + 1 : 1000001;
          cells *= (double)n[d];
        }
        fits = cells <= (double)a.max_cells;
        if (!fits) c *= 1.26f;
      }
      if (fits && me_finite(c) && me_finite(1.0f / c)) {
        h.c = c; h.inv_c = 1.0f / c;
        h.nx = n[0]; h.ny = n[1]; h.nz = n[2]; h.ncells = n[0] * n[1] * n[2]; h.nmax = max(n[0], max(n[1], n[2]));
      }
    }
  }
  h.valid = valid ? 1 : 0;
  *a.hdr = h;
}

// cell coordinate along one axis: clamped as a float first, so neither a NaN nor a value beyond int ever becomes an index
__device__ __forceinline__ int np_cell1(float g, int n) { return (int)fminf(fmaxf(floorf(g), 0.f), (float)(n - 1)); }
__device__ __forceinline__ int np_cell_of(const NpGridHdr& h, float x, float y, float z) {
  const int ix = np_cell1((x - h.x0) * h.inv_c, h.nx), iy = np_cell1((y - h.y0) * h.inv_c, h.ny), iz = np_cell1((z - h.z0) * h.inv_c, h.nz);
  return (iz * h.ny + iy) * h.nx + ix;
}

__global__ __launch_bounds__(256) void k_np_clear(NpArgs a) {
  const int nc = min(a.hdr->ncells, a.max_cells);
  for (int i = blockIdx.x * 256 + threadIdx.x; i <= nc; i += gridDim.x * 256) { a.cell_start[i] = 0; if (i < nc) a.cell_fill[i] = 0; }
}
__global__ __launch_bounds__(256) void k_np_count(NpArgs a) {
  const NpGridHdr h = *a.hdr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.M; i += (int64_t)gridDim.x * 256) {
    const float x = a.refs[3 * i], y = a.refs[3 * i + 1], z = a.refs[3 * i + 2];
    if (me_finite(x) && me_finite(y) && me_finite(z)) atomicAdd(&a.cell_start[np_cell_of(h, x, y, z)], 1);
  }
}
__global__ __launch_bounds__(256) void k_np_fill(NpArgs a) {
  const NpGridHdr h = *a.hdr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.M; i += (int64_t)gridDim.x * 256) {
    const float x = a.refs[3 * i], y = a.refs[3 * i + 1], z = a.refs[3 * i + 2];
    if (!(me_finite(x) && me_finite(y) && me_finite(z))) continue;
    const int cidx = np_cell_of(h, x, y, z);
    const int slot = a.cell_start[cidx] + atomicAdd(&a.cell_fill[cidx], 1);
    if (slot >= 0 && slot < a.M) a.sorted[slot] = make_float4(x, y, z, __int_as_float((int)i));
  }
}

// The (2 r + 1)^3 block of cells around the query's cell, clipped to the grid, has been searched after ring r.  A
// reference not yet seen lies in a cell beyond one of the block's faces, and only a face that is not on the grid's boundary
// has cells behind it; such a reference is at least the gap from the query to that face's plane away.  The cell
// coordinate g(x) = (x - x0) * inv_c is monotonic in x and is computed for queries exactly as it was for the references,
// so the gap in cell units, less the rounding of g (a few 2^-24 of its magnitude, which is at most the grid's size for a
// plane of the grid, and relative to the gap itself where the query is far outside), times c, is a lower bound.
__global__ __launch_bounds__(256) void k_np_query(NpArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  const NpGridHdr h = *a.hdr;
  const float x = a.queries[3 * (int64_t)i], y = a.queries[3 * (int64_t)i + 1], z = a.queries[3 * (int64_t)i + 2];
  if (!(me_finite(x) && me_finite(y) && me_finite(z))) { a.dist[i] = __int_as_float(0x7fc00000); a.index[i] = -1; return; }
  if (!h.valid) { a.dist[i] = INFINITY; a.index[i] = -1; return; }
  const float gx = (x - h.x0) * h.inv_c, gy = (y - h.y0) * h.inv_c, gz = (z - h.z0) * h.inv_c;
  const int ix = np_cell1(gx, h.nx), iy = np_cell1(gy, h.ny), iz = np_cell1(gz, h.nz);
  const float slack = 2.0e-6f * (float)(h.nmax + 2);
  // a lower bound, in world units, of a gap given in cell units
  auto world_gap = [&](float cells) { return fmaxf(cells * (1.0f - 2.0e-6f) - slack, 0.f) * h.c * (1.0f - 2.0e-6f); };
  float best = INFINITY;
  int bi = -1;
  auto visit = [&](int j0, int j1) __attribute__((always_inline)) {
    for (int j = j0; j < j1; ++j) {
      const float4 c = a.sorted[j];
      const float dx = x - c.x, dy = y - c.y, dz = z - c.z;
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      if (d < best || bi < 0) { best = d; bi = __float_as_int(c.w); }
    }
  };
  for (int r = 0;; ++r) {
    const int xlo = max(ix - r, 0), xhi = min(ix + r, h.nx - 1);
    const int ylo = max(iy - r, 0), yhi = min(iy + r, h.ny - 1);
    const int zlo = max(iz - r, 0), zhi = min(iz + r, h.nz - 1);
    for (int cz = zlo; cz <= zhi; ++cz) {
      const float lz = fmaxf(fmaxf((float)cz - gz, gz - (float)(cz + 1)), 0.f);
      for (int cy = ylo; cy <= yhi; ++cy) {
        const float ly = fmaxf(fmaxf((float)cy - gy, gy - (float)(cy + 1)), 0.f);
        if (world_gap(fmaxf(ly, lz)) > best) continue;             // nothing in this row can be closer
        const int rowb = (cz * h.ny + cy) * h.nx;
        if (abs(cz - iz) == r || abs(cy - iy) == r) {              // a row of the shell: its cells are one range
          visit(a.cell_start[rowb + xlo], a.cell_start[rowb + xhi + 1]);
        } else {                                                    // an inner row: the shell's two end cells
          if (ix - r >= 0) visit(a.cell_start[rowb + ix - r], a.cell_start[rowb + ix - r + 1]);
          if (ix + r <= h.nx - 1) visit(a.cell_start[rowb + ix + r], a.cell_start[rowb + ix + r + 1]);
        }
      }
    }
    float gap = INFINITY;                                          // faces with cells behind them
    if (ix - r > 0) gap = fminf(gap, gx - (float)(ix - r));
    if (ix + r < h.nx - 1) gap = fminf(gap, (float)(ix + r + 1) - gx);
    if (iy - r > 0) gap = fminf(gap, gy - (float)(iy - r));
    if (iy + r < h.ny - 1) gap = fminf(gap, (float)(iy + r + 1) - gy);
    if (iz - r > 0) gap = fminf(gap, gz - (float)(iz - r));
    if (iz + r < h.nz - 1) gap = fminf(gap, (float)(iz + r + 1) - gz);
    if (gap == INFINITY) break;                                    // the grid is exhausted
    if (best <= world_gap(gap)) break;
  }
  a.dist[i] = best;
  a.index[i] = (int64_t)bi;
}

// cells of the grid over the references: 2 per reference (k_np_header), bounded
static int np_max_cells(int64_t M) { return (int)std::min<int64_t>(std::max<int64_t>(2 * M, 64), 1 << 22); }
// workspace: the grid over the references and the references grouped by its cells (a.M is set; the queries take none)
static void np_layout(NpArgs& a, WsArena& ws) {
  a.max_cells = np_max_cells(a.M);
  a.hdr = ws.take<NpGridHdr>(1);
  a.part = ws.take<float>(6 * NP_BBOX_BLOCKS);
  a.cell_start = ws.take<int>((int64_t)a.max_cells + 1);
  a.cell_fill = ws.take<int>(a.max_cells);
  a.scan_part = ws.take<int>(scan_partial_count<ME_SCAN_PER>(a.max_cells) + 1);
  a.sorted = ws.take<float4>(a.M);
}
int64_t ngm_nearest_point_bytes(int64_t M, int64_t N) {
  (void)N;
  NpArgs a = {};
  a.M = (int)M;
  return ws_bytes(np_layout, a);
}
// the grid over a.refs, built once: bounding box -> header -> counts -> exclusive scan -> cell-sorted copy
static void np_build_grid(const NpArgs& a, hipStream_t st) {
  const unsigned ref_blocks = (unsigned)std::min<int64_t>(((int64_t)a.M + 255) / 256, 8192);
  hipLaunchKernelGGL(k_np_bbox, dim3((unsigned)a.bbox_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_np_header, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_np_clear, dim3((unsigned)std::min((a.max_cells + 256) / 256, 4096)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_np_count, dim3(ref_blocks), dim3(256), 0, st, a);
  launch_scan<int, ME_SCAN_PER, false>(a.cell_start, &a.hdr->ncells, a.max_cells, a.scan_part, st);
  hipLaunchKernelGGL(k_np_fill, dim3(ref_blocks), dim3(256), 0, st, a);
}
int ngm_launch_nearest_point(const float* refs, int64_t M, const float* queries, int64_t N, float* dist, int64_t* index, void* workspace,
                             int64_t workspace_bytes, hipStream_t st) {
  NpArgs a = {};
  a.refs = refs; a.queries = queries; a.M = (int)M; a.N = (int)N; a.dist = dist; a.index = index;
  a.bbox_blocks = (int)std::min<int64_t>((M + 255) / 256, NP_BBOX_BLOCKS);
  WsArena ws(workspace);
  np_layout(a, ws);
  if (!ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  if (N == 0) return 0;
  np_build_grid(a, st);
  hipLaunchKernelGGL(k_np_query, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a);
  return 0;
}

// ---- subdivision to a maximum edge length -------------------------------------------------------------------------------
// trimesh.Trimesh.subdivide_to_size (mesh_culling.py:260-261) in closed form: a face whose longest edge L needs k exact
// halvings until L > max_edge is false becomes the uniform split into 4^k children, n = 2^k segments per edge (the rule and
// the orders are written down in include/ngm_hip.h).
//   k_sub_level  : one thread per face: level, number of children, number of new vertices; the largest level by atomic max
//   k_scan_*     : exclusive int64 scans of the two counts (the scans above); k_sub_totals: the three totals
//   k_sub_faces  : one thread per OUTPUT face: parent by binary search in the scanned child counts, row formula -> (i, j)
//   k_sub_verts  : one thread per OUTPUT vertex: parent by binary search in the scanned vertex counts, row formula -> (i, j)
// A workgroup's first and last thread search all faces, the others between the two parents found: no thread loops over children.
// After it: vertex normals (k_vn_*) and point-to-plane ICP (k_icp_*) -- evaluation._align_mesh, evaluation.py:133-160.
constexpr int SUB_MAX_ITER = 10;
constexpr int SUB_T = 256;

struct SubArgs {
  const float* verts; const int64_t* faces; const float* attrs;
  int64_t V, F;
  int C;
  int* level;           // (F)
  int64_t* vscan;       // (F + 1) new vertices per face, then their exclusive scan; [F] = total
  int64_t* fscan;       // (F + 1) child faces per face, likewise
  int64_t* totals;      // [new vertices, output faces, largest level]
  double max_edge; int max_iter;
  int64_t new_vertices, out_faces;
  float* out_verts; int64_t* out_faces_idx; float* out_attrs; int64_t* out_parent;
};

__device__ __forceinline__ double sub_edge(const float* p, const float* q) {
  const double dx = (double)q[0] - (double)p[0], dy = (double)q[1] - (double)p[1], dz = (double)q[2] - (double)p[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);              // contraction is off in this file: no fused multiply-add
}

__global__ __launch_bounds__(SUB_T) void k_sub_level(SubArgs a) {
  __shared__ int red[SUB_T];
  const int64_t f = (int64_t)blockIdx.x * SUB_T + threadIdx.x;
  int k = 0;
  if (f < a.F) {
    const int64_t i0 = a.faces[3 * f], i1 = a.faces[3 * f + 1], i2 = a.faces[3 * f + 2];
    if (i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V) {
      const float *p0 = a.verts + 3 * i0, *p1 = a.verts + 3 * i1, *p2 = a.verts + 3 * i2;
      const double l0 = sub_edge(p0, p1), l1 = sub_edge(p1, p2), l2 = sub_edge(p2, p0);
      // the longest as np.max takes it: a NaN length makes it NaN, which compares false -- level 0
      double L = l0;
      if (l1 > L) L = l1;
      if (l2 > L) L = l2;
      const bool nan = l0 != l0 || l1 != l1 || l2 != l2;
      // halving is exact; +inf never passes and ends one past max_iter, as does every length that needs more rounds
      while (!nan && L > a.max_edge && k <= a.max_iter) { L *= 0.5; ++k; }
    }
    const bool ok = k <= a.max_iter;                       // beyond max_iter the caller refuses: the face counts as unsplit
    const int64_t n = (int64_t)1 << (ok ? k : 0);
    a.level[f] = k;
    a.fscan[f] = n * n;
    a.vscan[f] = (n + 1) * (n + 2) / 2 - 3;
  }
  red[threadIdx.x] = k;
  __syncthreads();
  for (int s = SUB_T / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0] > 0) atomicMax(reinterpret_cast<unsigned long long*>(a.totals + 2), (unsigned long long)red[0]);
}

__global__ void k_sub_totals(SubArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { a.totals[0] = a.vscan[a.F]; a.totals[1] = a.fscan[a.F]; }
}

// the face p with scan[p] <= g < scan[p + 1], searched in [lo, hi] (scan has F + 1 entries, scan[F] the total); F when
// g is at or beyond scan[hi + 1]
__device__ __forceinline__ int64_t sub_parent(const int64_t* scan, int64_t lo, int64_t hi, int64_t g) {
  int64_t l = lo, h = hi + 1;                              // first index in [lo, hi + 1] with scan[index + 1] > g
  while (l < h) { const int64_t mid = l + ((h - l) >> 1); if (scan[mid + 1] > g) h = mid; else l = mid + 1; }
  return l;
}
// parent of output element g for every thread of the workgroup: threads 0 and SUB_T - 1 search [0, F - 1], the rest between them
__device__ __forceinline__ int64_t sub_parent_block(const int64_t* scan, int64_t F, int64_t g, int64_t total, int64_t* lds) {
  const int t = threadIdx.x;
  const bool in = g < total;
  int64_t p = F;
  if (t == 0 || t == SUB_T - 1) {
    // the last thread may stand beyond the total: it searches for the last element instead
    p = sub_parent(scan, 0, F - 1, in ? g : total - 1);
    lds[t == 0 ? 0 : 1] = p;
  }
  __syncthreads();
  if (t != 0 && t != SUB_T - 1 && in) p = sub_parent(scan, lds[0], min(lds[1], F - 1), g);
  return in ? p : F;
}

__device__ __forceinline__ int sub_isqrt_ceil(int m) {     // ceil(sqrt(m)), 1 <= m <= 2^20
  int s = (int)sqrtf((float)m);
  while (s * s < m) ++s;
  while (s > 0 && (s - 1) * (s - 1) >= m) --s;
  return s;
}
// index of lattice point (i, j) of face p in the output vertices: the corners are the originals
__device__ __forceinline__ int64_t sub_vertex_index(const SubArgs& a, int64_t p, int n, int i, int j, const int64_t (&c)[3]) {
  if (i == 0 && j == 0) return c[0];
  if (i == n && j == 0) return c[1];
  if (i == 0 && j == n) return c[2];
  const int lin = j * (n + 1) - j * (j - 1) / 2 + i;       // row j holds i = 0 .. n - j
  return a.V + a.vscan[p] + (lin - 1 - (lin > n ? 1 : 0));
}

__global__ __launch_bounds__(SUB_T) void k_sub_faces(SubArgs a) {
  __shared__ int64_t lds[2];
  const int64_t g = (int64_t)blockIdx.x * SUB_T + threadIdx.x;
  const int64_t total = min(a.out_faces, a.fscan[a.F]);
  if ((int64_t)blockIdx.x * SUB_T >= total) return;        // the whole workgroup: nothing before the barrier
  const int64_t p = sub_parent_block(a.fscan, a.F, g, total, lds);
  if (p >= a.F) return;
  const int64_t c[3] = {a.faces[3 * p], a.faces[3 * p + 1], a.faces[3 * p + 2]};
  const int64_t children = a.fscan[p + 1] - a.fscan[p];
  int64_t o[3] = {c[0], c[1], c[2]};
  if (children > 1) {
    const int n = 1 << ((63 - __clzll((unsigned long long)children)) >> 1);   // children = n * n
    const int t = (int)(g - a.fscan[p]);
    // row j holds 2 (n - j) - 1 children, r (2 n - r) come before row r: j = n - ceil(sqrt(n^2 - t))
    const int j = n - sub_isqrt_ceil(n * n - t);
    const int u = t - j * (2 * n - j);
    const int i = u >> 1;
    if ((u & 1) == 0) {                                    // upright: (i, j) (i + 1, j) (i, j + 1)
      o[0] = sub_vertex_index(a, p, n, i, j, c); o[1] = sub_vertex_index(a, p, n, i + 1, j, c); o[2] = sub_vertex_index(a, p, n, i, j + 1, c);
    } else {                                               // inverted: (i + 1, j) (i + 1, j + 1) (i, j + 1)
      o[0] = sub_vertex_index(a, p, n, i + 1, j, c); o[1] = sub_vertex_index(a, p, n, i + 1, j + 1, c); o[2] = sub_vertex_index(a, p, n, i, j + 1, c);
    }
  }
  a.out_faces_idx[3 * g] = o[0]; a.out_faces_idx[3 * g + 1] = o[1]; a.out_faces_idx[3 * g + 2] = o[2];
  a.out_parent[g] = p;
}

// x0 w0 + x1 w1 + x2 w2 in fp64, a term of weight 0 left out, rounded once to fp32.  The weights are multiples of 2^-10 and
// the values have 24 bits: every product is exact.  On a parent's edge one weight is 0, so the value is ONE rounding of the
// exact sum of two products that depend on the edge's two ends and the position along it alone -- the same bits from either
// face that shares the edge, in either order of its corners (fp64 addition commutes), at any two levels.
__device__ __forceinline__ float sub_mix(float x0, float x1, float x2, double w0, double w1, double w2) {
  const double t0 = (double)x0 * w0, t1 = (double)x1 * w1, t2 = (double)x2 * w2;
  double s;
  if (w0 == 0.0) s = (w1 == 0.0) ? t2 : ((w2 == 0.0) ? t1 : t1 + t2);
  else if (w1 == 0.0) s = (w2 == 0.0) ? t0 : t0 + t2;
  else if (w2 == 0.0) s = t0 + t1;
  else s = (t0 + t1) + t2;
  return (float)s;
}

__global__ __launch_bounds__(SUB_T) void k_sub_verts(SubArgs a) {
  __shared__ int64_t lds[2];
  const int64_t g = (int64_t)blockIdx.x * SUB_T + threadIdx.x;      // over the NEW vertices
  const int64_t total = min(a.new_vertices, a.vscan[a.F]);
  if ((int64_t)blockIdx.x * SUB_T >= total) return;
  const int64_t p = sub_parent_block(a.vscan, a.F, g, total, lds);
  if (p >= a.F) return;
  const int64_t count = a.vscan[p + 1] - a.vscan[p];                // (n + 1)(n + 2) / 2 - 3 > 0: the indices were in range
  const int64_t children = a.fscan[p + 1] - a.fscan[p];
  const int n = 1 << ((63 - __clzll((unsigned long long)children)) >> 1);
  const int64_t c0 = a.faces[3 * p], c1 = a.faces[3 * p + 1], c2 = a.faces[3 * p + 2];
  const int l = (int)(g - a.vscan[p]);
  if (count <= 0 || n < 2 || c0 < 0 || c0 >= a.V || c1 < 0 || c1 >= a.V || c2 < 0 || c2 >= a.V) return;
  const int lin = l + 1 + (l + 1 >= n ? 1 : 0);            // the lattice point's number with the corners counted
  // row j starts at j (2 n + 3 - j) / 2: the largest j whose start is <= lin
  const int b = 2 * n + 3;
  int j = (int)(((float)b - sqrtf(fmaxf((float)(b * b - 8 * lin), 0.f))) * 0.5f);
  j = max(0, min(j, n));
  while (j < n && (j + 1) * (b - (j + 1)) / 2 <= lin) ++j;
  while (j > 0 && j * (b - j) / 2 > lin) --j;
  const int i = lin - j * (b - j) / 2;
  const double inv = 1.0 / (double)n;                      // a power of two: every weight below is exact
  const double w0 = (double)(n - i - j) * inv, w1 = (double)i * inv, w2 = (double)j * inv;
  const int64_t o = a.V + g;
#pragma unroll
  for (int d = 0; d < 3; ++d) a.out_verts[3 * o + d] = sub_mix(a.verts[3 * c0 + d], a.verts[3 * c1 + d], a.verts[3 * c2 + d], w0, w1, w2);
  for (int ch = 0; ch < a.C; ++ch)
    a.out_attrs[o * a.C + ch] = sub_mix(a.attrs[c0 * a.C + ch], a.attrs[c1 * a.C + ch], a.attrs[c2 * a.C + ch], w0, w1, w2);
}

// the V originals, unchanged and in place
__global__ __launch_bounds__(SUB_T) void k_sub_copy(SubArgs a) {
  const int64_t g = (int64_t)blockIdx.x * SUB_T + threadIdx.x;
  if (g < 3 * a.V) a.out_verts[g] = a.verts[g];
  if (a.C > 0 && g < a.V * a.C) a.out_attrs[g] = a.attrs[g];
}

struct SubLayout { int* level; int64_t* vscan; int64_t* fscan; int64_t* partial; };
// workspace: count and emit see the same layout from F alone
static SubLayout sub_layout(int64_t F, WsArena& ws) {
  SubLayout l;
  l.level = ws.take<int>(F);
  l.vscan = ws.take<int64_t>(F + 1);
  l.fscan = ws.take<int64_t>(F + 1);
  l.partial = ws.take<int64_t>(scan_partial_count<ME_SCAN_PER>(F) + 1);
  return l;
}
int64_t ngm_mesh_subdivide_bytes(int64_t F) { return ws_bytes(sub_layout, F); }
int ngm_launch_mesh_subdivide_count(const float* verts, int64_t V, const int64_t* faces, int64_t F, double max_edge, int max_iter,
                                    void* workspace, int64_t workspace_bytes, int64_t* totals, hipStream_t st) {
  if (max_iter < 0 || max_iter > SUB_MAX_ITER) return -1;
  WsArena ws(workspace);
  const SubLayout l = sub_layout(F, ws);
  if (F > 0 && !ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  if (hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), st) != hipSuccess) return -4;
  if (F == 0) return 0;
  SubArgs a = {};
  a.verts = verts; a.faces = faces; a.V = V; a.F = F; a.level = l.level; a.vscan = l.vscan; a.fscan = l.fscan; a.totals = totals;
  a.max_edge = max_edge; a.max_iter = max_iter;
  hipLaunchKernelGGL(k_sub_level, dim3((unsigned)((F + SUB_T - 1) / SUB_T)), dim3(SUB_T), 0, st, a);
  launch_scan<int64_t, ME_SCAN_PER, false>(l.vscan, nullptr, F, l.partial, st);
  launch_scan<int64_t, ME_SCAN_PER, false>(l.fscan, nullptr, F, l.partial, st);
  hipLaunchKernelGGL(k_sub_totals, dim3(1), dim3(64), 0, st, a);
  return 0;
}
int ngm_launch_mesh_subdivide_emit(const float* verts, int64_t V, const int64_t* faces, int64_t F, const float* attrs, int C,
                                   const void* workspace, int64_t new_vertices, int64_t out_faces, float* out_verts,
                                   int64_t* out_faces_idx, float* out_attrs, int64_t* out_parent, hipStream_t st) {
  WsArena ws(workspace);
  const SubLayout l = sub_layout(F, ws);
  SubArgs a = {};
  a.verts = verts; a.faces = faces; a.attrs = attrs; a.V = V; a.F = F; a.C = attrs ? C : 0;
  a.level = l.level; a.vscan = l.vscan; a.fscan = l.fscan;
  a.new_vertices = new_vertices; a.out_faces = out_faces;
  a.out_verts = out_verts; a.out_faces_idx = out_faces_idx; a.out_attrs = out_attrs; a.out_parent = out_parent;
  const int64_t copy = std::max<int64_t>(3 * V, V * a.C);
  if (copy > 0) hipLaunchKernelGGL(k_sub_copy, dim3((unsigned)((copy + SUB_T - 1) / SUB_T)), dim3(SUB_T), 0, st, a);
  if (F > 0 && new_vertices > 0)
    hipLaunchKernelGGL(k_sub_verts, dim3((unsigned)((new_vertices + SUB_T - 1) / SUB_T)), dim3(SUB_T), 0, st, a);
  if (F > 0 && out_faces > 0)
    hipLaunchKernelGGL(k_sub_faces, dim3((unsigned)((out_faces + SUB_T - 1) / SUB_T)), dim3(SUB_T), 0, st, a);
  return 0;
}

// ---- vertex normals ---------------------------------------------------------------------------------------------------
// Open3D's compute_vertex_normals: every face adds (v1 - v0) x (v2 - v0) to its three vertices, the sums are normalised.
// The sums are EXACT integer sums, so neither the order of the faces nor the order of the atomics shows:
//   k_vn_clear : exponent, valence and the three int64 sums of every vertex
//   k_vn_scale : per face: atomic max of the largest binary exponent among its normal's components, valence + 1, per corner
//   k_vn_add   : per face: the normal again (fp64 from the fp32 vertices), times 2^(62 - e_v - ceil(log2(valence + 1))), rounded
//                to int64 and added: |term| <= 2^(62 - L) and valence < 2^L, so the sum stays below 2^62
//   k_vn_finish: per vertex: normalise in fp64, round to fp32; (0, 0, 1) for a sum of length 0 or a non-finite vertex
// No thread loops over the faces of a vertex: a fan of any valence costs its faces one atomic each per pass.
constexpr int VN_EMPTY = -(1 << 20);
struct VnArgs {
  const float* verts; const int64_t* faces;
  int64_t V, F;
  int* emax;                       // (V)
  unsigned long long* valence;     // (V)
  unsigned long long* acc;         // (V, 3) int64 sums, two's complement
  float* normals;
};

// the corners' indices and the unnormalised normal of face f; false when the face adds nothing
__device__ __forceinline__ bool vn_face(const VnArgs& a, int64_t f, int64_t (&ix)[3], double (&n)[3]) {
  float p[3][3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t i = a.faces[3 * f + k];
    ix[k] = i;
    if (i < 0 || i >= a.V) { ok = false; p[k][0] = p[k][1] = p[k][2] = 0.f; continue; }
#pragma unroll
    for (int d = 0; d < 3; ++d) { p[k][d] = a.verts[3 * i + d]; ok = ok && me_finite(p[k][d]); }
  }
  const double ax = (double)p[1][0] - (double)p[0][0], ay = (double)p[1][1] - (double)p[0][1], az = (double)p[1][2] - (double)p[0][2];
  const double bx = (double)p[2][0] - (double)p[0][0], by = (double)p[2][1] - (double)p[0][1], bz = (double)p[2][2] - (double)p[0][2];
  n[0] = ay * bz - az * by; n[1] = az * bx - ax * bz; n[2] = ax * by - ay * bx;       // finite: |products| < 2^258
  return ok;
}
// e with |v| < 2^e for a finite v != 0 (frexp's exponent); VN_EMPTY for 0.  The products of fp32 differences are never subnormal.
__device__ __forceinline__ int vn_exponent(double v) {
  if (v == 0.0) return VN_EMPTY;
  return (int)((__double_as_longlong(v) >> 52) & 0x7ff) - 1022;
}

__global__ __launch_bounds__(256) void k_vn_clear(VnArgs a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  a.emax[v] = VN_EMPTY; a.valence[v] = 0ull;
  a.acc[3 * v] = 0ull; a.acc[3 * v + 1] = 0ull; a.acc[3 * v + 2] = 0ull;
}
__global__ __launch_bounds__(256) void k_vn_scale(VnArgs a) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  int64_t ix[3];
  double n[3];
  if (!vn_face(a, f, ix, n)) return;
  const int e = max(vn_exponent(n[0]), max(vn_exponent(n[1]), vn_exponent(n[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (e != VN_EMPTY) atomicMax(&a.emax[ix[k]], e);
    atomicAdd(&a.valence[ix[k]], 1ull);
  }
}
__global__ __launch_bounds__(256) void k_vn_add(VnArgs a) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  int64_t ix[3];
  double n[3];
  if (!vn_face(a, f, ix, n)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = a.emax[ix[k]];
    if (e == VN_EMPTY) continue;                                     // every normal at this vertex is exactly zero
    const int L = 64 - __clzll((long long)a.valence[ix[k]]);          // ceil(log2(valence + 1)), valence >= 1 here
    const int shift = 62 - e - L;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const long long q = llrint(ldexp(n[d], shift));
      if (q != 0) atomicAdd(&a.acc[3 * ix[k] + d], (unsigned long long)q);
    }
  }
}
__global__ __launch_bounds__(256) void k_vn_finish(VnArgs a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  float o[3] = {0.f, 0.f, 1.f};
  if (me_finite(a.verts[3 * v]) && me_finite(a.verts[3 * v + 1]) && me_finite(a.verts[3 * v + 2])) {
    const double sx = (double)(long long)a.acc[3 * v], sy = (double)(long long)a.acc[3 * v + 1], sz = (double)(long long)a.acc[3 * v + 2];
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);          // the common scale 2^shift cancels
    if (len > 0.0) { o[0] = (float)(sx / len); o[1] = (float)(sy / len); o[2] = (float)(sz / len); }
  }
  a.normals[3 * v] = o[0]; a.normals[3 * v + 1] = o[1]; a.normals[3 * v + 2] = o[2];
}

static void vn_layout(VnArgs& a, WsArena& ws) {
  a.emax = ws.take<int>(a.V);
  a.valence = ws.take<unsigned long long>(a.V);
  a.acc = ws.take<unsigned long long>(3 * a.V);
}
int64_t ngm_mesh_vertex_normals_bytes(int64_t V) {
  VnArgs a = {};
  a.V = V;
  return ws_bytes(vn_layout, a);
}
int ngm_launch_mesh_vertex_normals(const float* verts, int64_t V, const int64_t* faces, int64_t F, float* normals, void* workspace,
                                   int64_t workspace_bytes, hipStream_t st) {
  VnArgs a = {};
  a.verts = verts; a.faces = faces; a.V = V; a.F = F; a.normals = normals;
  WsArena ws(workspace);
  vn_layout(a, ws);
  if (!ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  if (V == 0) return 0;
  const unsigned vb = (unsigned)((V + 255) / 256), fb = (unsigned)((F + 255) / 256);
  hipLaunchKernelGGL(k_vn_clear, dim3(vb), dim3(256), 0, st, a);
  if (F > 0) {
    hipLaunchKernelGGL(k_vn_scale, dim3(fb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_vn_add, dim3(fb), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_vn_finish, dim3(vb), dim3(256), 0, st, a);
  return 0;
}

// ---- point-to-plane ICP -------------------------------------------------------------------------------------------------
// Open3D's registration_icp with TransformationEstimationPointToPlane (evaluation._align_mesh, evaluation.py:133-160); the
// rules are written down in include/ngm_hip.h.  The grid over the target is built ONCE (np_build_grid); then per pass
//   k_icp_accumulate : a FIXED grid of ICP_BLOCKS x ICP_T threads strides over the source points: p = R s + t in fp64, the ring
//                      search of k_np_query from (float)p -- ties to the smallest original index, stopped where the proven gap
//                      is beyond the threshold --, the correspondence test in fp64, 29 fp64 sums in registers; reduced per
//                      wave (shuffles), per workgroup (LDS), one row of ICP_ROW doubles per workgroup, written on every pass
//   k_icp_solve      : one workgroup: the rows in a fixed order, fitness / rmse / convergence, 6 x 6 Cholesky by one thread,
//                      T <- U T.  Once it sets `done` in the state both kernels of the remaining passes return at once.
// Nothing is read back; all passes are enqueued at once.
constexpr int ICP_BLOCKS = 1024, ICP_T = 256, ICP_SUMS = 29, ICP_ROW = 32;
constexpr int ICP_S_FITNESS = 16, ICP_S_RMSE = 17, ICP_S_ITER = 18, ICP_S_CONV = 19, ICP_S_SUMS = 20, ICP_S_DONE = 49, ICP_STATE = 64;
struct IcpArgs {
  NpArgs np;                 // the grid over the target
  const float* source; const float* normals;
  int N, max_iteration;
  double threshold, relative_fitness, relative_rmse;
  double* state;             // (64) on the device
  double* partial;           // (ICP_BLOCKS, ICP_ROW)
};
struct IcpInit { double t[16]; };

__global__ void k_icp_init(double* state, IcpInit init) {
  const int t = threadIdx.x;
  if (t < ICP_STATE) state[t] = t < 16 ? init.t[t] : 0.0;
}

// k_np_query's search with three differences: equal distances go to the smallest original index (and the search goes on
// while an unseen point could TIE), rows and rings whose proven gap exceeds `stop` are left out, and the coordinates of the
// point found come back with its index.  -1: no finite target within `stop`.
__device__ __forceinline__ int icp_search(const NpArgs& a, const NpGridHdr& h, float x, float y, float z, float stop, float (&q)[3]) {
  const float gx = (x - h.x0) * h.inv_c, gy = (y - h.y0) * h.inv_c, gz = (z - h.z0) * h.inv_c;
  const int ix = np_cell1(gx, h.nx), iy = np_cell1(gy, h.ny), iz = np_cell1(gz, h.nz);
  const float slack = 2.0e-6f * (float)(h.nmax + 2);
  auto world_gap = [&](float cells) { return fmaxf(cells * (1.0f - 2.0e-6f) - slack, 0.f) * h.c * (1.0f - 2.0e-6f); };
  float best = INFINITY;
  int bi = -1;
  auto visit = [&](int j0, int j1) __attribute__((always_inline)) {
    for (int j = j0; j < j1; ++j) {
      const float4 c = a.sorted[j];
      const float dx = x - c.x, dy = y - c.y, dz = z - c.z;
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      const int id = __float_as_int(c.w);
      if (bi < 0 || d < best || (d == best && id < bi)) { best = d; bi = id; q[0] = c.x; q[1] = c.y; q[2] = c.z; }
    }
  };
  for (int r = 0;; ++r) {
    const int xlo = max(ix - r, 0), xhi = min(ix + r, h.nx - 1);
    const int ylo = max(iy - r, 0), yhi = min(iy + r, h.ny - 1);
    const int zlo = max(iz - r, 0), zhi = min(iz + r, h.nz - 1);
    for (int cz = zlo; cz <= zhi; ++cz) {
      const float lz = fmaxf(fmaxf((float)cz - gz, gz - (float)(cz + 1)), 0.f);
      for (int cy = ylo; cy <= yhi; ++cy) {
        const float ly = fmaxf(fmaxf((float)cy - gy, gy - (float)(cy + 1)), 0.f);
        if (world_gap(fmaxf(ly, lz)) > fminf(best, stop)) continue; // nothing in this row can be closer, or as close as `stop`
        const int rowb = (cz * h.ny + cy) * h.nx;
        if (abs(cz - iz) == r || abs(cy - iy) == r) {
          visit(a.cell_start[rowb + xlo], a.cell_start[rowb + xhi + 1]);
        } else {
          if (ix - r >= 0) visit(a.cell_start[rowb + ix - r], a.cell_start[rowb + ix - r + 1]);
          if (ix + r <= h.nx - 1) visit(a.cell_start[rowb + ix + r], a.cell_start[rowb + ix + r + 1]);
        }
      }
    }
    float gap = INFINITY;
    if (ix - r > 0) gap = fminf(gap, gx - (float)(ix - r));
    if (ix + r < h.nx - 1) gap = fminf(gap, (float)(ix + r + 1) - gx);
    if (iy - r > 0) gap = fminf(gap, gy - (float)(iy - r));
    if (iy + r < h.ny - 1) gap = fminf(gap, (float)(iy + r + 1) - gy);
    if (iz - r > 0) gap = fminf(gap, gz - (float)(iz - r));
    if (iz + r < h.nz - 1) gap = fminf(gap, (float)(iz + r + 1) - gz);
    if (gap == INFINITY) break;
    const float wg = world_gap(gap);
    if (best < wg || wg > stop) break;                             // strictly: a point at exactly `best` may carry a smaller index
  }
  return bi;
}

__global__ __launch_bounds__(ICP_T) void k_icp_accumulate(IcpArgs a) {
  __shared__ double red[ICP_T / 64][ICP_ROW];
  if (a.state[ICP_S_DONE] != 0.0) return;                           // the same for every thread: nobody reaches the barrier
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = a.state[i];
  const NpGridHdr h = *a.np.hdr;
  double acc[ICP_SUMS];
#pragma unroll
  for (int i = 0; i < ICP_SUMS; ++i) acc[i] = 0.0;
  const float thr_f = (float)a.threshold * 1.0001f;
  for (int64_t i = (int64_t)blockIdx.x * ICP_T + threadIdx.x; i < a.N; i += (int64_t)ICP_BLOCKS * ICP_T) {
    const float sx = a.source[3 * i], sy = a.source[3 * i + 1], sz = a.source[3 * i + 2];
    if (!(me_finite(sx) && me_finite(sy) && me_finite(sz)) || !h.valid) continue;
    const double px = ((T[0] * (double)sx + T[1] * (double)sy) + T[2] * (double)sz) + T[3];
    const double py = ((T[4] * (double)sx + T[5] * (double)sy) + T[6] * (double)sz) + T[7];
    const double pz = ((T[8] * (double)sx + T[9] * (double)sy) + T[10] * (double)sz) + T[11];
    const float x = (float)px, y = (float)py, z = (float)pz;
    if (!(me_finite(x) && me_finite(y) && me_finite(z))) continue;
    // beyond `stop` from (float)p means beyond the threshold from p: the rounding of p is 2^-24 of each coordinate
    const float stop = thr_f + 4.0e-7f * ((fabsf(x) + fabsf(y)) + fabsf(z));
    float q[3];
    const int bi = icp_search(a.np, h, x, y, z, stop, q);
    if (bi < 0) continue;
    const double dx = px - (double)q[0], dy = py - (double)q[1], dz = pz - (double)q[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(sqrt(d2) < a.threshold)) continue;
    const float nxf = a.normals[3 * (int64_t)bi], nyf = a.normals[3 * (int64_t)bi + 1], nzf = a.normals[3 * (int64_t)bi + 2];
    if (!(me_finite(nxf) && me_finite(nyf) && me_finite(nzf))) continue;
    const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
    const double rr = (dx * nx + dy * ny) + dz * nz;
    const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) acc[k++] += J[r] * J[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] += J[r] * rr;
    acc[27] += d2;
    acc[28] += 1.0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < ICP_SUMS; ++s) {
    double v = acc[s];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) red[wave][s] = v;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < ICP_ROW) a.partial[(int64_t)blockIdx.x * ICP_ROW + t] = t < ICP_SUMS ? ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t] : 0.0;
}

// x of A x = b by Cholesky, A the 21 upper entries row by row; false (nothing written) where a pivot is not above
// 1e-12 x the largest diagonal entry or the solution is not finite
__device__ bool icp_cholesky(const double* up, const double* b, double (&x)[6]) {
  double A[6][6], Lm[6][6];
  int k = 0;
  for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { A[r][c] = up[k]; A[c][r] = up[k]; ++k; }
  double dmax = 0.0;
  for (int r = 0; r < 6; ++r) dmax = fmax(dmax, A[r][r]);
  for (int j = 0; j < 6; ++j) {
    double piv = A[j][j];
    for (int m = 0; m < j; ++m) piv -= Lm[j][m] * Lm[j][m];
    if (!(piv > 1e-12 * dmax)) return false;
    const double l = sqrt(piv);
    Lm[j][j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int m = 0; m < j; ++m) s -= Lm[i][m] * Lm[j][m];
      Lm[i][j] = s / l;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) { double s = b[i]; for (int m = 0; m < i; ++m) s -= Lm[i][m] * y[m]; y[i] = s / Lm[i][i]; }
  for (int i = 5; i >= 0; --i) { double s = y[i]; for (int m = i + 1; m < 6; ++m) s -= Lm[m][i] * x[m]; x[i] = s / Lm[i][i]; }
  for (int i = 0; i < 6; ++i) if (!(fabs(x[i]) < (double)INFINITY)) return false;
  return true;
}

__global__ __launch_bounds__(256) void k_icp_solve(IcpArgs a, int pass) {
  __shared__ double red[8][ICP_ROW];
  double* S = a.state;
  if (S[ICP_S_DONE] != 0.0) return;
  const int t = threadIdx.x, col = t & (ICP_ROW - 1), seg = t / ICP_ROW;
  constexpr int SEG = ICP_BLOCKS / 8;
  double v = 0.0;
  for (int b = seg * SEG; b < (seg + 1) * SEG; ++b) v += a.partial[(int64_t)b * ICP_ROW + col];
  red[seg][col] = v;
  __syncthreads();
  if (t != 0) return;
  double sum[ICP_SUMS];
  for (int s = 0; s < ICP_SUMS; ++s) {
    double w = red[0][s];
    for (int j = 1; j < 8; ++j) w += red[j][s];
    sum[s] = w;
    S[ICP_S_SUMS + s] = w;
  }
  const double count = sum[28];
  const double fitness = count / (double)a.N, rmse = count > 0.0 ? sqrt(sum[27] / count) : 0.0;
  const double fitness0 = S[ICP_S_FITNESS], rmse0 = S[ICP_S_RMSE];
  S[ICP_S_FITNESS] = fitness; S[ICP_S_RMSE] = rmse; S[ICP_S_ITER] = (double)pass;
  if (pass >= 1 && fabs(fitness - fitness0) < a.relative_fitness && fabs(rmse - rmse0) < a.relative_rmse) {
    S[ICP_S_CONV] = 1.0; S[ICP_S_DONE] = 1.0;
    return;
  }
  if (pass >= a.max_iteration) { S[ICP_S_DONE] = 1.0; return; }
  double b[6], x[6];
  for (int i = 0; i < 6; ++i) b[i] = -sum[21 + i];
  if (!(count > 0.0) || !icp_cholesky(sum, b, x)) return;           // identity update: T stays
  const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
  // U = Rz(x2) Ry(x1) Rx(x0), translation x3..x5
  const double U[3][4] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]},
                          {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]},
                          {-sb, cb * sa, cb * ca, x[5]}};
  double Tn[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double w = (U[r][0] * S[c] + U[r][1] * S[4 + c]) + U[r][2] * S[8 + c];
      if (c == 3) w += U[r][3];                                      // the last row of T is 0 0 0 1
      Tn[4 * r + c] = w;
    }
  for (int i = 0; i < 12; ++i) S[i] = Tn[i];
}

static void icp_layout(IcpArgs& a, WsArena& ws) {
  np_layout(a.np, ws);
  a.partial = ws.take<double>((int64_t)ICP_BLOCKS * ICP_ROW);
}
int64_t ngm_icp_point_to_plane_bytes(int64_t M, int64_t N) {
  (void)N;
  IcpArgs a = {};
  a.np.M = (int)M;
  return ws_bytes(icp_layout, a);
}
int ngm_launch_icp_point_to_plane(const float* source, int64_t N, const float* target, const float* target_normals, int64_t M,
                                  double threshold, int max_iteration, double relative_fitness, double relative_rmse, const double* init,
                                  double* state, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  IcpArgs a = {};
  a.np.refs = target; a.np.M = (int)M;
  a.np.bbox_blocks = (int)std::min<int64_t>((M + 255) / 256, NP_BBOX_BLOCKS);
  a.source = source; a.normals = target_normals; a.N = (int)N; a.max_iteration = max_iteration;
  a.threshold = threshold; a.relative_fitness = relative_fitness; a.relative_rmse = relative_rmse; a.state = state;
  WsArena ws(workspace);
  icp_layout(a, ws);
  if (!ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  IcpInit in;
  for (int i = 0; i < 16; ++i) in.t[i] = init ? init[i] : (i % 5 == 0 ? 1.0 : 0.0);
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, st, state, in);
  if (N == 0) return 0;
  np_build_grid(a.np, st);
  for (int pass = 0; pass <= max_iteration; ++pass) {
    hipLaunchKernelGGL(k_icp_accumulate, dim3(ICP_BLOCKS), dim3(ICP_T), 0, st, a);
    hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(256), 0, st, a, pass);
  }
  return 0;
}
