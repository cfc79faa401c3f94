// Culling a mesh on the device: the two device parts of mesh_culling._cull_mesh (mesh_culling.py:228-352).
//   depth rasteriser (mesh_culling.py:41-120: two pyrender depth renders with flipped winding, merged by minimum)
//     k_depth_fill   : every pixel := the bit pattern of +inf
//     k_mesh_depth   : one thread per (face, pose).  Pose -> world-to-camera (columns 1 and 2 negated, affine inverse by
//                      adjugate, as k_fields_repose), the three corners to camera space, the triangle clipped against
//                      z >= near (0, 3 or 4 corners: at most two triangles), projected, and every pixel centre of its
//                      bounding box that lies inside or on it (either winding) gets the perspective-correct camera z,
//                      minimum over all faces by an INTEGER atomicMin on the bit pattern of the positive float: the order
//                      of the faces does not matter, the map is bitwise deterministic.
//                      Load balance: a lane walks its own bounding box when that holds at most CULL_SMALL_PIXELS pixels
//                      (extracted meshes: triangles of a few pixels); the larger ones (ground-truth walls that fill the
//                      screen) are taken one at a time by the whole wave -- ballot, the triangle broadcast from its lane,
//                      8 x 8 pixel tiles of its box strided over the 64 lanes.  No queue, no workspace, no counters.
//                      A mesh of few faces is drawn in bands of rows over blockIdx.z, so that its screen-filling
//                      triangles are shared by many workgroups and not walked by one wave.
//     k_depth_finish : pixels nothing was drawn to := 0.0
//   visibility (mesh_culling.py:143-225: _cull_from_one_pose and the accumulation of _apply_culling_strategy)
//     k_mesh_visibility : one thread per vertex, all poses of the call; the inverted poses of 64 poses at a time are staged
//                      in LDS by the first wave.  The thread owns its vertex: one plain add to each counter, no atomics.
// Plain C++ and vector stores only.  Every index that reaches memory is checked (face indices against V) or clamped
// (pixel boxes to the image; the visibility kernel reads a pixel only for a vertex it found inside the image).
#include "ngm_device.h"
#include "ngm_launch.h"

#include <algorithm>

#pragma clang fp contract(off)

constexpr int CULL_SMALL_PIXELS = 32;                 // bounding boxes of up to this many pixels stay with their lane
constexpr unsigned CULL_EMPTY = 0x7f800000u;          // +inf: above every depth that can be stored (z <= far, finite)

struct CullCam { int W, H; float fx, fy, cx, cy; };

__device__ __forceinline__ bool cull_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// World-to-camera of one OpenGL camera-to-world pose (row-major 4 x 4): w[4 r + c], c = 3 the translation.  Columns 1 and 2
// of the rotation are negated first (mesh_culling.py:164-167), the affine part is inverted by adjugate and determinant --
// no orthonormality assumed.  false: the pose has a non-finite entry (it then contributes nothing anywhere).  A singular
// pose gives non-finite rows, which no comparison downstream accepts.
__device__ __forceinline__ bool cull_w2c(const float* c, float (&w)[12]) {
  float m[16];
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) { m[i] = c[i]; fin = fin && cull_finite(m[i]); }
  const float r00 = m[0], r01 = -m[1], r02 = -m[2], r10 = m[4], r11 = -m[5], r12 = -m[6], r20 = m[8], r21 = -m[9], r22 = -m[10];
  const float c00 = r11 * r22 - r12 * r21, c01 = r12 * r20 - r10 * r22, c02 = r10 * r21 - r11 * r20;
  const float det = r00 * c00 + r01 * c01 + r02 * c02;
  w[0] = c00 / det;  w[1] = (r02 * r21 - r01 * r22) / det;  w[2] = (r01 * r12 - r02 * r11) / det;
  w[4] = c01 / det;  w[5] = (r00 * r22 - r02 * r20) / det;  w[6] = (r02 * r10 - r00 * r12) / det;
  w[8] = c02 / det;  w[9] = (r01 * r20 - r00 * r21) / det;  w[10] = (r00 * r11 - r01 * r10) / det;
  const float tx = m[3], ty = m[7], tz = m[11];
  w[3] = -(w[0] * tx + w[1] * ty + w[2] * tz);
  w[7] = -(w[4] * tx + w[5] * ty + w[6] * tz);
  w[11] = -(w[8] * tx + w[9] * ty + w[10] * tz);
  return fin;
}

__device__ __forceinline__ void cull_to_camera(const float (&w)[12], float x, float y, float z, float (&o)[3]) {
  o[0] = (w[0] * x + w[1] * y + w[2] * z) + w[3];
  o[1] = (w[4] * x + w[5] * y + w[6] * z) + w[7];
  o[2] = (w[8] * x + w[9] * y + w[10] * z) + w[11];
}

// ---- depth rasteriser -------------------------------------------------------------------------------------------------
struct DepthArgs {
  const float* verts; const int64_t* faces; const float* c2w;
  int64_t V; int F; int P;
  CullCam cam; float near, far;
  int band_rows;        // workgroups of blockIdx.z draw rows [z band_rows, (z + 1) band_rows) only (launcher: few faces, many rows)
  unsigned* depth;      // (P, H, W): bit patterns while the faces are drawn, floats after k_depth_finish
};

// a projected triangle: corners in pixels, 1 / z per corner, the pixels whose centres its bounding box holds (inclusive)
struct ScreenTri { float x[3], y[3], iz[3]; int u0, u1, v0, v1; };

__global__ __launch_bounds__(256) void k_depth_fill(unsigned* depth, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) depth[i] = CULL_EMPTY;
}
__global__ __launch_bounds__(256) void k_depth_finish(unsigned* depth, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (depth[i] == CULL_EMPTY) depth[i] = 0u;
}

// corners k0, k1, k2 of the clipped polygon -> t; false for a triangle with no projected area, a projection that is not
// finite in fp32, or a bounding box that holds no pixel centre of the image
__device__ __forceinline__ bool cull_screen_tri(const CullCam& cam, int row_lo, int row_hi, const float (&sx)[4], const float (&sy)[4],
                                                const float (&sz)[4], int k0, int k1, int k2, ScreenTri& t) {
  const int k[3] = {k0, k1, k2};
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t.x[i] = sx[k[i]]; t.y[i] = sy[k[i]]; t.iz[i] = 1.0f / sz[k[i]];
    fin = fin && cull_finite(t.x[i]) && cull_finite(t.y[i]) && cull_finite(t.iz[i]);
  }
  if (!fin) return false;
  const float area2 = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
  if (!(area2 != 0.f)) return false;
  const float xlo = fminf(fminf(t.x[0], t.x[1]), t.x[2]), xhi = fmaxf(fmaxf(t.x[0], t.x[1]), t.x[2]);
  const float ylo = fminf(fminf(t.y[0], t.y[1]), t.y[2]), yhi = fmaxf(fmaxf(t.y[0], t.y[1]), t.y[2]);
  // pixel u is sampled at u + 0.5: u >= lo - 0.5, u <= hi - 0.5; clamped as floats first, so no value beyond int is converted
  t.u0 = (int)fminf(fmaxf(ceilf(xlo - 0.5f), 0.f), (float)cam.W);
  t.u1 = (int)fminf(fmaxf(floorf(xhi - 0.5f), -1.f), (float)(cam.W - 1));
  t.v0 = (int)fminf(fmaxf(ceilf(ylo - 0.5f), 0.f), (float)cam.H);
  t.v1 = (int)fminf(fmaxf(floorf(yhi - 0.5f), -1.f), (float)(cam.H - 1));
  t.v0 = max(t.v0, row_lo); t.v1 = min(t.v1, row_hi);                  // this workgroup's band of rows
  return t.u0 <= t.u1 && t.v0 <= t.v1;
}

// One sample: pixel (u, v) of `img` (inside the image by construction of the boxes) against triangle t.  The same
// arithmetic whichever lane runs it, so the small and the large path store the same bits.
__device__ __forceinline__ void cull_sample(const ScreenTri& t, int u, int v, float far, unsigned* img, int W) {
  const float px = (float)u + 0.5f, py = (float)v + 0.5f;
  const float w0 = (t.x[2] - t.x[1]) * (py - t.y[1]) - (t.y[2] - t.y[1]) * (px - t.x[1]);
  const float w1 = (t.x[0] - t.x[2]) * (py - t.y[2]) - (t.y[0] - t.y[2]) * (px - t.x[2]);
  const float w2 = (t.x[1] - t.x[0]) * (py - t.y[0]) - (t.y[1] - t.y[0]) * (px - t.x[0]);
  const bool inside = (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f) || (w0 <= 0.f && w1 <= 0.f && w2 <= 0.f);
  if (!inside) return;
  // perspective-correct: 1 / z is linear on the screen
  const float z = ((w0 + w1) + w2) / ((w0 * t.iz[0] + w1 * t.iz[1]) + w2 * t.iz[2]);
  if (!(z > 0.f) || !(z <= far)) return;
  atomicMin(&img[(int64_t)v * W + u], __float_as_uint(z));
}

// face corners `p` (world) under world-to-camera `w` -> up to two screen triangles; bit t of the result: tri[t] is to be drawn
__device__ __forceinline__ int cull_face_setup(const CullCam& cam, int row_lo, int row_hi, float near, const float (&w)[12],
                                               const float (&p)[3][3], ScreenTri (&tri)[2]) {
  float c[3][3];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    cull_to_camera(w, p[k][0], p[k][1], p[k][2], c[k]);
    fin = fin && cull_finite(c[k][0]) && cull_finite(c[k][1]) && cull_finite(c[k][2]);
  }
  if (!fin) return 0;
  // clip against z >= near: walk the edges i -> j, keep corners in front, add the crossing where the side changes; the
  // crossing is always formed from the corner in front towards the one behind, whichever way the edge is walked.  The side
  // changes twice or not at all, so there are 0, 3 or 4 corners.  Slots are chosen by compares, not by an index: registers.
  float qx[4] = {0.f, 0.f, 0.f, 0.f}, qy[4] = {0.f, 0.f, 0.f, 0.f}, qz[4] = {1.f, 1.f, 1.f, 1.f};
  int n = 0;
  auto put = [&](float X, float Y, float Z) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (n == k) { qx[k] = X; qy[k] = Y; qz[k] = Z; }
    ++n;
  };
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3;
    const bool in_i = c[i][2] >= near, in_j = c[j][2] >= near;
    if (in_i) put(c[i][0], c[i][1], c[i][2]);
    if (in_i != in_j) {
      const float ax = in_i ? c[i][0] : c[j][0], ay = in_i ? c[i][1] : c[j][1], az = in_i ? c[i][2] : c[j][2];
      const float bx = in_i ? c[j][0] : c[i][0], by = in_i ? c[j][1] : c[i][1], bz = in_i ? c[j][2] : c[i][2];
      const float s = (az - near) / (az - bz);
      put(ax + s * (bx - ax), ay + s * (by - ay), near);
    }
  }
  if (n < 3) return 0;
  float sx[4], sy[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { sx[i] = (cam.fx * qx[i]) / qz[i] + cam.cx; sy[i] = (cam.fy * qy[i]) / qz[i] + cam.cy; }
  int ok = cull_screen_tri(cam, row_lo, row_hi, sx, sy, qz, 0, 1, 2, tri[0]) ? 1 : 0;
  if (n == 4 && cull_screen_tri(cam, row_lo, row_hi, sx, sy, qz, 0, 2, 3, tri[1])) ok |= 2;
  return ok;
}

__global__ __launch_bounds__(256) void k_mesh_depth(DepthArgs a) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t HW = (int64_t)a.cam.H * a.cam.W;
  const int row_lo = (int)min((int64_t)blockIdx.z * a.band_rows, (int64_t)a.cam.H);
  const int row_hi = (int)min((int64_t)row_lo + a.band_rows, (int64_t)a.cam.H) - 1;
  // the face's corners, once for all poses of this thread; not ok: an index outside [0, V) or a non-finite coordinate
  float p[3][3];
  bool face_ok = f < a.F;
  if (face_ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t i = a.faces[3 * f + k];
      if (i < 0 || i >= a.V) { face_ok = false; p[k][0] = p[k][1] = p[k][2] = 0.f; continue; }
#pragma unroll
      for (int d = 0; d < 3; ++d) { p[k][d] = a.verts[3 * i + d]; face_ok = face_ok && cull_finite(p[k][d]); }
    }
  }
  // every lane stays in the loop (the wave works together below); the pose is the same for the whole workgroup
  for (int pose = blockIdx.y; pose < a.P; pose += gridDim.y) {
    float w[12];
    if (!cull_w2c(a.c2w + 16 * (int64_t)pose, w)) continue;
    unsigned* img = a.depth + (int64_t)pose * HW;
    ScreenTri tri[2];
    const int drawn = face_ok ? cull_face_setup(a.cam, row_lo, row_hi, a.near, w, p, tri) : 0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const ScreenTri& s = tri[t];
      const bool have = (drawn >> t) & 1;
      const bool large = have && (int64_t)(s.u1 - s.u0 + 1) * (s.v1 - s.v0 + 1) > CULL_SMALL_PIXELS;
      if (have && !large)
        for (int v = s.v0; v <= s.v1; ++v)
          for (int u = s.u0; u <= s.u1; ++u) cull_sample(s, u, v, a.far, img, a.cam.W);
      unsigned long long todo = __ballot(large);
#ifdef NGM_CULL_SKIP_LARGE                        // measurement builds only (tools/mesh_cull_bench.py --skip-large-lib): what the shared path costs
      todo = 0;
#endif
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        ScreenTri b;
#pragma unroll
        for (int k = 0; k < 3; ++k) { b.x[k] = __shfl(s.x[k], src); b.y[k] = __shfl(s.y[k], src); b.iz[k] = __shfl(s.iz[k], src); }
        b.u0 = __shfl(s.u0, src); b.u1 = __shfl(s.u1, src); b.v0 = __shfl(s.v0, src); b.v1 = __shfl(s.v1, src);
        for (int ty = b.v0; ty <= b.v1; ty += 8)
          for (int tx = b.u0; tx <= b.u1; tx += 8) {
            const int u = tx + (lane & 7), v = ty + (lane >> 3);
            if (u <= b.u1 && v <= b.v1) cull_sample(b, u, v, a.far, img, a.cam.W);
          }
      }
    }
  }
}

int ngm_launch_mesh_depth(const float* verts, int64_t V, const int64_t* faces, int64_t F, const float* c2w, int64_t P, int W, int H,
                          float fx, float fy, float cx, float cy, float near, float far, float* depth, hipStream_t st) {
  DepthArgs a = {};
  a.verts = verts; a.faces = faces; a.c2w = c2w; a.V = V; a.F = (int)F; a.P = (int)P;
  a.cam = {W, H, fx, fy, cx, cy}; a.near = near; a.far = far; a.depth = reinterpret_cast<unsigned*>(depth);
  const int64_t n = P * (int64_t)H * W;
  const unsigned fill_blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 16384);
  hipLaunchKernelGGL(k_depth_fill, dim3(fill_blocks), dim3(256), 0, st, a.depth, n);
  // A mesh of few faces (a ground truth of two triangles per wall) gives few workgroups, and each of its triangles is a whole
  // screen for one wave to walk: the rows are then split into bands of a multiple of 8 over blockIdx.z, until there are about
  // 2048 workgroups.  A large mesh keeps one band: every band repeats the set-up of every face.
  const int64_t fb = (F + 255) / 256, py = std::min<int64_t>(P, 65535);
  int64_t bands = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(2048 / std::max<int64_t>(fb * py, 1), ((int64_t)H + 7) / 8), 64));
  a.band_rows = (int)std::min<int64_t>((((int64_t)H + bands - 1) / bands + 7) / 8 * 8, 0x7ffffff8);
  bands = ((int64_t)H + a.band_rows - 1) / a.band_rows;
  if (F > 0) hipLaunchKernelGGL(k_mesh_depth, dim3((unsigned)fb, (unsigned)py, (unsigned)bands), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_depth_finish, dim3(fill_blocks), dim3(256), 0, st, a.depth, n);
  return 0;
}

// ---- visibility -------------------------------------------------------------------------------------------------------
struct VisArgs {
  const float* verts; const float* c2w; const float* depth;      // depth NULL: frustum only
  int64_t V; int P; int num_frustum_poses;
  CullCam cam; float eps;
  int32_t* in_frustum; int32_t* observed;
};
constexpr int VIS_POSES = 64;

// _cull_from_one_pose in fp32, decision by decision (mesh_culling.py:173-188): camera space, uvz = K @ camera space,
// pz = z + 1e-8, px = u / pz, py = v / pz; inside: 0 <= px <= width - 1, 0 <= py <= height - 1 (the reference's bound, kept
// as it is), pz > 0; pixel = clamp then truncate; observed: inside and pz < depth[v, u] + eps.
__global__ __launch_bounds__(256) void k_mesh_visibility(VisArgs a) {
  __shared__ float sw[VIS_POSES][13];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < a.V;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) { x = a.verts[3 * i]; y = a.verts[3 * i + 1]; z = a.verts[3 * i + 2]; }
  const float wmax = (float)(a.cam.W - 1), hmax = (float)(a.cam.H - 1);
  const int64_t HW = (int64_t)a.cam.H * a.cam.W;
  int nf = 0, no = 0;
  for (int base = 0; base < a.P; base += VIS_POSES) {
    const int cnt = min(VIS_POSES, a.P - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      float w[12];
      const bool ok = cull_w2c(a.c2w + 16 * (int64_t)(base + threadIdx.x), w);
#pragma unroll
      for (int k = 0; k < 12; ++k) sw[threadIdx.x][k] = w[k];
      sw[threadIdx.x][12] = ok ? 1.f : 0.f;
    }
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < cnt; ++j) {
      if (sw[j][12] == 0.f) continue;
      const float X = (sw[j][0] * x + sw[j][1] * y + sw[j][2] * z) + sw[j][3];
      const float Y = (sw[j][4] * x + sw[j][5] * y + sw[j][6] * z) + sw[j][7];
      const float Z = (sw[j][8] * x + sw[j][9] * y + sw[j][10] * z) + sw[j][11];
      const float pz = Z + 1e-8f;
      const float px = (a.cam.fx * X + a.cam.cx * Z) / pz;
      const float py = (a.cam.fy * Y + a.cam.cy * Z) / pz;
      const bool inside = 0.f <= px && px <= wmax && 0.f <= py && py <= hmax && pz > 0.f;
      if (!inside) continue;
      if (base + j < a.num_frustum_poses) ++nf;
      bool seen = true;
      if (a.depth) {
        const int u = (int)fminf(fmaxf(px, 0.f), wmax), v = (int)fminf(fmaxf(py, 0.f), hmax);
        seen = pz < a.depth[(int64_t)(base + j) * HW + (int64_t)v * a.cam.W + u] + a.eps;
      }
      if (seen) ++no;
    }
  }
  if (live) { a.in_frustum[i] += nf; a.observed[i] += no; }
}

int ngm_launch_mesh_visibility(const float* verts, int64_t V, const float* c2w, int64_t P, int W, int H, float fx, float fy, float cx,
                               float cy, const float* depth, float eps, int64_t num_frustum_poses, int32_t* in_frustum,
                               int32_t* observed, hipStream_t st) {
  VisArgs a = {};
  a.verts = verts; a.c2w = c2w; a.depth = depth; a.V = V; a.P = (int)P;
  a.num_frustum_poses = (int)std::min<int64_t>(num_frustum_poses, P);
  a.cam = {W, H, fx, fy, cx, cy}; a.eps = eps; a.in_frustum = in_frustum; a.observed = observed;
  hipLaunchKernelGGL(k_mesh_visibility, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, a);
  return 0;
}
