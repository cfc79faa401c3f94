// Training-target sampler, device part (NeuralGraphMap._sample_target_mv, rm.py:1259-1459).
// The random draws (field subsets, sphere offsets, keyframe ids, pixel uniforms) stay with the caller's
// torch generator, exactly as in the reference; these two kernels replace the ~40 small tensor ops between them:
//   k_target_visibility : which keyframes see which field (20 points on the field sphere projected into every
//                         keyframe, depth test against the keyframe's depth image) + the 2-D bounding box of
//                         the projections per (field, keyframe)                                  rm.py:1321-1392
//   k_target_rays       : per sampled ray: pixel inside the box, near/far from the field sphere, RGB-D target,
//                         ray distance of the depth, masks, termination target                  rm.py:1394-1459
// HBM-bound gathers; one thread per (field, keyframe) resp. per ray.
#include "ngm_device.h"
#include "ngm_launch.h"
#include "ngm_workspace.h"

#pragma clang fp contract(off)

struct Cam3 { float x, y, z; };

// p_c = R^T (p_w - t)  (utils.transform_points(..., inv=True), utils.py:279-282), T row-major 4x4
__device__ __forceinline__ Cam3 world_to_cam(const float* T, float px, float py, float pz) {
  const float dx = px - T[3], dy = py - T[7], dz = pz - T[11];
  Cam3 c;
  c.x = T[0] * dx + T[4] * dy + T[8] * dz;
  c.y = T[1] * dx + T[5] * dy + T[9] * dz;
  c.z = T[2] * dx + T[6] * dy + T[10] * dz;
  return c;
}

// One (field, keyframe) pair of rm.py:1321-1392: does keyframe c see the field at (px, py, pz)?  *box = the projected sphere
// samples' 2-D bounding box, clamped to the image.  Shared by k_target_visibility and the device sampler's k_tsmv_visibility,
// so the two give the same bits by construction.
__device__ __forceinline__ bool target_visibility_one(const ngm_keyframes& kf, int c, float px, float py, float pz, int num_offsets,
                                                      const float* __restrict__ offsets, float radius, float4* box) {
  const float* T = kf.c2ws + 16 * (int64_t)c;
  const float* img = kf.rgbd + kf.frame_to_store[c] * (int64_t)kf.height * kf.width * 4;
  // Camera.project_points(points, "opengl") with the default pixel centre 0.5 (camera.py:119-154,176-180)
  const float cxp = kf.cx + 0.5f, cyp = kf.cy + 0.5f;
  bool in_front = false, in_front_depth = false, in_frustum = false;
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  for (int s = 0; s < num_offsets; ++s) {
    const float wx = px + offsets[3 * s] * radius * 1.0f, wy = py + offsets[3 * s + 1] * radius * 1.0f,
                wz = pz + offsets[3 * s + 2] * radius * 1.0f;
    const Cam3 p = world_to_cam(T, wx, wy, wz);
    const float depth = -p.z;
    const float xh = kf.fx * p.x + (-cxp) * p.z, yh = (-kf.fy) * p.y + (-cyp) * p.z, zh = -p.z;
    const float X = xh / zh, Y = yh / zh;
    const int xi = (int)X, yi = (int)Y;                            // .int(): truncation towards zero (rm.py:1337)
    const bool valid = xi >= 0 && xi < kf.width && yi >= 0 && yi < kf.height;
    const float kd = valid ? img[((int64_t)yi * kf.width + xi) * 4 + 3] : 0.f;
    in_front |= depth > 0.f;
    in_front_depth |= depth < kd;
    in_frustum |= valid;
    mnx = fminf(mnx, X); mny = fminf(mny, Y); mxx = fmaxf(mxx, X); mxy = fmaxf(mxy, Y);
  }
  // boxes are stored clamped to the image as the reference does before gathering them (rm.py:1388-1392)
  *box = make_float4(fmaxf(mnx, 0.f), fmaxf(mny, 0.f), fminf(mxx, (float)kf.width), fminf(mxy, (float)kf.height));
  return in_front && in_front_depth && in_frustum;
}

__global__ void k_target_visibility(ngm_keyframes kf, int F, const float* __restrict__ field_pos, int num_offsets,
                                    const float* __restrict__ offsets, float radius, uint8_t* __restrict__ kf_mask,
                                    float* __restrict__ bbox) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= F * kf.num_frames) return;
  const int f = idx / kf.num_frames, c = idx - f * kf.num_frames;
  float4 box;
  const bool seen = target_visibility_one(kf, c, field_pos[3 * f], field_pos[3 * f + 1], field_pos[3 * f + 2], num_offsets, offsets,
                                          radius, &box);
  kf_mask[idx] = seen ? 1 : 0;
  reinterpret_cast<float4*>(bbox)[idx] = box;
}

// One ray of rm.py:1394-1459: keyframe c, pixel uniforms (ux, uy) inside the box bb -> output row `idx` of o.  Shared by
// k_target_rays and the device sampler's k_tsmv_rays.
__device__ __forceinline__ void target_ray_one(const ngm_keyframes& kf, float fpx, float fpy, float fpz, float radius, float4 bb,
                                               int64_t c, float ux, float uy, const ngm_target_out& o, int64_t idx) {
  const float x = (bb.z - bb.x) * ux + bb.x, y = (bb.w - bb.y) * uy + bb.y;          // rm.py:1400-1402
  int j = min((int)x, kf.width - 1), i = min((int)y, kf.height - 1);                 // rm.py:1403-1407
  // (a negative index can only come from a keyframe that does not see the field; torch would wrap it around)
  const int jc = max(j, 0), ic = max(i, 0);
  const float* T = kf.c2ws + 16 * c;
  if (o.c2ws) {
    float4* dst = reinterpret_cast<float4*>(o.c2ws + 16 * idx);
    const float4* src = reinterpret_cast<const float4*>(T);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
  }
  o.ijs[2 * idx] = i; o.ijs[2 * idx + 1] = j;
  const Cam3 pc = world_to_cam(T, fpx, fpy, fpz);
  // ijs_to_directions, OpenGL (camera.py:186-203) and the OpenCV z component for depth_to_distance (:339-340)
  const float dx = ((float)j - kf.cx) / kf.fx, dy = ((float)i - kf.cy) / kf.fy;
  const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + 1.0f), 1e-12f);
  const float gx = dx / nrm, gy = (-dy) / nrm, gz = -1.0f / nrm;
  const float center = pc.x * gx + pc.y * gy + pc.z * gz;
  const float nearv = fmaxf(center - radius, 0.f), farv = fmaxf(center + radius, 0.f);
  const float4 px = reinterpret_cast<const float4*>(kf.rgbd)[(kf.frame_to_store[c] * kf.height + ic) * (int64_t)kf.width + jc];
  const float gt = px.w / (1.0f / nrm);
  const bool vd = gt != 0.0f;
  o.near[idx] = nearv; o.far[idx] = farv; o.gt[idx] = gt;
  reinterpret_cast<float4*>(o.rgbds)[idx] = px;
  o.rgb_mask[idx] = (px.x != 0.f || px.y != 0.f) ? 1 : 0;
  o.depth_mask[idx] = (gt > nearv && gt < farv && vd) ? 1 : 0;
  o.term_probs[idx] = (gt < farv) ? 1.0f : 0.0f;
  o.term_mask[idx] = (gt > nearv && vd) ? 1 : 0;
}

__global__ void k_target_rays(ngm_keyframes kf, int F, int R, const float* __restrict__ field_pos, float radius,
                              const float* __restrict__ bbox, const int64_t* __restrict__ frame_cids,
                              const float* __restrict__ u_xy, ngm_target_out o) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)F * R) return;
  const int f = (int)(idx / R);
  const int64_t c = frame_cids[idx];
  const float4 bb = reinterpret_cast<const float4*>(bbox)[(int64_t)f * kf.num_frames + c];
  target_ray_one(kf, field_pos[3 * f], field_pos[3 * f + 1], field_pos[3 * f + 2], radius, bb, c, u_xy[2 * idx], u_xy[2 * idx + 1], o,
                 idx);
}

// ---- single-view variant (NeuralGraphMap._sample_target_sv, rm.py:1461-1583) ------------------------------------
// k_target_sv_intersect: does the segment camera origin -> back-projected depth point n pass through the sphere of field f?
//   geometry.LineSegments.closest_points / intersects_spheres (geometry.py:67-105) with p1 = 0: t = clamp(c.p / |p|^2, 0, 1)
//   (|p|^2 == 0 -> 1), closest = p t, hit = |c - closest|^2 <= r^2.  One thread per (field, point); 50 000 points x up
//   to a few hundred fields of byte output: HBM-bound.
// the one segment-sphere test of the single-view samplers (r2 = radius * radius)
__device__ __forceinline__ bool target_sv_hit(float cx, float cy, float cz, float px, float py, float pz, float r2) {
  float sq = (px * px + py * py) + pz * pz;
  if (sq == 0.0f) sq = 1.0f;
  const float t = fminf(fmaxf(((cx * px + cy * py) + cz * pz) / sq, 0.0f), 1.0f);
  const float ex = cx - px * t, ey = cy - py * t, ez = cz - pz * t;
  return (ex * ex + ey * ey) + ez * ez <= r2;
}
__global__ void k_target_sv_intersect(int F, int64_t N, const float* __restrict__ pos_c, const float* __restrict__ points, float radius,
                                      uint8_t* __restrict__ hit) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int f = blockIdx.y;
  if (n >= N) return;
  const float px = points[3 * n], py = points[3 * n + 1], pz = points[3 * n + 2];
  const float cx = pos_c[3 * f], cy = pos_c[3 * f + 1], cz = pos_c[3 * f + 2];
  hit[(int64_t)f * N + n] = target_sv_hit(cx, cy, cz, px, py, pz, radius * radius) ? 1 : 0;
}
// One ray of rm.py:1536-1561: pixel (i, j) of `image` against the field centre (pcx, pcy, pcz) in the camera frame -> output
// row `idx` of o.  Shared by k_target_sv_rays and the device sampler's k_tssv_rows.
__device__ __forceinline__ void target_sv_ray_one(float pcx, float pcy, float pcz, float radius, int64_t i, int64_t j,
                                                  const float* __restrict__ image, int width, float fx, float fy, float cx, float cy,
                                                  const ngm_target_out& o, int64_t idx) {
  o.ijs[2 * idx] = i; o.ijs[2 * idx + 1] = j;
  const float dx = ((float)j - cx) / fx, dy = ((float)i - cy) / fy;
  const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + 1.0f), 1e-12f);
  const float gx = dx / nrm, gy = (-dy) / nrm, gz = -1.0f / nrm;
  const float center = pcx * gx + pcy * gy + pcz * gz;
  const float nearv = center - radius, farv = center + radius;
  const float4 px = reinterpret_cast<const float4*>(image)[i * (int64_t)width + j];
  const float gt = px.w / (1.0f / nrm);
  const bool dm = gt < farv;
  o.near[idx] = nearv; o.far[idx] = farv; o.gt[idx] = gt;
  reinterpret_cast<float4*>(o.rgbds)[idx] = px;
  o.rgb_mask[idx] = dm ? 1 : 0;
  o.depth_mask[idx] = dm ? 1 : 0;
  o.term_probs[idx] = dm ? 1.0f : 0.0f;
  o.term_mask[idx] = 1;
}
// k_target_sv_rays: per sampled segment: pixel, direction, near / far from the field sphere (NOT clamped at 0 here,
// rm.py:1543-1544), RGB-D target, ray distance of the depth, masks (rm.py:1536-1561)
__global__ void k_target_sv_rays(int F, int R, const float* __restrict__ pos_c, float radius, const int64_t* __restrict__ pts_ijs,
                                 const int64_t* __restrict__ segments, const float* __restrict__ image, int height, int width,
                                 float fx, float fy, float cx, float cy, ngm_target_out o) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)F * R) return;
  const int f = (int)(idx / R);
  const int64_t sgm = segments[idx];
  const int64_t i = pts_ijs[2 * sgm], j = pts_ijs[2 * sgm + 1];
  target_sv_ray_one(pos_c[3 * f], pos_c[3 * f + 1], pos_c[3 * f + 2], radius, i, j, image, width, fx, fy, cx, cy, o, idx);
  (void)height;
}
int ngm_launch_target_sv_intersect(int F, int64_t N, const float* pos_c, const float* points, float radius, uint8_t* hit, hipStream_t st) {
  hipLaunchKernelGGL(k_target_sv_intersect, dim3((unsigned)((N + 255) / 256), (unsigned)F), dim3(256), 0, st, F, N, pos_c, points, radius, hit);
  return 0;
}
int ngm_launch_target_sv_rays(int F, int R, const float* pos_c, float radius, const int64_t* pts_ijs, const int64_t* segments,
                              const float* image, int height, int width, float fx, float fy, float cx, float cy, const ngm_target_out& o,
                              hipStream_t st) {
  const int64_t n = (int64_t)F * R;
  hipLaunchKernelGGL(k_target_sv_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, F, R, pos_c, radius, pts_ijs, segments, image,
                     height, width, fx, fy, cx, cy, o);
  return 0;
}

int ngm_launch_target_visibility(const ngm_keyframes& kf, int F, const float* field_pos, int num_offsets, const float* offsets,
                                 float radius, uint8_t* kf_mask, float* bbox, hipStream_t st) {
  const int n = F * kf.num_frames;
  hipLaunchKernelGGL(k_target_visibility, dim3((n + 127) / 128), dim3(128), 0, st, kf, F, field_pos, num_offsets, offsets, radius,
                     kf_mask, bbox);
  return 0;
}
int ngm_launch_target_rays(const ngm_keyframes& kf, int F, int R, const float* field_pos, float radius, const float* bbox,
                           const int64_t* frame_cids, const float* u_xy, const ngm_target_out& o, hipStream_t st) {
  const int64_t n = (int64_t)F * R;
  hipLaunchKernelGGL(k_target_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kf, F, R, field_pos, radius, bbox,
                     frame_cids, u_xy, o);
  return 0;
}

// ---- the whole sampler on the device (ngm_target_sample_mv, include/ngm_hip.h) -----------------------------------------
// Three launches, no host synchronisation:
//   k_tsmv_draw       one workgroup: iteration (explicit or read from the device counter, which it advances), both field
//                     subsets (k smallest of unique 64-bit keys by an MSB-first radix select), their union, the owner filter,
//                     the 20 sphere offsets, the field centres gathered from the map
//   k_tsmv_visibility one thread per (slot, keyframe): target_visibility_one + a "some keyframe sees it" flag per slot
//   k_tsmv_rays       one workgroup per (slot, ray chunk): the slot's output row (scan over the flags), the field's visible
//                     keyframes in ascending frame id (ballot + prefix, in LDS; a workspace list past TSMV_LDS_FRAMES), the
//                     ray draws and target_ray_one; invisible slots write the padding rows
constexpr uint32_t TSMV_STREAM_OBS = 0x54470001u, TSMV_STREAM_RAND = 0x54470002u, TSMV_STREAM_OFFSETS = 0x54470003u,
                   TSMV_STREAM_RAYS = 0x54470004u;
constexpr uint64_t TSMV_EXCLUDED = ~0ull;        // never a real key: the low word of one is a position / field id < 2^31
constexpr int TSMV_DRAW_THREADS = 1024, TSMV_RAY_THREADS = 256, TSMV_LDS_FRAMES = 2048, TSMV_NUM_OFFSETS = 20;

struct tsmv_ws {
  int64_t* hdr;        // [0] iteration of this call, [1] owned fields drawn (slots in use)
  uint64_t* keys;      // max(num_current, num_fields)
  int64_t* slot_ids;   // capacity
  float* slot_pos;     // capacity x 3
  int* flags;          // capacity: some keyframe sees the slot's field
  float* offsets;      // 20 x 3
  uint8_t* kf_mask;    // capacity x num_frames
  float4* bbox;        // capacity x num_frames
  int* list;           // capacity x num_frames visible-keyframe lists, only when num_frames > TSMV_LDS_FRAMES
};

static tsmv_ws tsmv_layout(int num_frames, int num_current, int num_fields, int capacity, WsArena& ws) {
  const int64_t pairs = (int64_t)capacity * num_frames;
  tsmv_ws t;
  t.hdr = ws.take<int64_t>(2);
  t.keys = ws.take<uint64_t>(num_current > num_fields ? num_current : num_fields);
  t.slot_ids = ws.take<int64_t>(capacity);
  t.slot_pos = ws.take<float>((int64_t)capacity * 3);
  t.flags = ws.take<int>(capacity);
  t.offsets = ws.take<float>(TSMV_NUM_OFFSETS * 3);
  t.kf_mask = ws.take<uint8_t>(pairs);
  t.bbox = ws.take<float4>(pairs);
  t.list = num_frames > TSMV_LDS_FRAMES ? ws.take<int>(pairs) : nullptr;
  return t;
}

// Exact-rounding stand-ins for logf / sincosf (only +, -, *, / and bit operations, fp contraction off): the host restates the
// offsets bit for bit with numpy float32 (tests/test_gpu_target_device.py).  Series truncation errors < 1e-7.
__device__ __forceinline__ float tsmv_log(float u) {                     // u > 0, normal
  const uint32_t b = __float_as_uint(u);
  const float e = (float)((int)((b >> 23) & 255u) - 127);
  const float m = __uint_as_float((b & 0x7FFFFFu) | 0x3F800000u);        // [1, 2)
  const float s = (m - 1.0f) / (m + 1.0f), z = s * s;                    // log m = 2 atanh(s), s in [0, 1/3)
  float p = 0.0769230798f;                                                // 1/13
  p = p * z + 0.0909090936f; p = p * z + 0.111111112f; p = p * z + 0.142857149f; p = p * z + 0.200000003f;
  p = p * z + 0.333333343f; p = p * z + 1.0f;
  return e * 0.693147182f + 2.0f * s * p;
}
__device__ __forceinline__ void tsmv_sincos_2pi(float u, float* sn, float* cs) {   // u in [0, 1): sin / cos of 2 pi u
  const float u4 = u * 4.0f;
  const int q = (int)u4;
  const float ph = (u4 - (float)q) * 1.57079637f, z = ph * ph;           // [0, pi/2)
  float ps = 1.60590444e-10f;                                             // 1/13!
  ps = ps * z - 2.50521079e-08f; ps = ps * z + 2.75573188e-06f; ps = ps * z - 1.98412701e-04f; ps = ps * z + 8.33333377e-03f;
  ps = ps * z - 0.166666672f; ps = ps * z + 1.0f;
  float pc = 2.08767570e-09f;                                             // 1/12!
  pc = pc * z - 2.75573188e-07f; pc = pc * z + 2.48015876e-05f; pc = pc * z - 1.38888892e-03f; pc = pc * z + 4.16666679e-02f;
  pc = pc * z - 0.5f; pc = pc * z + 1.0f;
  const float s = ph * ps, c = pc;
  *sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
  *cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// The k smallest of keys[0..n) (TSMV_EXCLUDED skipped, the others unique), ascending, into out[0..k).  MSB-first radix select
// over 8-bit digits until the bin that holds the k-th key holds exactly the keys still wanted; then every key whose digits so
// far are <= the prefix is in, and a rank sort over the k orders them.  Block-uniform arguments; all threads must call.
__device__ void tsmv_k_smallest(const uint64_t* keys, int n, int k, uint64_t* out, uint64_t* scratch, int* hist, int* st) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (k <= 0) return;
  int shift = 64, rem = k;
  uint64_t prefix = 0;
  for (;;) {
    shift -= 8;
    for (int b = tid; b < 256; b += nt) hist[b] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
      const uint64_t key = keys[i];
      if (key == TSMV_EXCLUDED || (shift < 56 && (key >> (shift + 8)) != prefix)) continue;
      atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int cum = 0, b = 0;
      for (; b < 255; ++b) {
        if (cum + hist[b] >= rem) break;
        cum += hist[b];
      }
      st[0] = b; st[1] = rem - cum; st[2] = hist[b] == rem - cum;
    }
    __syncthreads();
    prefix = (prefix << 8) | (uint64_t)st[0];
    rem = st[1];
    const bool done = st[2] != 0 || shift == 0;
    __syncthreads();
    if (done) break;
  }
  if (tid == 0) st[3] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += nt) {
    const uint64_t key = keys[i];
    if (key != TSMV_EXCLUDED && (key >> shift) <= prefix) {
      const int p = atomicAdd(&st[3], 1);
      if (p < k) scratch[p] = key;
    }
  }
  __syncthreads();
  for (int i = tid; i < k; i += nt) {
    const uint64_t v = scratch[i];
    int r = 0;
    for (int j = 0; j < k; ++j) {
      const uint64_t u = scratch[j];
      r += (u < v || (u == v && j < i)) ? 1 : 0;
    }
    out[r] = v;
  }
  __syncthreads();
}

// The live variant (ngm_target_sample_mv_live): s.num_current / s.num_observed / s.num_random / kf.num_frames are the host's
// MAXIMA (strides, grids, workspace), the counts in force are read from device memory by every kernel.  LIVE = false is the
// code of ngm_target_sample_mv as it was: `lv` is not touched there.
struct tsmv_live {
  const int32_t* num_current;   // device: 0 <= * <= s.num_current (clamped)
  const int32_t* num_frames;    // device: 0 <= * <= kf.num_frames (clamped)
  int32_t* num_observed_out;    // device out (1)
  int32_t* num_random_out;      // device out (1)
  int num_train_fields;         // T
  const int32_t* num_fields;    // device, or NULL: the grow variant (ngm_target_sample_mv_grow), s.num_fields is the capacity then
};
template <bool LIVE>
__device__ __forceinline__ int tsmv_num_frames(const ngm_keyframes& kf, const tsmv_live& lv) {
  if (!LIVE) return kf.num_frames;
  return min(max(*lv.num_frames, 0), kf.num_frames);
}

template <bool LIVE>
__global__ __launch_bounds__(TSMV_DRAW_THREADS) void k_tsmv_draw(ngm_target_sample s, tsmv_ws w, tsmv_live lv) {
  __shared__ uint64_t sel[NGM_TARGET_MAX_DRAW], scratch[NGM_TARGET_MAX_DRAW];
  __shared__ int64_t drawn[NGM_TARGET_MAX_DRAW];
  __shared__ int hist[256], st[4];
  __shared__ int64_t s_iter;
  __shared__ int s_own;
  __shared__ float normals[3 * TSMV_NUM_OFFSETS];
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) {
    const int64_t it = s.iteration >= 0 ? s.iteration : *s.iteration_dev;
    s_iter = it;
    w.hdr[0] = it;
  }
  __syncthreads();
  const uint64_t it = (uint64_t)s_iter;
  if (tid == 0 && s.iteration < 0) *s.iteration_dev = (int64_t)it + 1;          // after the barrier: every read is done
  int num_current = s.num_current, n_obs = s.num_observed, n_rand = s.num_random;
  int num_fields = s.num_fields;                         // the fields in force; s.num_fields stays the stride of every array
  if (LIVE) {                                            // block-uniform: every thread reads the same word
    if (lv.num_fields) num_fields = min(max(*lv.num_fields, 0), s.num_fields);
    num_current = min(max(*lv.num_current, 0), min(s.num_current, num_fields));
    n_obs = min(lv.num_train_fields / 2, num_current);
    n_rand = max(min(lv.num_train_fields - n_obs, num_fields - n_obs), 0);
    if (tid == 0) { *lv.num_observed_out = n_obs; *lv.num_random_out = n_rand; }
    for (int i = n_obs + tid; i < s.num_observed; i += nt) s.subset_observed[i] = -1;
    for (int i = n_rand + tid; i < s.num_random; i += nt) s.subset_random[i] = -1;
  }
  const int n_all = n_obs + n_rand;
  // 1. observed fields: the n_obs smallest of (philox(id) << 32 | position), in key order = random order
  for (int j = tid; j < num_current; j += nt) {
    uint32_t q[4];
    philox_block(s.seed, it, (uint64_t)s.current_field_ids[j], TSMV_STREAM_OBS, q);
    w.keys[j] = ((uint64_t)q[0] << 32) | (uint32_t)j;
  }
  __syncthreads();
  tsmv_k_smallest(w.keys, num_current, n_obs, sel, scratch, hist, st);
  for (int i = tid; i < n_obs; i += nt) {
    const int64_t j = (int64_t)(sel[i] & 0xFFFFFFFFull);       // < num_current: the select returns exactly n_obs keys
    s.subset_observed[i] = j;
    drawn[i] = j < num_current ? s.current_field_ids[j] : -1;
  }
  __syncthreads();
  // 2. random fields: the n_rand smallest of (philox(f) << 32 | f) over the fields not drawn in 1.
  if (n_rand > 0) {
    for (int f = tid; f < num_fields; f += nt) {
      uint32_t q[4];
      philox_block(s.seed, it, (uint64_t)f, TSMV_STREAM_RAND, q);
      w.keys[f] = ((uint64_t)q[0] << 32) | (uint32_t)f;
    }
    __syncthreads();
    for (int i = tid; i < n_obs; i += nt) {
      const int64_t id = drawn[i];
      if (id >= 0 && id < num_fields) w.keys[id] = TSMV_EXCLUDED;
    }
    __syncthreads();
    tsmv_k_smallest(w.keys, num_fields, n_rand, sel, scratch, hist, st);
    for (int i = tid; i < n_rand; i += nt) {
      const int64_t id = (int64_t)(sel[i] & 0xFFFFFFFFull);
      s.subset_random[i] = id;
      drawn[n_obs + i] = id;
    }
    __syncthreads();
    // 3. the union sorted ascending (torch.unique)
    for (int i = tid; i < n_all; i += nt) {
      const int64_t v = drawn[i];
      int r = 0;
      for (int j = 0; j < n_all; ++j) {
        const int64_t u = drawn[j];
        r += (u < v || (u == v && j < i)) ? 1 : 0;
      }
      sel[r] = (uint64_t)v;
    }
    __syncthreads();
    for (int i = tid; i < n_all; i += nt) drawn[i] = (int64_t)sel[i];
    __syncthreads();
  }
  // 4. owner filter, order kept (ids outside [0, num_fields) dropped)
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < n_all; ++i) {
      const int64_t id = drawn[i];
      if (id >= 0 && id < num_fields && id % s.world_size == s.rank && n < s.capacity) scratch[n++] = (uint64_t)id;
    }
    s_own = n;
    w.hdr[1] = n;
    if (s.capacity == 0) *s.count = 0;                 // no k_tsmv_rays launch then
  }
  __syncthreads();
  const int n_own = s_own;
  for (int i = tid; i < s.capacity; i += nt) {
    w.flags[i] = 0;
    if (i < n_own) {
      const int64_t id = (int64_t)scratch[i];
      w.slot_ids[i] = id;
      w.slot_pos[3 * i] = s.field_positions[3 * id];
      w.slot_pos[3 * i + 1] = s.field_positions[3 * id + 1];
      w.slot_pos[3 * i + 2] = s.field_positions[3 * id + 2];
    }
  }
  // 5. sphere offsets: Box-Muller on 15 blocks (two pairs each), u1 = odd / 2^24 in (0, 1), then normalised
  if (tid < 3 * TSMV_NUM_OFFSETS / 2) {
    uint32_t q[4];
    philox_block(s.seed, it, (uint64_t)(tid >> 1), TSMV_STREAM_OFFSETS, q);
    const int h = 2 * (tid & 1);
    const float u1 = (float)((q[h] >> 9) * 2u + 1u) * (1.0f / 16777216.0f);
    const float u2 = philox_word_uniform(q[h + 1]);
    const float r = sqrtf(-2.0f * tsmv_log(u1));
    float sn, cs;
    tsmv_sincos_2pi(u2, &sn, &cs);
    normals[2 * tid] = r * cs;
    normals[2 * tid + 1] = r * sn;
  }
  __syncthreads();
  if (tid < TSMV_NUM_OFFSETS) {
    const float x = normals[3 * tid], y = normals[3 * tid + 1], z = normals[3 * tid + 2];
    const float n = sqrtf((x * x + y * y) + z * z);
    const float ox = x / n, oy = y / n, oz = z / n;
    w.offsets[3 * tid] = ox; w.offsets[3 * tid + 1] = oy; w.offsets[3 * tid + 2] = oz;
    s.offsets[3 * tid] = ox; s.offsets[3 * tid + 1] = oy; s.offsets[3 * tid + 2] = oz;
  }
}

template <bool LIVE>
__global__ void k_tsmv_visibility(ngm_keyframes kf, int capacity, float radius, tsmv_ws w, tsmv_live lv) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)capacity * kf.num_frames) return;
  const int slot = (int)(idx / kf.num_frames), c = (int)(idx - (int64_t)slot * kf.num_frames);
  if (slot >= (int)w.hdr[1]) return;
  if (LIVE && c >= tsmv_num_frames<true>(kf, lv)) return;          // kf.num_frames is the row stride there
  float4 box;
  const bool seen = target_visibility_one(kf, c, w.slot_pos[3 * slot], w.slot_pos[3 * slot + 1], w.slot_pos[3 * slot + 2],
                                          TSMV_NUM_OFFSETS, w.offsets, radius, &box);
  w.kf_mask[idx] = seen ? 1 : 0;
  w.bbox[idx] = box;
  if (seen) w.flags[slot] = 1;                       // every writer stores the same 1 (flags zeroed by k_tsmv_draw)
}

template <bool LIVE>
__global__ __launch_bounds__(TSMV_RAY_THREADS) void k_tsmv_rays(ngm_keyframes kf, ngm_target_sample s, ngm_target_out o, tsmv_ws w,
                                                                tsmv_live lv) {
  __shared__ int list[TSMV_LDS_FRAMES];
  __shared__ int red[2], wave_cnt[TSMV_RAY_THREADS / 64];
  const int slot = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_own = (int)w.hdr[1];
  const uint64_t it = (uint64_t)w.hdr[0];
  if (tid < 2) red[tid] = 0;
  __syncthreads();
  // output row: visible slots in order first (rows 0..count-1), then the others (padding rows count..capacity-1)
  int before = 0, total = 0;
  for (int i = tid; i < n_own; i += TSMV_RAY_THREADS) {
    const int f = w.flags[i];
    total += f;
    before += i < slot ? f : 0;
  }
  if (total) atomicAdd(&red[1], total);
  if (before) atomicAdd(&red[0], before);
  __syncthreads();
  const int count = red[1], vb = red[0];
  const bool vis = slot < n_own && w.flags[slot] != 0;
  const int row = vis ? vb : count + (slot - vb);
  const int R = s.num_rays, k = blockIdx.x * TSMV_RAY_THREADS + tid;
  if (blockIdx.x == 0 && tid == 0) {
    s.field_ids[row] = vis ? w.slot_ids[slot] : -1;
    if (slot == 0) *s.count = count;
  }
  if (!vis) {
    if (k < R) {
      const int64_t idx = (int64_t)row * R + k;
      if (o.c2ws) {
        float4* dst = reinterpret_cast<float4*>(o.c2ws + 16 * idx);
        dst[0] = dst[1] = dst[2] = dst[3] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      o.ijs[2 * idx] = 0; o.ijs[2 * idx + 1] = 0;
      o.near[idx] = 0.f; o.far[idx] = 0.f; o.gt[idx] = 0.f;
      reinterpret_cast<float4*>(o.rgbds)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
      o.rgb_mask[idx] = 0; o.depth_mask[idx] = 0; o.term_probs[idx] = 0.f; o.term_mask[idx] = 0;
      s.frame_cids[idx] = 0; s.u_xy[2 * idx] = 0.f; s.u_xy[2 * idx + 1] = 0.f;
    }
    return;
  }
  // the field's visible keyframes in ascending frame id (every block of the slot writes the same global list when it is used)
  const int stride = kf.num_frames, Nc = tsmv_num_frames<LIVE>(kf, lv);       // stride == Nc unless LIVE
  int* lst = stride <= TSMV_LDS_FRAMES ? list : w.list + (int64_t)slot * stride;
  const uint8_t* m = w.kf_mask + (int64_t)slot * stride;
  int base = 0;
  for (int c0 = 0; c0 < Nc; c0 += TSMV_RAY_THREADS) {
    const int c = c0 + tid;
    const bool on = c < Nc && m[c] != 0;
    const uint64_t bal = __ballot(on);
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int q = 0; q < TSMV_RAY_THREADS / 64; ++q) {
      off += q < wv ? wave_cnt[q] : 0;
      tot += wave_cnt[q];
    }
    if (on) lst[off + __popcll(bal & ((1ull << lane) - 1ull))] = c;
    base += tot;
    __syncthreads();
  }
  if (k >= R) return;
  const int64_t id = w.slot_ids[slot];
  uint32_t q[4];
  philox_block(s.seed, it, ((uint64_t)(uint32_t)id << 32) | (uint32_t)k, TSMV_STREAM_RAYS, q);
  const int c = lst[(int)(((uint64_t)q[0] * (uint64_t)base) >> 32)];
  const float ux = philox_word_uniform(q[1]), uy = philox_word_uniform(q[2]);
  const int64_t idx = (int64_t)row * R + k;
  s.frame_cids[idx] = c;
  s.u_xy[2 * idx] = ux; s.u_xy[2 * idx + 1] = uy;
  target_ray_one(kf, w.slot_pos[3 * slot], w.slot_pos[3 * slot + 1], w.slot_pos[3 * slot + 2], s.radius,
                 w.bbox[(int64_t)slot * stride + c], (int64_t)c, ux, uy, o, idx);
}

int64_t ngm_target_sample_mv_bytes(int num_frames, int num_current, int num_fields, int capacity) {
  return ws_bytes(tsmv_layout, num_frames, num_current, num_fields, capacity);
}
// live == nullptr: the sizes of kf / s are the counts in force.  Otherwise kf.num_frames = max_frames, s.num_current =
// max_current, s.num_observed / s.num_random = their maxima (include/ngm_hip.h) and the kernels read the counts from `live`.
template <bool LIVE>
static void tsmv_launch(const ngm_keyframes& kf, const ngm_target_sample& s, const tsmv_live& lv, const ngm_target_out& o,
                        const tsmv_ws& w, hipStream_t st) {
  hipLaunchKernelGGL(k_tsmv_draw<LIVE>, dim3(1), dim3(TSMV_DRAW_THREADS), 0, st, s, w, lv);
  if (s.capacity == 0) return;
  const int64_t pairs = (int64_t)s.capacity * kf.num_frames;
  hipLaunchKernelGGL(k_tsmv_visibility<LIVE>, dim3((unsigned)((pairs + 127) / 128)), dim3(128), 0, st, kf, s.capacity, s.radius, w, lv);
  hipLaunchKernelGGL(k_tsmv_rays<LIVE>, dim3((unsigned)((s.num_rays + TSMV_RAY_THREADS - 1) / TSMV_RAY_THREADS), (unsigned)s.capacity),
                     dim3(TSMV_RAY_THREADS), 0, st, kf, s, o, w, lv);
}
int ngm_launch_target_sample_mv(const ngm_keyframes& kf, const ngm_target_sample& s, const ngm_target_live* live,
                                const ngm_target_out& o, void* workspace, int64_t workspace_bytes, hipStream_t st,
                                const int32_t* num_fields_dev) {
  WsArena ws(workspace);
  const tsmv_ws w = tsmv_layout(kf.num_frames, s.num_current, s.num_fields, s.capacity, ws);
  if (!workspace || !ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  if (!live)
    tsmv_launch<false>(kf, s, tsmv_live{nullptr, nullptr, nullptr, nullptr, 0, nullptr}, o, w, st);
  else
    tsmv_launch<true>(kf, s, tsmv_live{live->num_current, live->num_frames, live->num_observed, live->num_random,
                                       live->num_train_fields, num_fields_dev}, o, w, st);
  return 0;
}

// ---- per-field training-iteration counts (rm.py:1188) -------------------------------------------------------------------
// training_iterations[field_ids[i]] += 1 for i < min(rows, *count); -1 (padding) and ids outside [0, num_fields) skipped.
__global__ void k_field_counts_add(const int64_t* __restrict__ field_ids, const int32_t* __restrict__ count, int rows, int num_fields,
                                   int64_t* __restrict__ training_iterations) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = count ? min(max(*count, 0), rows) : rows;
  if (i >= n) return;
  const int64_t id = field_ids[i];
  if (id < 0 || id >= num_fields) return;
  atomicAdd(reinterpret_cast<unsigned long long*>(training_iterations + id), 1ull);   // integer: order does not matter
}
int ngm_launch_field_counts_add(const int64_t* field_ids, const int32_t* count, int rows, int num_fields, int64_t* training_iterations,
                                hipStream_t st) {
  hipLaunchKernelGGL(k_field_counts_add, dim3((rows + 255) / 256), dim3(256), 0, st, field_ids, count, rows, num_fields,
                     training_iterations);
  return 0;
}

// ---- observed fields of one RGB-D frame (NeuralGraphMap._get_observed_fields, rm.py:1642-1670) ---------------------------
//   k_obs_keys     one thread per pixel (grid stride): key = (Philox word 0 of block ctr = pixel, stream ..05, offset = frame)
//                  << 32 | pixel for pixels with depth != 0, TSMV_EXCLUDED for the others; zeroes the histograms and counters
//   k_obs_hist x 8 MSB-first radix select of the num_points smallest keys over all workgroups: pass p histograms digit p of the
//                  keys that match the prefix so far (LDS histogram per workgroup, integer atomics into the global one).  Every
//                  workgroup derives the prefix from the finished histograms of the earlier passes itself, so there is no
//                  launch and no host read between passes; passes after the select is decided return at once
//   k_obs_collect  every key at or below the decided prefix takes a slot of `pixels` (integer atomic: the SET is
//                  deterministic, the order is not) -- or copies subset_in
//   k_obs_fields   one workgroup: back-projects the chosen pixels (LDS), their AABB, per field the AABB test and the
//                  origin -> point segment test against the field sphere (k_target_sv_intersect's arithmetic), then the
//                  observed ids ascending (ballot + prefix), -1 past the count; advances the frame counter
constexpr uint32_t TSMV_STREAM_PIXELS = 0x54470005u;
constexpr int OBS_THREADS = 256, OBS_MAX_BLOCKS = 1024, OBS_FIELD_THREADS = 1024, OBS_PASSES = 8;

struct obs_ws {
  uint64_t* keys;     // H x W
  int* hist;          // OBS_PASSES x 256
  int* counters;      // [0] slots handed out by k_obs_collect
};
static obs_ws obs_layout(int64_t pixels, WsArena& ws) {
  obs_ws t;
  t.keys = ws.take<uint64_t>(pixels);
  t.hist = ws.take<int>(OBS_PASSES * 256);
  t.counters = ws.take<int>(4);
  return t;
}

// What the pixel draw needs (k_obs_keys / k_obs_hist / k_obs_collect): shared by ngm_target_observed_fields and the
// single-view sampler, which differ in the stream id and in where the frame lies (a slot of a frame stack there).
struct obs_sel {
  const float* rgbd;            // (num_slots, n, 4)
  const int32_t* slot_dev;      // device, or NULL: slot 0
  int num_slots;
  int64_t n;                    // H x W
  int num_points;
  uint32_t stream;
  uint64_t seed;
  int64_t frame;                // >= 0, or < 0: *frame_dev
  const int64_t* frame_dev;
  const int64_t* subset_in;
  int64_t* pixels;
};
__device__ __forceinline__ const float* obs_frame(const obs_sel& a) {
  if (!a.slot_dev) return a.rgbd;
  return a.rgbd + (int64_t)min(max(*a.slot_dev, 0), a.num_slots - 1) * a.n * 4;
}
static obs_sel obs_sel_of(const ngm_observed_fields& a) {
  return obs_sel{a.rgbd, nullptr, 1, (int64_t)a.height * a.width, a.num_points, TSMV_STREAM_PIXELS, a.seed, a.frame, a.frame_dev, a.subset_in,
                 a.pixels};
}

__global__ __launch_bounds__(OBS_THREADS) void k_obs_keys(obs_sel a, obs_ws w) {
  const int64_t n = a.n;
  const int64_t gid = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x, gsz = (int64_t)gridDim.x * OBS_THREADS;
  if (gid < OBS_PASSES * 256) w.hist[gid] = 0;            // the grid has at least OBS_PASSES workgroups (see the launch)
  if (gid < 4) w.counters[gid] = 0;
  const uint64_t frame = (uint64_t)(a.frame >= 0 ? a.frame : *a.frame_dev);     // advanced by a later launch, after every read
  const float* rgbd = obs_frame(a);
  for (int64_t i = gid; i < n; i += gsz) {
    uint64_t key = TSMV_EXCLUDED;
    if (rgbd[4 * i + 3] != 0.0f) {
      uint32_t q[4];
      philox_block(a.seed, frame, (uint64_t)i, a.stream, q);
      key = ((uint64_t)q[0] << 32) | (uint32_t)i;
    }
    w.keys[i] = key;
  }
}

// The state of the select after `passes` finished passes, from their histograms (called by thread 0; sh = the histograms in
// LDS).  take_all: no more valid keys than wanted.  done: the keys whose leading digits are <= prefix (at `shift`) are exactly
// the k smallest.
struct obs_state { uint64_t prefix; int shift, rem, done, take_all; };
__device__ obs_state obs_select_state(const int* sh, int passes, int k) {
  obs_state s = {0ull, 64, k, 0, 0};
  if (passes == 0) return s;
  int total = 0;
  for (int b = 0; b < 256; ++b) total += sh[b];           // pass 0 counts every valid key
  if (total <= k) { s.take_all = 1; s.done = 1; return s; }
  for (int p = 0; p < passes; ++p) {
    const int* h = sh + 256 * p;
    int cum = 0, b = 0;
    for (; b < 255; ++b) {
      if (cum + h[b] >= s.rem) break;
      cum += h[b];
    }
    s.shift -= 8;
    s.prefix = (s.prefix << 8) | (uint64_t)b;
    s.rem -= cum;
    if (h[b] == s.rem || s.shift == 0) { s.done = 1; break; }
  }
  return s;
}
__device__ __forceinline__ obs_state obs_state_block(const obs_ws& w, int passes, int k, int* sh, obs_state* sst) {
  for (int i = threadIdx.x; i < 256 * passes; i += OBS_THREADS) sh[i] = w.hist[i];
  __syncthreads();
  if (threadIdx.x == 0) *sst = obs_select_state(sh, passes, k);
  __syncthreads();
  return *sst;
}

__global__ __launch_bounds__(OBS_THREADS) void k_obs_hist(obs_sel a, obs_ws w, int pass) {
  __shared__ int sh[OBS_PASSES * 256];
  __shared__ int local[256];
  __shared__ obs_state sst;
  const obs_state s = obs_state_block(w, pass, a.num_points, sh, &sst);
  if (s.done) return;                                     // block-uniform
  const int shift = s.shift - 8;                          // this pass' digit
  local[threadIdx.x] = 0;                                 // OBS_THREADS == 256
  __syncthreads();
  const int64_t n = a.n, gsz = (int64_t)gridDim.x * OBS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x; i < n; i += gsz) {
    const uint64_t key = w.keys[i];
    if (key == TSMV_EXCLUDED || (pass > 0 && (key >> (shift + 8)) != s.prefix)) continue;
    atomicAdd(&local[(key >> shift) & 255u], 1);
  }
  __syncthreads();
  const int v = local[threadIdx.x];
  if (v) atomicAdd(&w.hist[256 * pass + threadIdx.x], v);
}

__global__ __launch_bounds__(OBS_THREADS) void k_obs_collect(obs_sel a, obs_ws w) {
  __shared__ int sh[OBS_PASSES * 256];
  __shared__ obs_state sst;
  const int64_t gid = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x, gsz = (int64_t)gridDim.x * OBS_THREADS;
  const int64_t n = a.n;
  if (a.subset_in) {                                      // recorded draws: out-of-range entries become -1 (unused)
    for (int64_t i = gid; i < a.num_points; i += gsz) {
      const int64_t p = a.subset_in[i];
      a.pixels[i] = (p >= 0 && p < n) ? p : -1;
    }
    return;
  }
  const obs_state s = obs_state_block(w, OBS_PASSES, a.num_points, sh, &sst);
  for (int64_t i = gid; i < n; i += gsz) {
    const uint64_t key = w.keys[i];
    if (key == TSMV_EXCLUDED) continue;
    if (!s.take_all && (key >> s.shift) > s.prefix) continue;
    const int p = atomicAdd(&w.counters[0], 1);
    if (p < a.num_points) a.pixels[p] = i;
  }
}

// num_fields_dev (NULL: a.num_fields): the grow variant, a.num_fields is the length of current_field_ids then
__global__ __launch_bounds__(OBS_FIELD_THREADS) void k_obs_fields(ngm_observed_fields a, obs_ws w, const int32_t* num_fields_dev) {
  __shared__ float pts[3 * NGM_OBSERVED_MAX_POINTS];
  __shared__ float wmin[3 * (OBS_FIELD_THREADS / 64)], wmax[3 * (OBS_FIELD_THREADS / 64)];
  __shared__ float box[6];
  __shared__ int wave_cnt[OBS_FIELD_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = OBS_FIELD_THREADS / 64;
  const int64_t n = (int64_t)a.height * a.width;
  // 1. how many pixels were chosen; slots past them are -1
  int used = 0;
  if (a.subset_in) {
    used = a.num_points;                                  // entries of -1 are skipped below, one by one
  } else {
    used = min(w.counters[0], a.num_points);
    for (int i = used + tid; i < a.num_points; i += OBS_FIELD_THREADS) a.pixels[i] = -1;
  }
  // 2. back-projection (camera.py:374-390, OpenGL) and the AABB of the points
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int mine = 0;
  for (int i = tid; i < a.num_points; i += OBS_FIELD_THREADS) {
    const int64_t p = i < used ? a.pixels[i] : -1;
    const bool ok = p >= 0 && p < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (ok) {
      const int r = (int)(p / a.width), c = (int)(p - (int64_t)r * a.width);
      const float d = a.rgbd[4 * p + 3];
      x = (((float)c - a.cx) * d) / a.fx;
      y = ((-((float)r - a.cy)) * d) / a.fy;
      z = -d;
      mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
      mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
      ++mine;
    }
    pts[3 * i] = x; pts[3 * i + 1] = y; pts[3 * i + 2] = ok ? z : NAN;      // NaN z marks an unused slot
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int o = 32; o > 0; o >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
    }
    if (lane == 0) { wmin[3 * wv + k] = mn[k]; wmax[3 * wv + k] = mx[k]; }
  }
  const uint64_t any_b = __ballot(mine > 0);
  if (lane == 0) wave_cnt[wv] = __popcll(any_b);
  __syncthreads();
  if (tid < 3) {
    float lo = INFINITY, hi = -INFINITY;
    for (int q = 0; q < NW; ++q) { lo = fminf(lo, wmin[3 * q + tid]); hi = fmaxf(hi, wmax[3 * q + tid]); }
    box[tid] = lo; box[3 + tid] = hi;
  }
  int have = 0;
  for (int q = 0; q < NW; ++q) have += wave_cnt[q];
  __syncthreads();                                        // box ready, wave_cnt free again
  if (tid == 0) {
    int cnt = 0;                                          // valid chosen pixels (subset_in may hold unused entries)
    if (a.subset_in) { for (int i = 0; i < a.num_points; ++i) cnt += pts[3 * i + 2] == pts[3 * i + 2] ? 1 : 0; }
    else cnt = used;
    *a.num_used = cnt;
  }
  // 3. per field: sphere AABB vs. point AABB (geometry.py:26-42), then the segment test over the points (geometry.py:67-105)
  const float* T = a.c2w;
  const float r = a.radius, r2 = r * r;
  int base = 0;
  const int num_fields = num_fields_dev ? min(max(*num_fields_dev, 0), a.num_fields) : a.num_fields;      // block-uniform
  for (int f0 = 0; f0 < num_fields; f0 += OBS_FIELD_THREADS) {
    const int f = f0 + tid;
    bool seen = false;
    if (f < num_fields && have > 0) {
      const Cam3 c = world_to_cam(T, a.field_positions[3 * f], a.field_positions[3 * f + 1], a.field_positions[3 * f + 2]);
      const bool in_box = c.x - r <= box[3] && c.y - r <= box[4] && c.z - r <= box[5] && c.x + r >= box[0] && c.y + r >= box[1] &&
                          c.z + r >= box[2];
      if (in_box) {
        for (int i = 0; i < a.num_points && !seen; ++i) {
          const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
          if (pz != pz) continue;
          float sq = (px * px + py * py) + pz * pz;
          if (sq == 0.0f) sq = 1.0f;
          const float t = fminf(fmaxf(((c.x * px + c.y * py) + c.z * pz) / sq, 0.0f), 1.0f);
          const float ex = c.x - px * t, ey = c.y - py * t, ez = c.z - pz * t;
          seen = (ex * ex + ey * ey) + ez * ez <= r2;
        }
      }
    }
    // ascending compaction of this chunk
    const uint64_t bal = __ballot(seen);
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int q = 0; q < NW; ++q) {
      off += q < wv ? wave_cnt[q] : 0;
      tot += wave_cnt[q];
    }
    if (seen) a.current_field_ids[off + __popcll(bal & ((1ull << lane) - 1ull))] = f;
    base += tot;
    __syncthreads();
  }
  for (int i = base + tid; i < a.num_fields; i += OBS_FIELD_THREADS) a.current_field_ids[i] = -1;
  if (tid == 0) {
    *a.current_count = base;
    if (a.frame < 0) *a.frame_dev = *a.frame_dev + 1;     // every read of the counter was in k_obs_keys, an earlier launch
  }
}

// the pixel draw: keys + 8 histogram passes + collect, or with subset_in the copy alone
static void obs_launch_select(const obs_sel& a, const obs_ws& w, hipStream_t st) {
  const int64_t n = a.n;
  int blocks = (int)((n + OBS_THREADS - 1) / OBS_THREADS);
  blocks = blocks < OBS_PASSES ? OBS_PASSES : blocks > OBS_MAX_BLOCKS ? OBS_MAX_BLOCKS : blocks;
  if (!a.subset_in) {
    hipLaunchKernelGGL(k_obs_keys, dim3(blocks), dim3(OBS_THREADS), 0, st, a, w);
    for (int p = 0; p < OBS_PASSES; ++p) hipLaunchKernelGGL(k_obs_hist, dim3(blocks), dim3(OBS_THREADS), 0, st, a, w, p);
  }
  hipLaunchKernelGGL(k_obs_collect, dim3(a.subset_in ? (a.num_points + OBS_THREADS - 1) / OBS_THREADS : blocks), dim3(OBS_THREADS), 0, st,
                     a, w);
}

int64_t ngm_target_observed_fields_bytes(int height, int width) { return ws_bytes(obs_layout, (int64_t)height * width); }
int ngm_launch_target_observed_fields(const ngm_observed_fields& a, void* workspace, int64_t workspace_bytes, hipStream_t st,
                                      const int32_t* num_fields_dev) {
  WsArena ws(workspace);
  const obs_ws w = obs_layout((int64_t)a.height * a.width, ws);
  if (!workspace || !ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  obs_launch_select(obs_sel_of(a), w, st);
  hipLaunchKernelGGL(k_obs_fields, dim3(1), dim3(OBS_FIELD_THREADS), 0, st, a, w, num_fields_dev);
  return 0;
}

// ---- the single-view sampler, whole, on the device (ngm_target_sample_sv, include/ngm_hip.h) ------------------------------
// No host synchronisation, no hit matrix in memory:
//   k_obs_keys / k_obs_hist x 8 / k_obs_collect  the pixel draw (stream ..07), or the copy of pixels_in
//   k_tssv_points  one thread per chosen pixel: back-projection into the workspace, min / max / valid count per workgroup
//                  (partials, reduced by their readers: no float atomics); zeroes `hits`; keeps the iteration for the others
//   k_tssv_box     one workgroup, once per call: the box and the valid count from the partials; camera-frame centre and box test
//                  per active field, the fields in the box compacted into the workspace (ballot + prefix)
//   k_tssv_count   one lane per point; the fields in the box pass through LDS in tiles of 256 and every wave tests them
//                  against its 64 points: ballot + popcount into an LDS count, then one integer atomic per (workgroup, field)
//   k_tssv_draw    one workgroup: candidates in the order of active_field_ids (ballot + prefix), the field draw
//                  (tsmv_k_smallest over the candidates' keys, positions recovered by binary search), the owner filter
//   k_tssv_rows    one workgroup per row: re-tests the row's field against the points, forms the ray keys in the workspace,
//                  tsmv_k_smallest for the num_rays smallest, then target_sv_ray_one per ray; rows past the count are padding;
//                  advances the iteration counter (every read of it was in an earlier launch)
// tsmv_k_smallest ends in an O(k^2) rank sort: at num_rays = 512 each of the 512 threads reads 512 keys from LDS (the same
// address across a wave: broadcasts), about as much as one pass over 50 000 keys costs; rows run side by side on their CUs.
constexpr uint32_t TSSV_STREAM_PIXELS = 0x54470007u, TSSV_STREAM_FIELDS = 0x54470008u, TSSV_STREAM_RAYS = 0x54470009u;
constexpr int TSSV_PT_THREADS = 256, TSSV_DRAW_THREADS = 1024, TSSV_ROW_THREADS = 512;

struct __align__(16) tssv_pt { float x, y, z; int pix; };        // pix < 0: unused slot
struct __align__(16) tssv_part { float mn[3], mx[3]; int count, pad; };
struct __align__(16) tssv_box { float lo[3], hi[3]; int have, n_in; };   // have: valid points; n_in: entries of `inbox`
struct __align__(16) tssv_in { float x, y, z; int k; };          // k: position in active_field_ids

struct tssv_ws {
  obs_ws sel;
  int64_t* hdr;        // [0] iteration of this call
  tssv_pt* pts;        // num_points
  tssv_part* part;     // one per workgroup of k_tssv_points
  tssv_box* box;       // 1: the points' AABB, the valid points, the fields in the box
  tssv_in* inbox;      // num_active: camera-frame centres of the fields in the box
  int* cand;          // num_active: candidate -> position in active_field_ids
  uint64_t* fkeys;     // num_active: field keys by candidate
  uint64_t* rkeys;     // capacity x num_points: ray keys
};
static int tssv_pt_blocks(int num_points) { return (num_points + TSSV_PT_THREADS - 1) / TSSV_PT_THREADS; }
static tssv_ws tssv_layout(int64_t pixels, int num_active, int num_points, int capacity, WsArena& ws) {
  tssv_ws t;
  t.sel = obs_layout(pixels, ws);
  t.hdr = ws.take<int64_t>(2);
  t.pts = ws.take<tssv_pt>(num_points);
  t.part = ws.take<tssv_part>(tssv_pt_blocks(num_points));
  t.box = ws.take<tssv_box>(1);
  t.inbox = ws.take<tssv_in>(num_active);
  t.cand = ws.take<int>(num_active);
  t.fkeys = ws.take<uint64_t>(num_active);
  t.rkeys = ws.take<uint64_t>((int64_t)capacity * num_points);
  return t;
}

__device__ __forceinline__ int tssv_slot(const ngm_target_sample_sv_args& a) {
  return a.slot_dev ? min(max(*a.slot_dev, 0), a.num_slots - 1) : 0;
}

__global__ __launch_bounds__(TSSV_PT_THREADS) void k_tssv_points(ngm_target_sample_sv_args a, tssv_ws w) {
  __shared__ float wmin[3 * (TSSV_PT_THREADS / 64)], wmax[3 * (TSSV_PT_THREADS / 64)];
  __shared__ int wcnt[TSSV_PT_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = blockIdx.x * TSSV_PT_THREADS + tid;
  const int64_t n = (int64_t)a.height * a.width;
  if (blockIdx.x == 0 && tid == 0) w.hdr[0] = a.iteration >= 0 ? a.iteration : *a.iteration_dev;
  for (int k = i; k < a.num_active; k += gridDim.x * TSSV_PT_THREADS) a.hits[k] = 0;
  const int used = a.pixels_in ? a.num_points : min(w.sel.counters[0], a.num_points);
  const float* rgbd = a.rgbd + (int64_t)tssv_slot(a) * n * 4;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool ok = false;
  if (i < a.num_points) {
    int64_t p = -1;
    if (i < used) p = a.pixels[i];
    else a.pixels[i] = -1;                                 // slots past the chosen pixels (never with pixels_in)
    ok = p >= 0 && p < n;
    tssv_pt pt = {0.f, 0.f, 0.f, -1};
    if (ok) {                                              // camera.py:374-390, OpenGL: k_obs_fields' arithmetic
      const int r = (int)(p / a.width), c = (int)(p - (int64_t)r * a.width);
      const float d = rgbd[4 * p + 3];
      pt.x = (((float)c - a.cx) * d) / a.fx;
      pt.y = ((-((float)r - a.cy)) * d) / a.fy;
      pt.z = -d;
      pt.pix = (int)p;
      mn[0] = mx[0] = pt.x; mn[1] = mx[1] = pt.y; mn[2] = mx[2] = pt.z;
    }
    w.pts[i] = pt;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int o = 32; o > 0; o >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
    }
    if (lane == 0) { wmin[3 * wv + k] = mn[k]; wmax[3 * wv + k] = mx[k]; }
  }
  const uint64_t bal = __ballot(ok);
  if (lane == 0) wcnt[wv] = __popcll(bal);
  __syncthreads();
  if (tid == 0) {
    tssv_part q;
    q.count = 0; q.pad = 0;
    for (int k = 0; k < 3; ++k) { q.mn[k] = INFINITY; q.mx[k] = -INFINITY; }
    for (int v = 0; v < TSSV_PT_THREADS / 64; ++v) {
      q.count += wcnt[v];
      for (int k = 0; k < 3; ++k) { q.mn[k] = fminf(q.mn[k], wmin[3 * v + k]); q.mx[k] = fmaxf(q.mx[k], wmax[3 * v + k]); }
    }
    w.part[blockIdx.x] = q;
  }
}

// once per call: the points' box and count from the partials, and the active fields that are in force and in the box, with their
// camera-frame centres, compacted in the order of active_field_ids (ballot + prefix)
__global__ __launch_bounds__(TSSV_DRAW_THREADS) void k_tssv_box(ngm_target_sample_sv_args a, tssv_ws w, int pt_blocks) {
  __shared__ float red[6][TSSV_DRAW_THREADS / 64];
  __shared__ int redc[TSSV_DRAW_THREADS / 64], wave_cnt[TSSV_DRAW_THREADS / 64];
  __shared__ float box[6];
  __shared__ int s_have;
  constexpr int NW = TSSV_DRAW_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int cnt = 0;
  for (int b = tid; b < pt_blocks; b += TSSV_DRAW_THREADS) {       // exact min / max: the order of the partials does not matter
    const tssv_part q = w.part[b];
    cnt += q.count;
#pragma unroll
    for (int k = 0; k < 3; ++k) { mn[k] = fminf(mn[k], q.mn[k]); mx[k] = fmaxf(mx[k], q.mx[k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int o = 32; o > 0; o >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
    }
    if (lane == 0) { red[k][wv] = mn[k]; red[3 + k][wv] = mx[k]; }
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) redc[wv] = cnt;
  __syncthreads();
  if (tid < 6) {
    float v = red[tid][0];
    for (int q = 1; q < NW; ++q) v = tid < 3 ? fminf(v, red[tid][q]) : fmaxf(v, red[tid][q]);
    box[tid] = v;
  }
  if (tid == 6) {
    int have = 0;
    for (int q = 0; q < NW; ++q) have += redc[q];
    s_have = have;
  }
  __syncthreads();
  const int have = s_have;
  const float* T = a.c2w + 16 * (int64_t)tssv_slot(a);
  const float r = a.radius;
  const int nf = a.num_fields_dev ? min(max(*a.num_fields_dev, 0), a.num_fields) : a.num_fields;      // block-uniform
  int base = 0;
  for (int k0 = 0; k0 < a.num_active && have > 0; k0 += TSSV_DRAW_THREADS) {
    const int k = k0 + tid;
    bool in_box = false;
    Cam3 c = {0.f, 0.f, 0.f};
    if (k < a.num_active) {
      const int64_t id = a.active_field_ids[k];
      if (id >= 0 && id < nf) {
        c = world_to_cam(T, a.field_positions[3 * id], a.field_positions[3 * id + 1], a.field_positions[3 * id + 2]);
        in_box = c.x - r <= box[3] && c.y - r <= box[4] && c.z - r <= box[5] && c.x + r >= box[0] && c.y + r >= box[1] &&
                 c.z + r >= box[2];
      }
    }
    const uint64_t bal = __ballot(in_box);
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int q = 0; q < NW; ++q) {
      off += q < wv ? wave_cnt[q] : 0;
      tot += wave_cnt[q];
    }
    if (in_box) w.inbox[off + __popcll(bal & ((1ull << lane) - 1ull))] = tssv_in{c.x, c.y, c.z, k};
    base += tot;
    __syncthreads();
  }
  if (tid == 0) {
    tssv_box q;
    for (int k = 0; k < 3; ++k) { q.lo[k] = box[k]; q.hi[k] = box[3 + k]; }
    q.have = have; q.n_in = base;
    *w.box = q;
    *a.num_used = have;
  }
}

__global__ __launch_bounds__(TSSV_PT_THREADS) void k_tssv_count(ngm_target_sample_sv_args a, tssv_ws w) {
  __shared__ float tx[TSSV_PT_THREADS], ty[TSSV_PT_THREADS], tz[TSSV_PT_THREADS];
  __shared__ int tk[TSSV_PT_THREADS], tc[TSSV_PT_THREADS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int n_in = min(max(w.box->n_in, 0), a.num_active);          // block-uniform; 0 without valid points
  if (n_in == 0) return;                                  // `hits` is all zero already
  const int i = blockIdx.x * TSSV_PT_THREADS + tid;
  tssv_pt pt = {0.f, 0.f, 0.f, -1};
  if (i < a.num_points) pt = w.pts[i];
  const bool valid = pt.pix >= 0;
  const float r2 = a.radius * a.radius;
  for (int q0 = 0; q0 < n_in; q0 += TSSV_PT_THREADS) {
    const int nt = min(TSSV_PT_THREADS, n_in - q0);
    if (tid < nt) {
      const tssv_in f = w.inbox[q0 + tid];
      tx[tid] = f.x; ty[tid] = f.y; tz[tid] = f.z; tk[tid] = f.k;
    }
    tc[tid] = 0;
    __syncthreads();
    for (int q = 0; q < nt; ++q) {
      const bool h = valid && target_sv_hit(tx[q], ty[q], tz[q], pt.x, pt.y, pt.z, r2);
      const uint64_t bal = __ballot(h);
      if (lane == 0 && bal) atomicAdd(&tc[q], __popcll(bal));           // LDS; one global atomic per (workgroup, field) below
    }
    __syncthreads();
    if (tid < nt && tc[tid]) atomicAdd(&a.hits[tk[tid]], tc[tid]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(TSSV_DRAW_THREADS) void k_tssv_draw(ngm_target_sample_sv_args a, tssv_ws w) {
  __shared__ uint64_t sel[NGM_TARGET_MAX_DRAW], scratch[NGM_TARGET_MAX_DRAW];
  __shared__ int drawn[NGM_TARGET_MAX_DRAW];
  __shared__ int hist[256], st[4], wave_cnt[TSSV_DRAW_THREADS / 64];
  __shared__ int s_rows;
  constexpr int NW = TSSV_DRAW_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t it = (uint64_t)w.hdr[0];
  const int A = a.num_active, T = a.num_train_fields, R = a.num_rays;
  // 1. candidates in the order of active_field_ids (hits are counted only for fields in force and in the box)
  int base = 0;
  for (int k0 = 0; k0 < A; k0 += TSSV_DRAW_THREADS) {
    const int k = k0 + tid;
    const bool is_c = k < A && a.hits[k] >= R;
    const uint64_t bal = __ballot(is_c);
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int q = 0; q < NW; ++q) {
      off += q < wv ? wave_cnt[q] : 0;
      tot += wave_cnt[q];
    }
    if (is_c) w.cand[off + __popcll(bal & ((1ull << lane) - 1ull))] = k;
    base += tot;
    __syncthreads();
  }
  const int nc = base, n_draw = min(nc, T);
  if (tid == 0) *a.num_candidates = nc;
  for (int i = tid; i < T; i += TSSV_DRAW_THREADS) {
    drawn[i] = -1;
    a.subset_fields[i] = -1;
  }
  __syncthreads();
  // 2. the fields: all candidates, the recorded positions, or the T smallest keys in key order
  if (nc <= T) {
    for (int i = tid; i < nc; i += TSSV_DRAW_THREADS) { drawn[i] = w.cand[i]; a.subset_fields[i] = i; }
  } else if (a.subset_fields_in) {
    for (int i = tid; i < T; i += TSSV_DRAW_THREADS) {
      const int64_t c = a.subset_fields_in[i];
      if (c >= 0 && c < nc) { drawn[i] = w.cand[c]; a.subset_fields[i] = c; }
    }
  } else {
    for (int c = tid; c < nc; c += TSSV_DRAW_THREADS) {
      const uint64_t g = (uint64_t)a.active_field_ids[w.cand[c]];
      uint32_t q[4];
      philox_block(a.seed, it, g, TSSV_STREAM_FIELDS, q);
      w.fkeys[c] = ((uint64_t)q[0] << 32) | (uint32_t)g;
    }
    __syncthreads();
    tsmv_k_smallest(w.fkeys, nc, T, sel, scratch, hist, st);
    for (int c = tid; c < nc; c += TSSV_DRAW_THREADS) {   // the rank of candidate c among the chosen keys, if it is one
      const uint64_t key = w.fkeys[c];
      int lo = 0, hi = T;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sel[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < T && sel[lo] == key) { drawn[lo] = w.cand[c]; a.subset_fields[lo] = c; }
    }
  }
  __syncthreads();
  // 3. owner filter, draw order kept
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < n_draw; ++i) {
      if (drawn[i] < 0) continue;
      const int64_t g = a.active_field_ids[drawn[i]];
      if (g % a.world_size == a.rank && n < a.capacity) a.field_ids[n++] = g;
    }
    s_rows = n;
    *a.count = n;
    if (a.capacity == 0 && a.iteration < 0) *a.iteration_dev = (int64_t)it + 1;      // no k_tssv_rows launch then
  }
  __syncthreads();
  for (int i = s_rows + tid; i < a.capacity; i += TSSV_DRAW_THREADS) a.field_ids[i] = -1;
}

__device__ __forceinline__ void tssv_zero_ray(const ngm_target_out& o, int64_t idx) {
  if (o.c2ws) {
    float4* dst = reinterpret_cast<float4*>(o.c2ws + 16 * idx);
    dst[0] = dst[1] = dst[2] = dst[3] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  o.ijs[2 * idx] = 0; o.ijs[2 * idx + 1] = 0;
  o.near[idx] = 0.f; o.far[idx] = 0.f; o.gt[idx] = 0.f;
  reinterpret_cast<float4*>(o.rgbds)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
  o.rgb_mask[idx] = 0; o.depth_mask[idx] = 0; o.term_probs[idx] = 0.f; o.term_mask[idx] = 0;
}

__global__ __launch_bounds__(TSSV_ROW_THREADS) void k_tssv_rows(ngm_target_sample_sv_args a, ngm_target_out o, tssv_ws w) {
  __shared__ uint64_t sel[NGM_TARGET_MAX_DRAW], scratch[NGM_TARGET_MAX_DRAW];
  __shared__ int hist[256], st[4];
  const int row = blockIdx.x, tid = threadIdx.x, R = a.num_rays;
  const uint64_t it = (uint64_t)w.hdr[0];
  const int cnt = min(max(*a.count, 0), a.capacity);
  if (row == 0 && tid == 0 && a.iteration < 0) *a.iteration_dev = (int64_t)it + 1;
  if (row >= cnt) {                                       // block-uniform
    for (int k = tid; k < R; k += TSSV_ROW_THREADS) {
      tssv_zero_ray(o, (int64_t)row * R + k);
      a.segments[(int64_t)row * R + k] = -1;
    }
    return;
  }
  const int64_t n = (int64_t)a.height * a.width;
  const int slot = tssv_slot(a);
  const float* T = a.c2w + 16 * (int64_t)slot;
  const float* image = a.rgbd + (int64_t)slot * n * 4;
  const int64_t g = a.field_ids[row];
  const Cam3 c = world_to_cam(T, a.field_positions[3 * g], a.field_positions[3 * g + 1], a.field_positions[3 * g + 2]);
  if (!a.segments_in) {
    const float r2 = a.radius * a.radius;
    uint64_t* keys = w.rkeys + (int64_t)row * a.num_points;
    for (int i = tid; i < a.num_points; i += TSSV_ROW_THREADS) {
      const tssv_pt pt = w.pts[i];
      uint64_t key = TSMV_EXCLUDED;
      if (pt.pix >= 0 && target_sv_hit(c.x, c.y, c.z, pt.x, pt.y, pt.z, r2)) {
        uint32_t q[4];
        philox_block(a.seed, it, ((uint64_t)g << 32) | (uint32_t)pt.pix, TSSV_STREAM_RAYS, q);
        key = ((uint64_t)q[0] << 32) | (uint32_t)pt.pix;
      }
      keys[i] = key;
    }
    __syncthreads();
    tsmv_k_smallest(keys, a.num_points, R, sel, scratch, hist, st);
  }
  for (int k = tid; k < R; k += TSSV_ROW_THREADS) {
    const int64_t idx = (int64_t)row * R + k;
    int64_t p = -1;
    if (a.segments_in) {
      const int64_t s = a.segments_in[idx];
      if (s >= 0 && s < a.num_points) p = w.pts[s].pix;
    } else {
      p = (int64_t)(sel[k] & 0xFFFFFFFFull);
    }
    if (p < 0 || p >= n) {                                // a recorded draw that names an unused point
      tssv_zero_ray(o, idx);
      a.segments[idx] = -1;
      continue;
    }
    a.segments[idx] = p;
    if (o.c2ws) {
      float4* dst = reinterpret_cast<float4*>(o.c2ws + 16 * idx);
      const float4* src = reinterpret_cast<const float4*>(T);
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
    }
    const int64_t i = p / a.width, j = p - i * a.width;
    target_sv_ray_one(c.x, c.y, c.z, a.radius, i, j, image, a.width, a.fx, a.fy, a.cx, a.cy, o, idx);
  }
}

int64_t ngm_target_sample_sv_bytes(int height, int width, int num_active, int num_points, int capacity) {
  return ws_bytes(tssv_layout, (int64_t)height * width, num_active, num_points, capacity);
}
int ngm_launch_target_sample_sv(const ngm_target_sample_sv_args& a, const ngm_target_out& o, void* workspace, int64_t workspace_bytes,
                                hipStream_t st) {
  WsArena ws(workspace);
  const int64_t n = (int64_t)a.height * a.width;
  const tssv_ws w = tssv_layout(n, a.num_active, a.num_points, a.capacity, ws);
  if (!workspace || !ws.covers(workspace_bytes)) return NGM_E_WORKSPACE;
  obs_launch_select(obs_sel{a.rgbd, a.slot_dev, a.num_slots, n, a.num_points, TSSV_STREAM_PIXELS, a.seed, a.iteration, a.iteration_dev,
                            a.pixels_in, a.pixels}, w.sel, st);
  const int pb = tssv_pt_blocks(a.num_points);
  hipLaunchKernelGGL(k_tssv_points, dim3(pb), dim3(TSSV_PT_THREADS), 0, st, a, w);
  hipLaunchKernelGGL(k_tssv_box, dim3(1), dim3(TSSV_DRAW_THREADS), 0, st, a, w, pb);
  if (a.num_active > 0) hipLaunchKernelGGL(k_tssv_count, dim3(pb), dim3(TSSV_PT_THREADS), 0, st, a, w);
  hipLaunchKernelGGL(k_tssv_draw, dim3(1), dim3(TSSV_DRAW_THREADS), 0, st, a, w);
  if (a.capacity > 0) hipLaunchKernelGGL(k_tssv_rows, dim3(a.capacity), dim3(TSSV_ROW_THREADS), 0, st, a, o, w);
  return 0;
}

// ---- reserved field rows: a keyframe's growth as one launch (ngm_fields_append, include/ngm_hip.h) ------------------------
// blockIdx.z = tensor, blockIdx.y = new row, blockIdx.x strides over the row (k_adam_multi's shape).  Block (0, 0, 0) also
// writes the poses, the iteration counts and the new field count: nothing in this launch reads them, and the next launch on
// the stream starts after every store of this one.
struct FieldsAppendK {
  ngm_append_tensor t[NGM_APPEND_MAX_TENSORS];
  int n, first, num_new;
  const float* new_pos; const float* new_quat;
  float* pos; float* quat;
  int64_t* training_iterations;
  int32_t* num_fields_dev;
};
__global__ __launch_bounds__(256) void k_fields_append(FieldsAppendK a) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    for (int i = tid; i < 3 * a.num_new; i += blockDim.x) a.pos[3 * (int64_t)a.first + i] = a.new_pos[i];
    for (int i = tid; i < 4 * a.num_new; i += blockDim.x) a.quat[4 * (int64_t)a.first + i] = a.new_quat[i];
    if (a.training_iterations)
      for (int i = tid; i < a.num_new; i += blockDim.x) a.training_iterations[a.first + i] = 0;
    if (tid == 0) *a.num_fields_dev = a.first + a.num_new;
  }
  if ((int)blockIdx.z >= a.n) return;                     // a launch without tensors still has one z slice
  const ngm_append_tensor& t = a.t[blockIdx.z];
  const int64_t row = (int64_t)a.first + blockIdx.y;
  const int64_t base = row * t.stride;
  const bool vec = ((t.numel | t.stride) & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.prototype) |
                     reinterpret_cast<uintptr_t>(t.exp_avg) | reinterpret_cast<uintptr_t>(t.exp_avg_sq)) & 15) == 0;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + tid, step = (int64_t)gridDim.x * blockDim.x;
  if (vec) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* S4 = reinterpret_cast<const float4*>(t.prototype);
    float4* P4 = reinterpret_cast<float4*>(t.param + base);
    float4* M4 = t.exp_avg ? reinterpret_cast<float4*>(t.exp_avg + base) : nullptr;
    float4* V4 = t.exp_avg_sq ? reinterpret_cast<float4*>(t.exp_avg_sq + base) : nullptr;
    for (int64_t i = i0; i < (t.numel >> 2); i += step) {
      const float4 p = S4[i];
      P4[i] = p;
      if (M4) M4[i] = zero;
      if (V4) V4[i] = zero;
      if (t.param_lp) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ngm_stp(t.param_lp, base + 4 * i + c, (&p.x)[c], t.lp_dtype);
      }
    }
    return;
  }
  for (int64_t i = i0; i < t.numel; i += step) {
    const float p = t.prototype[i];
    t.param[base + i] = p;
    if (t.exp_avg) t.exp_avg[base + i] = 0.f;
    if (t.exp_avg_sq) t.exp_avg_sq[base + i] = 0.f;
    if (t.param_lp) ngm_stp(t.param_lp, base + i, p, t.lp_dtype);
  }
}
int ngm_launch_fields_append(const ngm_fields_append_args& a, hipStream_t st) {
  FieldsAppendK k = {};
  int64_t mx = 1;
  for (int i = 0; i < a.num_tensors; ++i) { k.t[i] = a.tensors[i]; mx = mx > a.tensors[i].numel ? mx : a.tensors[i].numel; }
  k.n = a.num_tensors; k.first = a.first; k.num_new = a.num_new;
  k.new_pos = a.new_positions; k.new_quat = a.new_orientations; k.pos = a.positions; k.quat = a.orientations;
  k.training_iterations = a.training_iterations; k.num_fields_dev = a.num_fields_dev;
  int64_t bx = (mx / 4 + 255) / 256 + 1;                  // one pass over the largest tensor in 16-byte accesses, at most 64 blocks
  bx = bx > 64 ? 64 : bx;
  hipLaunchKernelGGL(k_fields_append, dim3((unsigned)bx, (unsigned)a.num_new, (unsigned)(a.num_tensors > 0 ? a.num_tensors : 1)),
                     dim3(256), 0, st, k);
  return 0;
}
