// Re-pose the map after a pose-graph update (ngm_fields_repose, include/ngm_hip.h): every field follows the keyframe it is
// anchored to, NeuralGraphMap._update_field_poses (rm.py:937-952) = _absolute_map_dict_to_relative with the previous
// keyframe poses followed by _relative_map_dict_to_absolute with the new ones (rm.py:844-885; utils.transform_points /
// transform_quaternions, utils.py:270-286), as one launch, in place, in fp32.
//   k_fields_repose : one thread per field; 2 x 64 B of pose table (cached: many fields share an anchor), 28 B of field
//                     pose in and out.  No atomics, no cross-thread traffic: bitwise deterministic.
//   k_pose_advance  : prev := new afterwards (advance_prev), one thread per pose row, a launch of its own because the
//                     threads of the first still read prev.
#include "ngm_launch.h"

#pragma clang fp contract(off)

struct Quat { float w, x, y, z; };

__device__ __forceinline__ bool repose_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// pytorch3d.transforms.matrix_to_quaternion of the row-major 3x3 m: of the four candidates (pivot w, x, y, z) the one with
// the largest |component| (the first on ties, as torch.argmax), divided by 2 max(|component|, 0.1); real part made
// non-negative (standardize_quaternion).  Accurate at a rotation by pi, where the trace-only formula divides by ~0.
__device__ __forceinline__ Quat repose_matrix_to_quat(const float* m) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
  const float s0 = 1.f + m00 + m11 + m22, s1 = 1.f + m00 - m11 - m22, s2 = 1.f - m00 + m11 - m22, s3 = 1.f - m00 - m11 + m22;
  const float a0 = s0 > 0.f ? sqrtf(s0) : 0.f, a1 = s1 > 0.f ? sqrtf(s1) : 0.f;
  const float a2 = s2 > 0.f ? sqrtf(s2) : 0.f, a3 = s3 > 0.f ? sqrtf(s3) : 0.f;
  int best = 0;
  float ab = a0;
  if (a1 > ab) { best = 1; ab = a1; }
  if (a2 > ab) { best = 2; ab = a2; }
  if (a3 > ab) { best = 3; ab = a3; }
  const float d = 2.f * (ab > 0.1f ? ab : 0.1f);
  Quat q;
  if (best == 0)      q = { a0 * a0, m21 - m12, m02 - m20, m10 - m01 };
  else if (best == 1) q = { m21 - m12, a1 * a1, m10 + m01, m02 + m20 };
  else if (best == 2) q = { m02 - m20, m10 + m01, a2 * a2, m12 + m21 };
  else                q = { m10 - m01, m20 + m02, m21 + m12, a3 * a3 };
  q.w = q.w / d; q.x = q.x / d; q.y = q.y / d; q.z = q.z / d;
  if (q.w < 0.f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
  return q;
}

// raw Hamilton product a (x) b: no standardisation, no normalisation
__device__ __forceinline__ Quat repose_quat_mul(const Quat& a, const Quat& b) {
  Quat o;
  o.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  o.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  o.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  o.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  return o;
}

struct ReposeK {
  float* pos; float* quat;
  const int32_t* anchor;
  const float* prev; const float* nw;
  const int32_t* num_fields_dev;
  int num_fields, num_poses;
};

__global__ __launch_bounds__(256) void k_fields_repose(ReposeK a) {
  int nf = a.num_fields;
  if (a.num_fields_dev) {
    const int d = *a.num_fields_dev;
    nf = d < 0 ? 0 : (d < nf ? d : nf);
  }
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;                                     // rows at or beyond the count in force
  const int s = a.anchor[f];
  if (s < 0 || s >= a.num_poses) return;                   // unanchored, or an anchor the tables have no row for
  const float* P = a.prev + 16 * (int64_t)s;
  const float* N = a.nw + 16 * (int64_t)s;
  float p[16], n[16];
  bool same = true, finite = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    p[i] = P[i]; n[i] = N[i];
    same = same && __float_as_uint(p[i]) == __float_as_uint(n[i]);
    finite = finite && repose_finite(p[i]) && repose_finite(n[i]);
  }
  if (same || !finite) return;                             // the keyframe did not move / a lost pose: not one bit changes

  // W = inverse(prev), affine with last row (0, 0, 0, 1): 3x3 inverse by adjugate and determinant (rm.py:870 `.inverse()`)
  const float r00 = p[0], r01 = p[1], r02 = p[2], r10 = p[4], r11 = p[5], r12 = p[6], r20 = p[8], r21 = p[9], r22 = p[10];
  const float c00 = r11 * r22 - r12 * r21, c01 = r12 * r20 - r10 * r22, c02 = r10 * r21 - r11 * r20;
  const float det = r00 * c00 + r01 * c01 + r02 * c02;
  float w[9];
  w[0] = c00 / det;                       w[1] = (r02 * r21 - r01 * r22) / det;  w[2] = (r01 * r12 - r02 * r11) / det;
  w[3] = c01 / det;                       w[4] = (r00 * r22 - r02 * r20) / det;  w[5] = (r02 * r10 - r00 * r12) / det;
  w[6] = c02 / det;                       w[7] = (r01 * r20 - r00 * r21) / det;  w[8] = (r00 * r11 - r01 * r10) / det;
  const float tx = p[3], ty = p[7], tz = p[11];
  const float wtx = -(w[0] * tx + w[1] * ty + w[2] * tz);
  const float wty = -(w[3] * tx + w[4] * ty + w[5] * tz);
  const float wtz = -(w[6] * tx + w[7] * ty + w[8] * tz);

  const float px = a.pos[3 * (int64_t)f], py = a.pos[3 * (int64_t)f + 1], pz = a.pos[3 * (int64_t)f + 2];
  const Quat q = { a.quat[4 * (int64_t)f], a.quat[4 * (int64_t)f + 1], a.quat[4 * (int64_t)f + 2], a.quat[4 * (int64_t)f + 3] };
  // absolute -> relative to the previous keyframe pose (rm.py:875-876)
  const float rx = (w[0] * px + w[1] * py + w[2] * pz) + wtx;
  const float ry = (w[3] * px + w[4] * py + w[5] * pz) + wty;
  const float rz = (w[6] * px + w[7] * py + w[8] * pz) + wtz;
  const Quat q_rel = repose_quat_mul(repose_matrix_to_quat(w), q);
  // relative -> absolute under the new keyframe pose (rm.py:852-853)
  const float ox = (n[0] * rx + n[1] * ry + n[2] * rz) + n[3];
  const float oy = (n[4] * rx + n[5] * ry + n[6] * rz) + n[7];
  const float oz = (n[8] * rx + n[9] * ry + n[10] * rz) + n[11];
  const float nr[9] = { n[0], n[1], n[2], n[4], n[5], n[6], n[8], n[9], n[10] };
  const Quat o = repose_quat_mul(repose_matrix_to_quat(nr), q_rel);
  // a singular previous pose (determinant 0) gives no finite result: such a field stays where it is, like a lost pose
  if (!(repose_finite(ox) && repose_finite(oy) && repose_finite(oz) && repose_finite(o.w) && repose_finite(o.x) &&
        repose_finite(o.y) && repose_finite(o.z)))
    return;
  a.pos[3 * (int64_t)f] = ox; a.pos[3 * (int64_t)f + 1] = oy; a.pos[3 * (int64_t)f + 2] = oz;
  a.quat[4 * (int64_t)f] = o.w; a.quat[4 * (int64_t)f + 1] = o.x; a.quat[4 * (int64_t)f + 2] = o.y; a.quat[4 * (int64_t)f + 3] = o.z;
}

// prev[s] := new[s] for every finite row of new.  A row with a non-finite entry is not copied: the fields anchored to it
// were not moved, so prev keeps the pose they still stand at, and the re-pose after the pose is found again is exact.
__global__ __launch_bounds__(256) void k_pose_advance(float* prev, const float* nw, int num_poses) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= num_poses) return;
  float n[16];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) { n[i] = nw[16 * (int64_t)s + i]; finite = finite && repose_finite(n[i]); }
  if (!finite) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) prev[16 * (int64_t)s + i] = n[i];
}

int ngm_launch_fields_repose(const ngm_fields_repose_args& a, hipStream_t st) {
  ReposeK k = {};
  k.pos = a.positions; k.quat = a.orientations; k.anchor = a.anchor_slot; k.prev = a.prev_poses; k.nw = a.new_poses;
  k.num_fields_dev = a.num_fields_dev; k.num_fields = a.num_fields; k.num_poses = a.num_poses;
  if (a.num_fields > 0 && a.num_poses > 0)
    hipLaunchKernelGGL(k_fields_repose, dim3((unsigned)((a.num_fields + 255) / 256)), dim3(256), 0, st, k);
  if (a.advance_prev && a.num_poses > 0)
    hipLaunchKernelGGL(k_pose_advance, dim3((unsigned)((a.num_poses + 255) / 256)), dim3(256), 0, st, a.prev_poses, a.new_poses,
                       a.num_poses);
  return 0;
}
