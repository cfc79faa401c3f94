"""Host restatement (numpy) of the reference's re-pose of the map after a pose-graph update, in a chosen dtype (float64: the
yardstick; float32: the rounding a faithful fp32 implementation has):

  utils.transform_points / transform_quaternions          utils.py:270-286
  _absolute_map_dict_to_relative / _relative_..._absolute  run_mapping.py:844-885
  _update_graph's keyframe removal and rewiring            run_mapping.py:907-929
  _update_field_poses                                      run_mapping.py:937-952
  the multi-view keyframe slots with release               run_mapping.py:913-915, 1673-1713

plus the three "not touched" rules of include/ngm_hip.h ngm_fields_repose, which are stricter than the reference.
pytorch3d's matrix_to_quaternion / quaternion_raw_multiply are restated from their public definitions."""
import numpy as np


def quat_mul(a, b):
    """raw Hamilton product, real part first (pytorch3d quaternion_raw_multiply): no standardisation, no normalisation"""
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def matrix_to_quaternion(m, dt=np.float64):
    """pytorch3d.transforms.matrix_to_quaternion on (n, 3, 3): the candidate with the largest |component| of the four
    (first on ties), over 2 max(|component|, 0.1); real part non-negative (standardize_quaternion)"""
    m = np.asarray(m, dt)
    one = dt(1)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i, j] for i in range(3) for j in range(3))
    sq = np.stack((one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22), -1)
    q_abs = np.where(sq > 0, np.sqrt(np.maximum(sq, 0)), dt(0)).astype(dt)
    cand = np.stack((np.stack((q_abs[:, 0] * q_abs[:, 0], m21 - m12, m02 - m20, m10 - m01), -1),
                     np.stack((m21 - m12, q_abs[:, 1] * q_abs[:, 1], m10 + m01, m02 + m20), -1),
                     np.stack((m02 - m20, m10 + m01, q_abs[:, 2] * q_abs[:, 2], m12 + m21), -1),
                     np.stack((m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] * q_abs[:, 3]), -1)), 1).astype(dt)   # (n, 4, 4)
    best = np.argmax(q_abs, -1)
    rows = np.arange(m.shape[0])
    d = dt(2) * np.maximum(q_abs[rows, best], dt(0.1))
    q = (cand[rows, best] / d[:, None]).astype(dt)
    return np.where(q[:, :1] < 0, -q, q)


def affine_inverse(T, dt=np.float64):
    """inverse of (n, 4, 4) affine matrices with last row (0, 0, 0, 1): 3x3 inverse by adjugate and determinant, translation
    -(R^-1 t); no orthonormality assumed (rm.py:870 calls .inverse())"""
    T = np.asarray(T, dt)
    r = lambda i, j: T[:, i, j]
    c00, c01, c02 = r(1, 1) * r(2, 2) - r(1, 2) * r(2, 1), r(1, 2) * r(2, 0) - r(1, 0) * r(2, 2), r(1, 0) * r(2, 1) - r(1, 1) * r(2, 0)
    det = r(0, 0) * c00 + r(0, 1) * c01 + r(0, 2) * c02
    adj = np.stack((c00, r(0, 2) * r(2, 1) - r(0, 1) * r(2, 2), r(0, 1) * r(1, 2) - r(0, 2) * r(1, 1),
                    c01, r(0, 0) * r(2, 2) - r(0, 2) * r(2, 0), r(0, 2) * r(1, 0) - r(0, 0) * r(1, 2),
                    c02, r(0, 1) * r(2, 0) - r(0, 0) * r(2, 1), r(0, 0) * r(1, 1) - r(0, 1) * r(1, 0)), -1)
    with np.errstate(all="ignore"):
        R = (adj / det[:, None]).reshape(-1, 3, 3).astype(dt)
    t = T[:, :3, 3]
    out = np.zeros_like(T)
    out[:, :3, :3] = R
    out[:, :3, 3] = -((R[:, :, 0] * t[:, :1] + R[:, :, 1] * t[:, 1:2]) + R[:, :, 2] * t[:, 2:3])
    out[:, 3, 3] = 1
    return out


def transform_points(points, transforms):
    """utils.py:276-286 (inv=False): R p + t, the products summed left to right"""
    R, t, p = transforms[:, :3, :3], transforms[:, :3, 3], points
    return ((R[:, :, 0] * p[:, :1] + R[:, :, 1] * p[:, 1:2]) + R[:, :, 2] * p[:, 2:3]) + t


def transform_quaternions(quaternions, transforms, dt):
    """utils.py:270-273"""
    return quat_mul(matrix_to_quaternion(transforms[:, :3, :3], dt), quaternions)


def absolute_to_relative(positions, orientations, kf_ids, kf2ws, dt=np.float64):
    """rm.py:864-885"""
    w2kfs = affine_inverse(np.asarray(kf2ws, dt)[kf_ids], dt)
    p, q = np.asarray(positions, dt), np.asarray(orientations, dt)
    return transform_points(p, w2kfs).astype(dt), transform_quaternions(q, w2kfs, dt).astype(dt)


def relative_to_absolute(positions, orientations, kf_ids, kf2ws, dt=np.float64):
    """rm.py:844-862"""
    T = np.asarray(kf2ws, dt)[kf_ids]
    p, q = np.asarray(positions, dt), np.asarray(orientations, dt)
    return transform_points(p, T).astype(dt), transform_quaternions(q, T, dt).astype(dt)


def touched_rows(anchor, prev, new, num=None):
    """The rows ngm_fields_repose moves: below the count in force, anchor inside the tables, both pose rows finite and not
    bitwise equal (the tables as float32, which is what the device holds)."""
    anchor = np.asarray(anchor)
    prev32, new32 = np.asarray(prev, np.float32), np.asarray(new, np.float32)
    n = anchor.shape[0] if num is None else min(max(int(num), 0), anchor.shape[0])
    ok = (np.arange(anchor.shape[0]) < n) & (anchor >= 0) & (anchor < prev32.shape[0])
    a = np.where(ok, anchor, 0)
    if prev32.shape[0] == 0:
        return np.zeros_like(ok)
    finite = np.isfinite(prev32[a]).all((1, 2)) & np.isfinite(new32[a]).all((1, 2))
    same = (prev32[a].view(np.uint32) == new32[a].view(np.uint32)).all((1, 2))
    return ok & finite & ~same


def repose(positions, orientations, anchor, prev, new, dt=np.float64, num=None):
    """_update_field_poses (rm.py:937-952) for the touched rows; every other row is returned as given.  Returns (positions,
    orientations, touched mask)."""
    p, q = np.array(positions, dt), np.array(orientations, dt)
    m = touched_rows(anchor, prev, new, num)
    if m.any():
        a = np.asarray(anchor)[m]
        rp, rq = absolute_to_relative(p[m], q[m], a, prev, dt)
        p[m], q[m] = relative_to_absolute(rp, rq, a, new, dt)
    return p, q, m


def errors(pos, quat, ref_pos, ref_quat):
    """worst absolute error of positions, and of quaternions up to sign: min(|a - b|, |a + b|) per quaternion"""
    pos, quat = np.asarray(pos, np.float64), np.asarray(quat, np.float64)
    ep = float(np.abs(pos - ref_pos).max()) if pos.size else 0.0
    eq = float(np.minimum(np.abs(quat - ref_quat).max(-1), np.abs(quat + ref_quat).max(-1)).max()) if quat.size else 0.0
    return ep, eq


def rot(axis, angle):
    """rotation matrix (float64) about a coordinate axis or a 3-vector"""
    v = np.eye(3)[axis] if isinstance(axis, int) else np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


# ---------------------------------------------------------------------------------------------- rewiring (rm.py:899-926)
def rewire(kf_ids, prev_kfs, removed_kfs, current_keyframe=None):
    """kf_ids after _update_graph's removal loop: prev_kfs the keyframes before the update, removed_kfs those the new graph
    lacks, current_keyframe the frame id added by this update (or None)"""
    kf_ids = np.array(kf_ids)
    prev_kfs, removed_kfs = set(prev_kfs), set(removed_kfs)
    new_kfs = prev_kfs - removed_kfs
    if current_keyframe is not None:
        new_kfs.add(current_keyframe)
    for removed in sorted(removed_kfs):
        kf_after = min([i for i in new_kfs if i >= removed], default=None)
        kf_before = max([i for i in new_kfs if removed >= i], default=None)
        new_anchor = kf_after if kf_after in prev_kfs else kf_before
        kf_ids[kf_ids == removed] = new_anchor
    return kf_ids


# ---------------------------------------------------------------------------------------------- keyframe slots with release
class ReferenceKeyframesRelease:
    """_init_mv_training_data / _update_mv_training_data (rm.py:1673-1713) with _update_graph's release (rm.py:913-915) on
    numpy arrays.  One correction: the reference appends the removed FRAME ID to its free list (rm.py:914); the slot is what
    is free, and the slot is appended here."""

    def __init__(self, capacity, keyframes_only=False):
        self.free = list(range(capacity))
        self.keyframes_only = keyframes_only
        if not keyframes_only:
            self.free.pop(0)                                  # 0 will be used for current frame
        self.frame_id = np.full(capacity, -1, np.int64)
        self.images, self.poses = {}, {}                      # slot -> image tag, frame id -> pose

    def remove(self, frame_id):
        first = 0 if self.keyframes_only else 1               # slot 0 is the current frame's, never a keyframe's
        slot = first + int(np.nonzero(self.frame_id[first:] == frame_id)[0][0])
        self.free.append(slot)
        self.frame_id[slot] = -1

    def update(self, current=None, keyframe=None):
        """current: (frame_id, image, c2w) or None (pose missing); keyframe: (frame_id, image, c2w) or None"""
        if not self.keyframes_only:
            if current is None:
                self.frame_id[0] = -1
            else:
                self.images[0], self.frame_id[0] = current[1], current[0]
                self.poses[current[0]] = current[2]
        if keyframe is not None:
            if len(self.free) == 0:
                raise ValueError("Maximum number of keyframes reached.")
            slot = self.free.pop(0)
            self.images[slot], self.frame_id[slot] = keyframe[1], keyframe[0]
            self.poses[keyframe[0]] = keyframe[2]
        return self.lists()

    def lists(self):
        mask = self.frame_id != -1
        self.frame_cid_to_ncid = np.arange(len(mask))[mask]
        self.c_c2w = [self.poses[int(f)] for f in self.frame_id[mask]]
        return self.frame_cid_to_ncid, self.c_c2w
