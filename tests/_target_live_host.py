"""Host restatement (numpy) of the observed-field test on the device (csrc/ngm_target.hip k_obs_*, include/ngm_hip.h
ngm_target_observed_fields = NeuralGraphMap._get_observed_fields, rm.py:1642-1670): the Philox keys of the pixel draw, the k
smallest by the same MSB-first radix select, the back-projection, the AABB and the segment-sphere tests -- in float32 in the
kernel's operation order, and in float64 with the margins the GPU scenes are chosen by.  Also the reference's keyframe
bookkeeping (rm.py:1673-1713) restated on lists, for KeyframeStore.  Test infrastructure, no GPU."""
import numpy as np

from _target_device_host import philox_words

STREAM_PIXELS = 0x54470005
f32 = np.float32


# ---------------------------------------------------------------------------------------------- pixel draw
def pixel_keys(depth, seed, frame):
    """(keys uint64, pixel indices) of the pixels with depth != 0: (Philox word 0 of block ctr = pixel) << 32 | pixel"""
    pix = np.nonzero(np.asarray(depth).reshape(-1) != 0)[0].astype(np.uint64)
    w0 = philox_words(seed, frame, pix, STREAM_PIXELS)[0]
    return (w0 << np.uint64(32)) | pix, pix.astype(np.int64)


def k_smallest_radix(keys, k):
    """the k smallest keys (unique) as the kernels select them: 8-bit digits from the top until the bin holding the k-th key
    holds exactly the keys still wanted; then every key whose leading digits are <= the prefix.  Returns the SET, sorted."""
    keys = np.asarray(keys, dtype=np.uint64)
    if len(keys) <= k:
        return np.sort(keys)
    prefix, shift, rem = 0, 64, k
    while True:
        shift -= 8
        live = keys if shift == 56 else keys[(keys >> np.uint64(shift + 8)) == np.uint64(prefix)]
        hist = np.bincount(((live >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        cum, b = 0, 0
        while b < 255 and cum + hist[b] < rem:
            cum += hist[b]
            b += 1
        prefix, rem = (prefix << 8) | b, rem - cum
        if hist[b] == rem or shift == 0:
            break
    return np.sort(keys[(keys >> np.uint64(shift)) <= np.uint64(prefix)])


def draw_pixels(depth, num_points, seed, frame):
    """the chosen linear pixel indices, ascending (the device's order is unspecified)"""
    keys, _ = pixel_keys(depth, seed, frame)
    sel = k_smallest_radix(keys, num_points)
    return np.sort((sel & np.uint64(0xFFFFFFFF)).astype(np.int64))


# ---------------------------------------------------------------------------------------------- field test
def _world_to_cam(T, pos, dt):
    """csrc/ngm_target.hip world_to_cam: R^T (p - t), products summed left to right"""
    T = np.asarray(T, dtype=dt).reshape(16)
    p = np.asarray(pos, dtype=dt)
    dx, dy, dz = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
    return np.stack([(T[0] * dx + T[4] * dy) + T[8] * dz, (T[1] * dx + T[5] * dy) + T[9] * dz,
                     (T[2] * dx + T[6] * dy) + T[10] * dz], -1)


def back_project(rgbd, pixels, fx, fy, cx, cy, dt=f32):
    """camera.py:374-390 (OpenGL) for the given linear pixel indices"""
    H, W = rgbd.shape[:2]
    pixels = np.asarray(pixels, dtype=np.int64)
    r, c = pixels // W, pixels % W
    d = np.asarray(rgbd, dtype=f32)[..., 3].reshape(-1)[pixels].astype(dt)
    x = ((c.astype(dt) - dt(cx)) * d) / dt(fx)
    y = ((-(r.astype(dt) - dt(cy))) * d) / dt(fy)
    return np.stack([x, y, -d], -1)


def observed_from_pixels(rgbd, c2w, positions, radius, pixels, fx, fy, cx, cy, dt=f32, margins=False):
    """observed field ids (ascending) for the chosen pixels; margins=True also returns, relative to r resp. r^2, the smallest
    distance of an AABB comparison from its bound and of max over points of (r^2 - d^2) from 0, over all fields"""
    positions = np.asarray(positions, dtype=f32)
    if len(pixels) == 0:
        return (np.zeros(0, np.int64), np.inf, np.inf) if margins else np.zeros(0, np.int64)
    pts = back_project(rgbd, pixels, fx, fy, cx, cy, dt)
    lo, hi = pts.min(0), pts.max(0)
    c = _world_to_cam(np.asarray(c2w, dtype=f32), positions, dt)
    r = dt(radius)
    gaps = np.concatenate([hi[None] - (c - r), (c + r) - lo[None]], -1)          # >= 0 everywhere: the AABBs meet
    in_box = (gaps >= 0).all(-1)
    sq = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]
    sq = np.where(sq == 0, dt(1.0), sq)
    dot = (c[:, None, 0] * pts[None, :, 0] + c[:, None, 1] * pts[None, :, 1]) + c[:, None, 2] * pts[None, :, 2]
    t = np.minimum(np.maximum(dot / sq[None], dt(0.0)), dt(1.0))
    e = c[:, None, :] - pts[None] * t[..., None]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    slack = (r * r - d2).max(-1)                                                  # >= 0: some segment crosses the sphere
    ids = np.nonzero(in_box & (slack >= 0))[0].astype(np.int64)
    if not margins:
        return ids
    return ids, float(np.abs(gaps).min() / r), float(np.abs(slack).min() / (r * r))


def observed_fields(rgbd, c2w, positions, radius, num_points, seed, frame, fx, fy, cx, cy, dt=f32):
    """(pixels ascending, observed ids ascending)"""
    pixels = draw_pixels(np.asarray(rgbd)[..., 3], num_points, seed, frame)
    return pixels, observed_from_pixels(rgbd, c2w, positions, radius, pixels, fx, fy, cx, cy, dt)


# ---------------------------------------------------------------------------------------------- keyframe bookkeeping
class ReferenceKeyframes:
    """_init_mv_training_data / _update_mv_training_data (rm.py:1673-1713) on numpy arrays; the pose list is the current
    pose (when tracked) followed by the keyframes' own poses"""

    def __init__(self, capacity, keyframes_only=False):
        self.free = list(range(capacity))
        self.keyframes_only = keyframes_only
        if not keyframes_only:
            self.free.pop(0)                                  # 0 will be used for current frame
        self.frame_id = np.full(capacity, -1, np.int64)
        self.images, self.poses = {}, {}                      # slot -> image tag, frame id -> pose

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
        mask = self.frame_id != -1
        self.frame_cid_to_ncid = np.arange(len(mask))[mask]
        self.c_c2w = [self.poses[int(f)] for f in self.frame_id[mask]]
        return self.frame_cid_to_ncid, self.c_c2w
