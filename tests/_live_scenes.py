"""The RGB-D frames and field maps of tests/test_gpu_live_iteration.py, generated on the CPU from seeds (numpy), so that
tests/test_live_iteration_cpu.py can hold every one of them to the margin condition without a GPU: in float64 no field's
observed / not-observed decision is closer to its threshold than 1e-3 (relative to r for the AABB comparisons, to r^2 for
the segment test), about a hundred times the float32 rounding of these scenes' coordinates (<= 6 m).  Test infrastructure."""
import numpy as np

import _target_live_host as LH

RADIUS = 0.35
NUM_FIELDS = 70             # more than a wave, not a multiple of 64


def camera_params(H, W):
    """(fx, fy, cx, cy) at pixel centre 0"""
    return 0.8 * W, 0.8 * W, W / 2 - 0.5, H / 2 - 0.5


def pose(seed, look_away=False):
    """a camera near the origin looking down -z, turned a little about y (look_away: turned round, +z)"""
    g = np.random.RandomState(1000 + seed)
    a = 0.3 * (g.rand() - 0.5) + (np.pi if look_away else 0.0)
    T = np.eye(4, dtype=np.float32)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    T[:3, 3] = (g.rand(3) - 0.5).astype(np.float32) * np.float32(0.6)
    return T


def field_map(seed, num_fields=NUM_FIELDS, behind=10, aside=10):
    """field centres in the world: most in front of the pose(.) cameras at the frames' depths, the first `behind` behind
    them, the next `aside` far to the side of anything the frames see"""
    g = np.random.RandomState(2000 + seed)
    z = -(1.5 + 4.0 * g.rand(num_fields))
    pos = np.stack([(2 * g.rand(num_fields) - 1) * 0.6 * np.abs(z), (2 * g.rand(num_fields) - 1) * 0.4 * np.abs(z), z], -1)
    pos[:behind, 2] = 1.5 + 2.0 * g.rand(behind)
    pos[behind:behind + aside, 0] += 12.0
    return pos.astype(np.float32)


def frame(H, W, seed, zero_frac=0.3, valid=None):
    """(H, W, 4) float32 RGB-D: depth 2 .. 6 m, a fraction zero_frac of it missing (valid: exactly that many pixels kept)"""
    g = np.random.RandomState(3000 + seed)
    img = g.rand(H, W, 4).astype(np.float32)
    depth = (2.0 + 4.0 * img[..., 3]).astype(np.float32)
    depth[g.rand(H, W) < zero_frac] = 0.0
    if valid is not None:
        keep = g.permutation(H * W)[:valid]
        d = np.zeros(H * W, np.float32)
        d[keep] = np.maximum(depth.reshape(-1)[keep], np.float32(2.0))
        depth = d.reshape(H, W)
    img[..., 3] = depth
    return img


# name -> (H, W, num_points, frame kwargs); the draw is keyed by (SEED, frame number FRAME)
SEED, FRAME = 7, 3
OBSERVE_CASES = {
    "48x64": (48, 64, 500, dict(zero_frac=0.3)),
    "24x32": (24, 32, 64, dict(zero_frac=0.3)),
    "few_valid": (24, 32, 64, dict(valid=40)),
    "all_zero": (24, 32, 64, dict(zero_frac=2.0)),
}
# scene seeds chosen on the CPU (choose_seed below) so that the margin condition holds: tests/test_live_iteration_cpu.py
# re-checks every one
OBSERVE_SEEDS = {"48x64": 0, "24x32": 0, "few_valid": 0, "all_zero": 0}
# the four frames of the one-graph test: 24 x 32, 64 points, frame i drawn with (SEED, frame number i); (scene seed, frame
# kwargs): the second observes nothing (no depth at all), the others more than T / 2 = 6 fields
GRAPH_H, GRAPH_W, GRAPH_POINTS, GRAPH_MAP_SEED = 24, 32, 64, 0
GRAPH_FRAMES = [(100, dict(zero_frac=0.3)), (101, dict(zero_frac=2.0)), (102, dict(zero_frac=0.1)), (103, dict(zero_frac=0.5))]


def graph_frame(i):
    seed, kw = GRAPH_FRAMES[i]
    return dict(rgbd=frame(GRAPH_H, GRAPH_W, seed, **kw), c2w=pose(seed))


def observe_case(name, seed=None):
    H, W, num_points, kw = OBSERVE_CASES[name]
    seed = OBSERVE_SEEDS[name] if seed is None else seed
    return dict(H=H, W=W, num_points=num_points, rgbd=frame(H, W, seed, **kw), c2w=pose(seed), positions=field_map(seed))


def margins(rgbd, c2w, positions, num_points, seed, frame_no):
    """(observed ids in float64, AABB margin / r, segment margin / r^2) for the device's draw of (seed, frame_no)"""
    H, W = rgbd.shape[:2]
    pixels = LH.draw_pixels(rgbd[..., 3], num_points, seed, frame_no)
    return LH.observed_from_pixels(rgbd, c2w, positions, RADIUS, pixels, *camera_params(H, W), dt=np.float64, margins=True)


def choose_seed(name, tries=200):
    for s in range(tries):
        c = observe_case(name, s)
        ids, mb, ms = margins(c["rgbd"], c["c2w"], c["positions"], c["num_points"], SEED, FRAME)
        if mb >= 1e-3 and ms >= 1e-3:
            return s, len(ids)
    raise RuntimeError(name)
