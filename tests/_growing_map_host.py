"""Host side of the growing-map tests (tests/test_growing_map_cpu.py, tests/test_gpu_growing_map.py): the counts the grow
sampler computes on the device restated (include/ngm_hip.h ngm_target_sample_mv_grow), the four frames of the one-graph
test over a map that starts with START of its CAPACITY fields and gets the rest between frames 1 and 2, and a host
prediction of the fields every iteration of that run trains -- the observed set (tests/_target_live_host.py), the field draw
(tests/_target_device_host.py) and the keyframe visibility (the oracle's arithmetic, rm.py:1321-1379) -- by which the map
seed of the GPU test is chosen and checked without a GPU.  Test infrastructure."""
import numpy as np
import torch

import _live_scenes as S
import _target_device_host as TH
import _target_live_host as LH
from neural_graph_mapping_amd.keyframes import KeyframeStore
from oracle import ngm_oracle as O

CAPACITY, START = S.NUM_FIELDS, 60          # growth crosses the 64-lane boundary
T, R, SEED, PER_FRAME, GROW_AFTER = 12, 32, 5, 5, 2
# chosen with predict_trained (tests/test_growing_map_cpu.py re-checks it): on this map the host predicts fields >= START
# in TRAINED_NEW_ITERATIONS of the 10 iterations after the growth
MAP_SEED, TRAINED_NEW_ITERATIONS = 0, 8


# ---------------------------------------------------------------------------------------------- the device's counts
def owned(num_fields, world_size, rank):
    return (num_fields - rank + world_size - 1) // world_size if num_fields > rank else 0


def grow_counts(num_current, num_fields, max_current, max_fields, num_train_fields):
    """(nf, nc, n_obs, n_rand) as k_tsmv_draw computes them in the grow variant"""
    nf = min(max(num_fields, 0), max_fields)
    nc = min(max(num_current, 0), min(max_current, nf))
    n_obs = min(num_train_fields // 2, nc)
    return nf, nc, n_obs, max(min(num_train_fields - n_obs, nf - n_obs), 0)


def grow_capacity(max_fields, num_train_fields, world_size=1, rank=0):
    """the host-known rows: min(T, fields rank r owns among max_fields)"""
    return min(min(num_train_fields, max_fields), owned(max_fields, world_size, rank))


# ---------------------------------------------------------------------------------------------- the frames
class GrowFrames:
    """test_gpu_live_iteration.Frames on any device: the four frames, the two keyframes the store starts with, the store's
    update per frame (keyframes 2 -> 3 -> 3 -> 4, all poses moved in place at frame 2)"""

    def __init__(self, map_seed=MAP_SEED, num_fields=CAPACITY, behind=10, aside=10, device="cpu"):
        self.H, self.W, self.device = S.GRAPH_H, S.GRAPH_W, device
        self.positions = S.field_map(map_seed, num_fields, behind, aside)
        self.frames = [S.graph_frame(i) for i in range(len(S.GRAPH_FRAMES))]
        self.start = [(S.frame(self.H, self.W, 200 + k, zero_frac=0.1), S.pose(200 + k)) for k in range(2)]
        self.moved = np.stack([S.pose(300 + k) for k in range(3)])

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def store(self, capacity=6):
        st = KeyframeStore(capacity, self.H, self.W, device=self.device)
        for k, (img, c2w) in enumerate(self.start):
            st.add_keyframe(self.dev(img), 1000 + k, c2w=self.dev(c2w))
        return st

    def advance(self, st, f):
        fr = self.frames[f]
        st.set_current(self.dev(fr["rgbd"]), self.dev(fr["c2w"]), frame_id=f)
        if f in (1, 3):
            st.add_keyframe(self.dev(fr["rgbd"]), f)
        if f == 2:
            st.set_keyframe_poses(self.dev(self.moved))


# ---------------------------------------------------------------------------------------------- the prediction
def visible_fields(field_ids, positions, c_c2w, nc_rgbd, f2s, offsets, radius, H, W):
    """the drawn fields some keyframe sees, in order (rm.py:1321-1379 as the oracle restates it, float32 on the CPU)"""
    cam = O.CameraSpec(W, H, *S.camera_params(H, W))
    pos_w = torch.from_numpy(positions)[torch.from_numpy(field_ids)]
    samples_w = pos_w.unsqueeze(1) + torch.from_numpy(offsets) * radius * 1.0
    samples_c = O.transform_points(samples_w.unsqueeze(-2), c_c2w, inv=True)
    depths = -samples_c[..., 2]
    xi = O.project_points_opengl(samples_c, cam).int()
    valid = (xi[..., 0] >= 0) & (xi[..., 0] < W) & (xi[..., 1] >= 0) & (xi[..., 1] < H)
    cids = torch.arange(c_c2w.shape[0]).expand(len(field_ids), offsets.shape[0], -1)
    kf_depths = torch.zeros_like(depths)
    kf_depths[valid] = nc_rgbd[f2s[cids[valid]], xi[..., 1][valid].long(), xi[..., 0][valid].long(), 3]
    kf_mask = (depths > 0).any(-2) & (depths < kf_depths).any(-2) & valid.any(-2)
    return field_ids[kf_mask.any(-1).numpy()]


def predict_trained(map_seed=MAP_SEED):
    """per iteration of the one-graph run (4 frames x PER_FRAME; START fields in frames 0-1, CAPACITY from frame 2 on): the
    number of fields in force and the ids the host expects the sampler to keep"""
    F = GrowFrames(map_seed)
    st = F.store()
    out, it = [], 0
    for f in range(4):
        F.advance(st, f)
        nf = START if f < GROW_AFTER else CAPACITY
        fr = F.frames[f]
        _, cur = LH.observed_fields(fr["rgbd"], fr["c2w"], F.positions[:nf], S.RADIUS, S.GRAPH_POINTS, S.SEED, f,
                                    *S.camera_params(F.H, F.W))
        m = st.count
        for _ in range(PER_FRAME):
            ids = TH.draw_fields(cur, nf, T, SEED, it)[2]
            kept = visible_fields(ids, F.positions, st.c_c2w[:m], st.nc_rgbd, st.frame_cid_to_ncid[:m], TH.offsets(SEED, it),
                                  S.RADIUS, F.H, F.W) if len(ids) else ids
            out.append((nf, kept))
            it += 1
    return out
