"""The training-target sampler on the device (NeuralGraphRenderer.sample_target_mv_device, include/ngm_hip.h
ngm_target_sample_mv): tied to the torch-draw sampler through its draws= replay (which G11 pins against the reference),
its draws restated on the host (tests/_target_device_host.py), its distribution, determinism and iteration counter, graph
capture (no host synchronisation), padding, rank sharding, edge shapes and a guard-band pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
from gpu_common import DEV, make_renderer  # noqa: E402
import _target_device_host as H  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = dict(encoding="fourier", dim_enc=32, num_layers=1)
TARGET_FIELDS = Rr.Target._fields
PADDED = TARGET_FIELDS + ("count", "frame_cids", "u_xy")


class Scene:
    """map + keyframe store: fields in a box in front of cameras that look down -z (OpenGL), random depth images"""

    def __init__(self, num_fields, num_frames, H=48, W=64, seed=0, store=None, behind=False, radius=1.0):
        g = torch.Generator().manual_seed(seed)
        pos = torch.rand(num_fields, 3, generator=g) * torch.tensor([8.0, 6.0, 5.0]) - torch.tensor([4.0, 3.0, 7.0])
        if behind:
            pos[:, 2] = -pos[:, 2] + 4.0                  # every field behind every camera
        c2w = torch.eye(4).repeat(num_frames, 1, 1)
        c2w[:, :3, 3] = torch.rand(num_frames, 3, generator=g) * 4.0 - 2.0
        ns = num_frames if store is None else store
        rgbd = torch.rand(ns, H, W, 4, generator=g)
        rgbd[..., 3] = 2.0 + 8.0 * rgbd[..., 3]
        self.positions = pos.to(DEV)
        self.c2w = c2w.to(DEV)
        self.rgbd = rgbd.to(DEV).contiguous()
        self.f2s = (torch.arange(num_frames) % ns).to(DEV)
        self.cam = Rr.Camera(W, H, 0.8 * W, 0.8 * W, W / 2 - 0.5, H / 2 - 0.5, pixel_center=0.0)
        self.num_fields, self.radius = num_fields, radius

    @staticmethod
    def g11():
        g = load_golden("g11_target_sampler")
        sc = Scene.__new__(Scene)
        sc.positions, sc.c2w = g["positions"].to(DEV), g["c_c2w"].to(DEV)
        sc.rgbd, sc.f2s = g["nc_rgbd"].to(DEV).contiguous(), g["frame_cid_to_ncid"].to(DEV)
        sc.cam = Rr.Camera(int(g["width"]), int(g["height"]), float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"]),
                           pixel_center=0.0)
        sc.num_fields, sc.radius = int(g["num_fields"]), 1.0
        return sc, g["current_field_ids"].to(DEV), int(g["num_train_fields"]), int(g["num_rays_per_field"])

    def renderer(self):
        r = make_renderer(SMALL, dict(num_samples_coarse=4, num_samples_depth_guided=4, field_radius=self.radius), 1)
        r.set_field_poses(self.positions, torch.zeros(self.num_fields, 4, device=DEV))
        return r

    def cur(self, n, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        return torch.randperm(self.num_fields, generator=g)[:n].to(DEV)

    def device(self, r, cur, T, R, **kw):
        return r.sample_target_mv_device(cur, self.c2w, self.rgbd, self.f2s, T, R, camera=self.cam, **kw)

    def replay(self, r, cur, T, R, draws):
        return r.sample_target_mv(cur, self.c2w, self.rgbd, self.f2s, T, R, camera=self.cam, draws=draws)

    def visibility(self, field_ids, offsets):
        fx, fy, cx, cy, _ = self.cam.get_pinhole_camera_parameters(0.0)
        kf = ops.keyframes_struct(self.c2w.contiguous(), self.rgbd, self.f2s, fx, fy, cx, cy)
        mask, _ = ops.target_visibility(kf, self.positions[field_ids].contiguous(), offsets, self.radius)
        return mask


def assert_replay_equal(sc, r, cur, T, R, **kw):
    t = sc.device(r, cur, T, R, **kw)
    m = t.materialize()
    ref = sc.replay(r, cur, T, R, t.draws())
    for k in TARGET_FIELDS:
        a, b = getattr(m, k), getattr(ref, k)
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k
    return t, m


def assert_padding(t):
    n = int(t.count)
    assert 0 <= n <= t.field_ids.shape[0]
    assert bool((t.field_ids[n:] == -1).all()) and bool((t.field_ids[:n] >= 0).all())
    for k in PADDED:
        if k in ("count", "field_ids"):
            continue
        v = getattr(t, k)[n:]
        assert not bool(v.to(torch.float64).abs().sum()), k
    m = t.materialize()
    for k in TARGET_FIELDS:
        assert getattr(m, k).shape[0] == n, k


# ------------------------------------------------------------------------------------------------ 1. replay
def test_replay_equals_device_g11():
    sc, cur, T, R = Scene.g11()
    r = sc.renderer()
    for it in range(6):
        assert_replay_equal(sc, r, cur, T, R, seed=3, iteration=it)


@pytest.mark.parametrize("case", [(200, 30, 32, 16, 0), (200, 30, 32, 64, 1), (12, 12, 32, 8, 2), (50, 0, 16, 8, 3), (10, 4, 32, 8, 4)])
def test_replay_equals_device_random_scenes(case):
    NF, ncur, T, R, seed = case
    sc = Scene(NF, 20, seed=seed)
    r = sc.renderer()
    cur = sc.cur(ncur, seed)
    seen = 0
    for it in range(4):
        t, m = assert_replay_equal(sc, r, cur, T, R, seed=seed, iteration=it)
        seen += m.field_ids.shape[0]
        assert_padding(t)
    assert seen > 0


# ------------------------------------------------------------------------------------------------ 2. host restatement
@pytest.mark.parametrize("case", ["n_rand", "no_rand", "empty_cur", "few_fields"])
def test_draws_equal_host_restatement(case):
    NF, ncur, T = dict(n_rand=(200, 30, 32), no_rand=(12, 12, 32), empty_cur=(50, 0, 16), few_fields=(10, 4, 32))[case]
    R = 24
    sc = Scene(NF, 16, seed=7)
    r = sc.renderer()
    cur = sc.cur(ncur, 7)
    for seed, it in ((0, 0), (5, 17), (2 ** 40 + 3, 123456)):
        t = sc.device(r, cur, T, R, seed=seed, iteration=it)
        sub_obs, sub_rand, ids = H.draw_fields(cur.cpu().numpy(), NF, T, seed, it)
        if case == "no_rand":
            assert len(sub_rand) == 0 and not np.all(np.diff(ids) > 0)         # the observed draw order, not sorted
        np.testing.assert_array_equal(t.subset_observed.cpu().numpy(), sub_obs)
        np.testing.assert_array_equal(t.subset_random.cpu().numpy(), sub_rand)
        off = H.offsets(seed, it)
        assert np.array_equal(t.offsets.cpu().numpy().view(np.uint32), off.view(np.uint32))
        ids_t = torch.from_numpy(ids).to(DEV)
        mask = sc.visibility(ids_t, torch.from_numpy(off).to(DEV))
        keep = mask.any(-1)
        m = t.materialize()
        np.testing.assert_array_equal(m.field_ids.cpu().numpy(), ids[keep.cpu().numpy()])
        fc, uxy = H.ray_draws(seed, it, ids[keep.cpu().numpy()], R, mask[keep].cpu().numpy())
        d = t.draws()
        np.testing.assert_array_equal(d["frame_cids"].cpu().numpy(), fc)
        assert np.array_equal(d["u_xy"].cpu().numpy().view(np.uint32), uxy.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. distribution
def _chi2_p(obs, exp, dof):
    from scipy import stats
    return float(stats.chi2.sf(float(((obs - exp) ** 2 / exp).sum()), dof))


@pytest.mark.parametrize("seed", [11, 12])
def test_distribution(seed):
    from scipy import stats
    NF, ncur, T, R, N = 60, 20, 16, 64, 2000
    sc = Scene(NF, 12, seed=seed)
    r = sc.renderer()
    cur = sc.cur(ncur, seed)
    n_obs, n_rand = H.plan(ncur, NF, T)
    c_obs = torch.zeros(ncur, dtype=torch.float64, device=DEV)
    c_rand = torch.zeros(NF, dtype=torch.float64, device=DEV)
    o_kf = torch.zeros(NF, sc.c2w.shape[0], dtype=torch.float64, device=DEV)
    e_kf = torch.zeros_like(o_kf)
    u = []
    for it in range(N):
        t = sc.device(r, cur, T, R, seed=seed, iteration=it)
        c_obs.index_add_(0, t.subset_observed, torch.ones(n_obs, dtype=torch.float64, device=DEV))
        c_rand.index_add_(0, t.subset_random, torch.ones(n_rand, dtype=torch.float64, device=DEV))
        m = t.materialize()
        if m.field_ids.shape[0] == 0:
            continue
        mask = sc.visibility(m.field_ids, t.offsets).to(torch.float64)
        e_kf.index_add_(0, m.field_ids, R * mask / mask.sum(-1, keepdim=True))
        fc = t.frame_cids[:m.field_ids.shape[0]]
        o_kf.view(-1).index_add_(0, (m.field_ids[:, None] * sc.c2w.shape[0] + fc).view(-1),
                                 torch.ones(fc.numel(), dtype=torch.float64, device=DEV))
        if it < 200:
            u.append(t.u_xy[:m.field_ids.shape[0]].reshape(-1))
    # observed draw: every current field with probability n_obs / len(cur)
    assert float(c_obs.sum()) == N * n_obs
    assert _chi2_p(c_obs.cpu(), torch.full((ncur,), N * n_obs / ncur, dtype=torch.float64), ncur - 1) > 1e-6
    # random draw: uniform over the fields the observed draw left
    in_cur = torch.zeros(NF, dtype=torch.bool)
    in_cur[cur.cpu()] = True
    p = torch.full((NF,), n_rand / (NF - n_obs), dtype=torch.float64)
    p[in_cur] *= 1.0 - n_obs / ncur
    assert _chi2_p(c_rand.cpu(), N * p, NF - 1) > 1e-6
    # keyframes: uniform over each field's visible keyframes
    o, e = o_kf.cpu(), e_kf.cpu()
    assert float(o[e == 0].sum()) == 0.0
    cells, fields = int((e > 0).sum()), int((e.sum(-1) > 0).sum())
    assert cells - fields > 10
    assert _chi2_p(o[e > 0], e[e > 0], cells - fields) > 1e-6
    uu = torch.cat(u).double().cpu().numpy()
    assert uu.size > 100000 and uu.min() >= 0.0 and uu.max() < 1.0
    assert stats.kstest(uu, "uniform").pvalue > 1e-6


# ------------------------------------------------------------------------------------------------ 4. determinism, counter
def test_determinism_and_counter():
    sc = Scene(200, 20, seed=21)
    r = sc.renderer()
    cur = sc.cur(30, 21)
    a = sc.device(r, cur, 32, 32, seed=4, iteration=9)
    b = sc.device(r, cur, 32, 32, seed=4, iteration=9)
    for k in PADDED:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert r._target_iter_dev is None                      # explicit iterations leave the counter alone
    seq = [sc.device(r, cur, 32, 32, seed=4) for _ in range(3)]
    assert int(r._target_iter_dev) == 3
    for i, t in enumerate(seq):
        e = sc.device(r, cur, 32, 32, seed=4, iteration=i)
        for k in PADDED:
            assert torch.equal(getattr(t, k), getattr(e, k)), (i, k)
    assert int(r._target_iter_dev) == 3
    for other in (sc.device(r, cur, 32, 32, seed=5, iteration=9), sc.device(r, cur, 32, 32, seed=4, iteration=10)):
        assert not torch.equal(other.offsets, a.offsets)
        assert not torch.equal(other.subset_random, a.subset_random) or not torch.equal(other.subset_observed, a.subset_observed)


# ------------------------------------------------------------------------------------------------ 5. graph capture
def test_graph_capture_replays_fresh_iterations():
    sc = Scene(200, 20, seed=31)
    r = sc.renderer()
    cur = sc.cur(30, 31)
    sc.device(r, cur, 32, 64, seed=8)                        # creates the counter (iteration 0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t = sc.device(r, cur, 32, 64, seed=8)
    torch.cuda.synchronize()
    i0 = int(r._target_iter_dev)
    assert i0 == 1                                           # capture records, it does not run
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = {n: getattr(t, n).clone() for n in PADDED}
        e = sc.device(r, cur, 32, 64, seed=8, iteration=i0 + k)
        for n in PADDED:
            assert torch.equal(got[n], getattr(e, n)), (k, n)
    assert int(r._target_iter_dev) == i0 + 3


# ------------------------------------------------------------------------------------------------ 6. padding
def test_padding_rows_and_empty():
    sc = Scene(200, 3, seed=41)
    r = sc.renderer()
    cur = sc.cur(30, 41)
    partial = 0
    for it in range(8):
        t = sc.device(r, cur, 64, 16, seed=1, iteration=it)
        assert_padding(t)
        partial += int(t.count) < t.field_ids.shape[0]
    assert partial > 0                                       # some field unseen by 3 keyframes
    sb = Scene(50, 4, seed=42, behind=True)
    rb = sb.renderer()
    t = sb.device(rb, sb.cur(10, 42), 16, 8, seed=1, iteration=0)
    assert int(t.count) == 0 and t.field_ids.shape[0] == 16
    assert_padding(t)
    m = t.materialize()
    assert m.ijs.shape == (0, 8, 2) and m.rgbds.shape == (0, 8, 4)


# ------------------------------------------------------------------------------------------------ 7. sharding
@pytest.mark.parametrize("W", [2, 3])
def test_sharding(W):
    sc = Scene(200, 20, seed=51)
    r = sc.renderer()
    cur = sc.cur(30, 51)
    for it in range(3):
        full = sc.device(r, cur, 32, 32, seed=6, iteration=it).materialize()
        got = []
        for rank in range(W):
            t = sc.device(r, cur, 32, 32, seed=6, iteration=it, world_size=W, rank=rank)
            assert t.field_ids.shape[0] == min(32, len(range(rank, 200, W)))
            assert_padding(t)
            m = t.materialize()
            sel = full.field_ids % W == rank
            for k in TARGET_FIELDS:
                assert torch.equal(getattr(m, k), getattr(full, k)[sel]), (rank, k)
            got.append(m.field_ids)
        assert torch.equal(torch.sort(torch.cat(got))[0], torch.sort(full.field_ids)[0])


# ------------------------------------------------------------------------------------------------ 8. edge shapes
def _edge_cases():
    sc1 = Scene(100, 1, seed=61)
    r1 = sc1.renderer()
    assert_replay_equal(sc1, r1, sc1.cur(20, 61), 16, 37, seed=2, iteration=0)
    big = Scene(60, 2100, H=24, W=32, seed=62, store=5)           # more keyframes than the LDS list holds
    rb = big.renderer()
    t, m = assert_replay_equal(big, rb, big.cur(20, 62), 16, 8, seed=2, iteration=1)
    assert int(t.count) > 0
    sc = Scene(200, 20, seed=63)
    r = sc.renderer()
    for R in (1, 37, 512):
        assert_replay_equal(sc, r, sc.cur(30, 63), 32, R, seed=3, iteration=R)
    huge = Scene(40000, 20, seed=64)
    rh = huge.renderer()
    cur = huge.cur(1000, 64)
    t, m = assert_replay_equal(huge, rh, cur, 32, 16, seed=9, iteration=5)
    sub_obs, sub_rand, ids = H.draw_fields(cur.cpu().numpy(), 40000, 32, 9, 5)
    np.testing.assert_array_equal(t.subset_observed.cpu().numpy(), sub_obs)
    np.testing.assert_array_equal(t.subset_random.cpu().numpy(), sub_rand)


def test_edge_shapes():
    _edge_cases()


# ------------------------------------------------------------------------------------------------ 9. guard bands
def test_guard_bands():
    from test_gpu_safety import guard_bands
    with guard_bands() as bands:
        sc, cur, T, R = Scene.g11()
        r = sc.renderer()
        assert_replay_equal(sc, r, cur, T, R, seed=3, iteration=0)
        sb = Scene(50, 4, seed=42, behind=True)
        assert_padding(sb.device(sb.renderer(), sb.cur(10, 42), 16, 8, seed=1, iteration=0))
        sp = Scene(200, 3, seed=41)
        assert_padding(sp.device(sp.renderer(), sp.cur(30, 41), 64, 16, seed=1, iteration=0))
        _edge_cases()
        n = bands.check()
    assert n > 20
