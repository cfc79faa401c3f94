"""One captured training graph across frames and keyframes: the observed-field test on the device
(NeuralGraphRenderer.observed_fields_device, include/ngm_hip.h ngm_target_observed_fields) against its host restatement
(tests/_target_live_host.py) and the reference's recorded result (G26); the sampler with its counts in device memory
(sample_target_mv_device(current_count=, num_frames=), ngm_target_sample_mv_live) bit for bit against the existing sampler;
capture_training over fixed-capacity buffers (KeyframeStore) replayed across frames against the existing per-frame path; the
per-field training-iteration counts; guard bands; two ranks."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from conftest import load_golden  # noqa: E402
from gpu_common import DEV, make_renderer  # noqa: E402
import _live_scenes as S  # noqa: E402
import _target_live_host as LH  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from neural_graph_mapping_amd.keyframes import KeyframeStore  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = dict(encoding="fourier", dim_enc=32, num_layers=1)
M1 = dict(encoding="fourier", dim_enc=64, num_layers=2)
HASH = dict(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
NETS = {"m1": M1, "hash": HASH}
LOSS_KEYS = ("combined", "termination", "photometric_l1", "depth_huber", "freespace", "tsdf")
TARGET_FIELDS = Rr.Target._fields
PADDED = TARGET_FIELDS + ("count", "frame_cids", "u_xy", "offsets")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def camera(H, W):
    return Rr.Camera(W, H, *S.camera_params(H, W), pixel_center=0.0)


def renderer(positions, fkw=SMALL, seed=0, trained=False, radius=S.RADIUS):
    """a renderer over the map `positions` (numpy (N, 3)); trained: oracle-initialised parameters, as the iteration tests use"""
    n = positions.shape[0]
    params = O.init_params(O.FieldSpec(**fkw), n, seed=seed, sigma=3.0) if trained else None
    r = make_renderer(fkw, dict(num_samples_coarse=4, num_samples_depth_guided=4, field_radius=radius), n, params)
    quat = torch.zeros(n, 4, device=DEV)
    quat[:, 0] = 1.0
    r.set_field_poses(dev(positions), quat)
    return r


def observe(r, c, seed=S.SEED, frame=S.FRAME, **kw):
    H, W = c["rgbd"].shape[:2]
    ids, count = r.observed_fields_device(dev(c["rgbd"]), dev(c["c2w"]), num_points=c["num_points"], seed=seed, frame=frame,
                                          camera=camera(H, W), **kw)
    return ids, count, r.last_observed["pixels"], r.last_observed["num_used"]


# ------------------------------------------------------------------------------------------------ 1. observed fields
@pytest.mark.parametrize("name", list(S.OBSERVE_CASES))
def test_observed_fields_equal_host_restatement(name):
    c = S.observe_case(name)
    H, W = c["H"], c["W"]
    r = renderer(c["positions"])
    ids, count, pixels, used = observe(r, c)
    px_host, ids_host = LH.observed_fields(c["rgbd"], c["c2w"], c["positions"], S.RADIUS, c["num_points"], S.SEED, S.FRAME,
                                           *S.camera_params(H, W))
    n, u = int(count), int(used)
    valid = int((c["rgbd"][..., 3] != 0).sum())
    assert ids.shape == (S.NUM_FIELDS,) and ids.dtype == torch.int64 and count.dtype == torch.int32
    assert pixels.shape == (c["num_points"],) and u == min(c["num_points"], valid) == len(px_host)
    np.testing.assert_array_equal(np.sort(pixels[:u].cpu().numpy()), px_host)          # the SET; the order is unspecified
    assert bool((pixels[u:] == -1).all())
    np.testing.assert_array_equal(ids[:n].cpu().numpy(), ids_host)                      # ascending, exactly the host's
    assert n == len(ids_host) and bool((ids[n:] == -1).all())
    if name == "all_zero":
        assert n == 0 and u == 0
    if name == "48x64":
        assert valid > 4 * 256 and n > 6               # several workgroups; some fields left out, some observed
        behind_or_aside = set(range(20))
        assert not behind_or_aside & set(ids[:n].tolist())


def test_observed_fields_g26_through_draws():
    import scene
    g = load_golden("g26_observed_fields")
    img = scene.sv_frame(int(g["frame_seed"])).to(DEV).contiguous()
    r = renderer(g["positions"].numpy(), radius=float(g["field_radius"]))
    cam = Rr.Camera(scene.SV_W, scene.SV_H, scene.SV_FX, scene.SV_FY, scene.SV_CX, scene.SV_CY, pixel_center=0.0)
    px = g["d_pixels"].to(DEV).long().contiguous()
    ids, count = r.observed_fields_device(img, g["c2w"].to(DEV), num_points=int(g["num_points"]), frame=0, camera=cam,
                                          draws=dict(pixels=px))
    n = int(count)
    assert torch.equal(ids[:n].cpu(), g["o_field_ids"]) and bool((ids[n:] == -1).all())
    assert torch.equal(r.last_observed["pixels"], px) and int(r.last_observed["num_used"]) == int(g["num_points"])
    # the device's own draw on the same frame: 500 distinct valid pixels of 64 000 (hundreds of workgroups)
    ids2, count2 = r.observed_fields_device(img, g["c2w"].to(DEV), num_points=500, seed=1, frame=0, camera=cam)
    own = r.last_observed["pixels"].cpu().numpy()
    host = LH.draw_pixels(img[..., 3].cpu().numpy(), 500, 1, 0)
    np.testing.assert_array_equal(np.sort(own), host)


def test_observed_fields_determinism_and_counter():
    c = S.observe_case("24x32")
    r = renderer(c["positions"])
    a = observe(r, c)
    b = observe(r, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.sort(a[2])[0], torch.sort(b[2])[0])
    assert r._observe_frame_dev is None                    # explicit frames leave the counter alone
    seq = [tuple(t.clone() for t in observe(r, c, frame=None)) for _ in range(3)]
    assert int(r._observe_frame_dev) == 3
    for i, t in enumerate(seq):
        e = observe(r, c, frame=i)
        assert torch.equal(t[0], e[0]) and torch.equal(t[1], e[1]) and torch.equal(torch.sort(t[2])[0], torch.sort(e[2])[0]), i
    assert int(r._observe_frame_dev) == 3
    assert not torch.equal(torch.sort(seq[0][2])[0], torch.sort(seq[1][2])[0])
    # out=: written in place
    ids_buf, cnt_buf = torch.full((S.NUM_FIELDS,), -5, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ids, cnt = observe(r, c, out=(ids_buf, cnt_buf))[:2]
    assert ids.data_ptr() == ids_buf.data_ptr() and cnt.data_ptr() == cnt_buf.data_ptr() and torch.equal(ids_buf, a[0])


@pytest.mark.parametrize("name", ["24x32", "few_valid"])
def test_observed_fields_draw_over_64_frames(name):
    c = S.observe_case(name)
    r = renderer(c["positions"])
    depth = c["rgbd"][..., 3].reshape(-1)
    valid = int((depth != 0).sum())
    px, used = [], []
    for f in range(64):
        _, _, p, u = observe(r, c, frame=f)
        px.append(p)
        used.append(u)
    px, used = torch.stack(px).cpu().numpy(), torch.cat(used).cpu().numpy()
    want = min(c["num_points"], valid)
    assert (used == want).all()
    for f in range(64):
        chosen = px[f, :want]
        assert len(np.unique(chosen)) == want and (chosen >= 0).all() and (depth[chosen] != 0).all(), f
        assert (px[f, want:] == -1).all()
    if name == "24x32":
        assert len({tuple(np.sort(p)) for p in px}) == 64          # every frame draws its own subset


# ------------------------------------------------------------------------------------------------ 2. live sampler
class LiveScene:
    """test_gpu_target_device.Scene's map and keyframes (N fields, 16 keyframes) with fixed-capacity input buffers whose tails
    hold valid but different values: other fields' ids, the other (finite, field-seeing) poses, store index 0"""

    def __init__(self, N=40, frames=16, seed=3):
        from test_gpu_target_device import Scene
        self.sc = Scene(N, frames, H=24, W=32, seed=seed)
        g = torch.Generator().manual_seed(77)
        self.perm = torch.randperm(N, generator=g).to(DEV)
        self.N, self.frames = N, frames

    def buffers(self, n, m):
        cur = self.perm.clone()                                        # [n:] other fields' ids
        c2w = self.sc.c2w.clone()                                      # [m:] the other keyframes' poses
        f2s = self.sc.f2s.clone()
        f2s[m:] = 0
        cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
        nf = torch.tensor([m], dtype=torch.int32, device=DEV)
        return cur, c2w, f2s, cnt, nf


@pytest.mark.parametrize("W", [1, 2, 3])
def test_live_sampler_equals_existing_sampler_bitwise(W):
    N, T, R = 40, 12, 32
    ls = LiveScene(N)
    sc = ls.sc
    r = sc.renderer()
    it = 0
    for n in (0, 1, 5, 6, 7, 40):
        for m in (1, 2, 5, 16):
            cur, c2w, f2s, cnt, nf = ls.buffers(n, m)
            for rank in range(W):
                it += 1
                live = r.sample_target_mv_device(cur, c2w, sc.rgbd, f2s, T, R, camera=sc.cam, seed=9, iteration=it, world_size=W,
                                                 rank=rank, current_count=cnt, num_frames=nf)
                ref = r.sample_target_mv_device(cur[:n].contiguous(), c2w[:m].contiguous(), sc.rgbd, f2s[:m].contiguous(), T, R,
                                                camera=sc.cam, seed=9, iteration=it, world_size=W, rank=rank)
                what = (n, m, W, rank)
                assert isinstance(live, Rr.LiveDeviceTarget) and isinstance(live, Rr.DeviceTarget)
                for k in PADDED:
                    a, b = getattr(live, k), getattr(ref, k)
                    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (what, k)
                n_obs, n_rand, cap = K.target_sample_mv_plan(n, N, T, R, W, rank)
                assert int(live.num_observed) == n_obs == ref.subset_observed.shape[0] and int(live.num_random) == n_rand
                assert live.field_ids.shape[0] == cap
                assert torch.equal(live.subset_observed[:n_obs], ref.subset_observed), what
                assert torch.equal(live.subset_random[:n_rand], ref.subset_random), what
                assert bool((live.subset_observed[n_obs:] == -1).all()) and bool((live.subset_random[n_rand:] == -1).all()), what
                assert live.subset_observed.shape[0] == min(T // 2, N) and live.subset_random.shape[0] == min(T, N)
                if W == 1:
                    dl, dr = live.draws(), ref.draws()
                    for k in dr:
                        assert torch.equal(dl[k], dr[k]), (what, k)
                ml, mr = live.materialize(), ref.materialize()
                for k in TARGET_FIELDS:
                    assert torch.equal(getattr(ml, k), getattr(mr, k)), (what, k)
    with pytest.raises(ValueError, match="go together"):
        r.sample_target_mv_device(cur, c2w, sc.rgbd, f2s, T, R, camera=sc.cam, iteration=0, current_count=cnt)


# ------------------------------------------------------------------------------------------------ 3. + 4. one graph across frames
def state(r):
    s = {}
    for k, v in r._model.all_fields_params.items():
        s["param " + k] = v.clone()
    for k, st in r._optim_state.items():
        s["exp_avg " + k], s["exp_avg_sq " + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    if r._model.lp_fields_params is not None:
        for k, v in r._model.lp_fields_params.items():
            s["lp " + k] = v.clone()
    return s


def assert_losses_equal(a, b, what):
    for k in LOSS_KEYS:
        assert torch.equal(a[k], b[k]) or (bool(torch.isnan(a[k])) and bool(torch.isnan(b[k]))), (what, k, a[k], b[k])


class Frames:
    """the four frames of the one-graph test (tests/_live_scenes.py) and the keyframes the store starts with"""
    T, R, SEED, PER_FRAME = 12, 32, 5, 5

    def __init__(self, num_fields=S.NUM_FIELDS, behind=10, aside=10):
        self.H, self.W = S.GRAPH_H, S.GRAPH_W
        self.cam = camera(self.H, self.W)
        self.positions = S.field_map(S.GRAPH_MAP_SEED, num_fields, behind, aside)
        self.frames = [S.graph_frame(i) for i in range(len(S.GRAPH_FRAMES))]
        self.start = [(S.frame(self.H, self.W, 200 + k, zero_frac=0.1), S.pose(200 + k)) for k in range(2)]
        self.moved = np.stack([S.pose(300 + k) for k in range(3)])          # new poses of the three keyframes held at frame 2

    def store(self, capacity=6):
        st = KeyframeStore(capacity, self.H, self.W, device=DEV)
        for k, (img, c2w) in enumerate(self.start):
            st.add_keyframe(dev(img), 1000 + k, c2w=dev(c2w))
        return st

    def advance(self, st, f):
        """the store's update at frame f: keyframes 2 -> 3 -> 3 -> 4, all poses moved in place at frame 2"""
        fr = self.frames[f]
        st.set_current(dev(fr["rgbd"]), dev(fr["c2w"]), frame_id=f)
        if f in (1, 3):
            st.add_keyframe(dev(fr["rgbd"]), f)
        if f == 2:
            st.set_keyframe_poses(dev(self.moved))


@pytest.mark.parametrize("net", ["m1", "hash"])
def test_one_graph_across_frames_and_keyframes(net):
    F = Frames()
    N, T, R, SEED = S.NUM_FIELDS, F.T, F.R, F.SEED
    ra, rb = renderer(F.positions, NETS[net], trained=True), renderer(F.positions, NETS[net], trained=True)
    ra.track_training_iterations = True
    start = state(ra)
    st = F.store()
    ids_buf = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    cnt_buf = torch.zeros(1, dtype=torch.int32, device=DEV)
    pose_buf = torch.eye(4, device=DEV)
    tally = torch.zeros(N, dtype=torch.int64)
    step, graph, it = None, None, 0
    observed, kept, frames_in_store = [], [], []
    for f in range(4):
        F.advance(st, f)
        pose_buf.copy_(dev(F.frames[f]["c2w"]))               # the pose is device memory, updated in place
        ra.observed_fields_device(st.nc_rgbd[0], pose_buf, num_points=S.GRAPH_POINTS, seed=S.SEED, frame=f, out=(ids_buf, cnt_buf),
                                  camera=F.cam)
        if step is None:
            step = ra.capture_training(ids_buf, st.c_c2w, st.nc_rgbd, st.frame_cid_to_ncid, T, R, seed=SEED, camera=F.cam,
                                       current_count=cnt_buf, num_frames=st.num_frames)
            graph = step.graph
            assert isinstance(graph, torch.cuda.CUDAGraph) and isinstance(step.target, Rr.LiveDeviceTarget)
            assert ra._step == 0 and int(ra._target_iter_dev) == 0
            assert all(torch.equal(v, start[k]) for k, v in state(ra).items()), "capture_training trains nothing by itself"
        n, m = int(cnt_buf), st.count
        assert m == int(st.num_frames)
        observed.append(n)
        frames_in_store.append(m)
        # reference: the existing sampler and iteration on tensors of this frame's shapes
        cur = ids_buf[:n].clone()
        c2w, f2s = st.c_c2w[:m].clone(), st.frame_cid_to_ncid[:m].clone()
        for _ in range(F.PER_FRAME):
            la = step()
            assert step.graph is graph
            k = int(step.target.count)
            kept.append(k)
            tally[step.target.field_ids[:k].cpu()] += 1
            la = {q: la[q].clone() for q in LOSS_KEYS}
            t = rb.sample_target_mv_device(cur, c2w, st.nc_rgbd, f2s, T, R, camera=F.cam, seed=SEED, iteration=it)
            assert int(t.count) == k and torch.equal(t.field_ids, step.target.field_ids), (f, it)
            lb = rb.optimization_iteration(t, seed=SEED)
            assert_losses_equal(la, lb, (f, it))
            it += 1
    torch.cuda.synchronize()
    assert frames_in_store == [3, 4, 4, 5]                             # the current frame + 2 -> 3 -> 3 -> 4 keyframes
    assert observed[1] == 0 and max(observed) > T // 2 and len(set(observed)) >= 3, observed
    assert max(kept) > 0 and len(set(kept)) > 1, kept
    sa, sb = state(ra), state(rb)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert [k for k in sa if not torch.equal(sa[k], start[k])], "nothing was trained"
    assert int(ra._target_iter_dev) == 20 and ra._step == 20 == int(ra._step_dev) == rb._step == int(rb._step_dev)
    # 4. the per-field iteration counts, kept on the device by the graph
    ti = ra._global_map_dict["training_iterations"]
    assert ti.dtype == torch.int64 and ti.shape == (N,) and torch.equal(ti.cpu(), tally) and int(tally.sum()) == sum(kept)
    assert torch.equal(ra.get_field_ids(2).cpu(), torch.where(tally >= 2)[0])
    assert torch.equal(ra.get_field_ids().cpu(), torch.arange(N))
    assert "training_iterations" not in rb._global_map_dict              # flag off: nothing kept, nothing launched
    # the graph reads its inputs in place: another tensor at replay is refused on the host
    ra._global_map_dict["training_iterations"] = ti.clone()
    with pytest.raises(RuntimeError, match="capture again"):
        step()


def _profiled_launches():
    import ctypes as C
    out = {}
    for k in K.KERNEL_IDS:
        n = C.c_int64(0)
        K.check(K.lib().ngm_profile_read(K.KERNEL_IDS[k], None, C.byref(n)), "ngm_profile_read")
        out[k] = n.value
    return out


def test_training_iteration_counts_plain_and_device_targets(monkeypatch):
    ls = LiveScene(40)
    sc = ls.sc
    calls = []
    real = ops.field_counts_add
    monkeypatch.setattr(ops, "field_counts_add", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    launches = {}
    for flag in (False, True):
        r = renderer(sc.positions.cpu().numpy(), SMALL, trained=True, radius=1.0)
        r.track_training_iterations = flag
        cur = ls.perm[:7].contiguous()
        tally = torch.zeros(40, dtype=torch.int64)
        del calls[:]
        K.lib().ngm_profile_enable(1)
        K.lib().ngm_profile_reset()
        try:
            for i in range(3):                                         # a DeviceTarget: the counted step
                t = r.sample_target_mv_device(cur, sc.c2w, sc.rgbd, sc.f2s, 12, 16, camera=sc.cam, seed=2, iteration=i)
                r.optimization_iteration(t, seed=2)
                tally[t.field_ids[:int(t.count)].cpu()] += 1
            for i in range(3, 5):                                      # a plain Target
                m = r.sample_target_mv_device(cur, sc.c2w, sc.rgbd, sc.f2s, 12, 16, camera=sc.cam, seed=2, iteration=i).materialize()
                r.optimization_iteration(m, seed=2)
                tally[m.field_ids.cpu()] += 1
            r.optimization_iteration(m, seed=2, update=False)          # no update: not a training iteration
            launches[flag] = _profiled_launches()
        finally:
            K.lib().ngm_profile_enable(0)
        if flag:
            assert len(calls) == 5                                     # exactly one more launch per update=True iteration
            assert torch.equal(r._global_map_dict["training_iterations"].cpu(), tally) and int(tally.sum()) > 0
            assert torch.equal(r.get_field_ids(2).cpu(), torch.where(tally >= 2)[0])
        else:
            assert not calls and "training_iterations" not in r._global_map_dict
            assert int(r.get_field_ids(1).numel()) == 0 and bool((r._global_map_dict["training_iterations"] == 0).all())
    assert launches[False] == launches[True] and sum(launches[False].values()) > 0      # every other launch unchanged


def test_field_counts_add_kernel():
    ti = torch.zeros(300, dtype=torch.int64, device=DEV)
    ids = torch.tensor([5, 299, -1, 0, 300, 7, 2 ** 40, -9] + list(range(10, 290)), dtype=torch.int64, device=DEV)
    ops.field_counts_add(ids, None, ti, 300)
    want = torch.zeros(300, dtype=torch.int64)
    want[[5, 299, 0, 7] + list(range(10, 290))] += 1
    assert torch.equal(ti.cpu(), want)
    cnt = torch.tensor([6], dtype=torch.int32, device=DEV)
    ops.field_counts_add(ids, cnt, ti, 300)
    want[[5, 299, 0, 7]] += 1
    assert torch.equal(ti.cpu(), want)
    ops.field_counts_add(ids, torch.tensor([0], dtype=torch.int32, device=DEV), ti, 300)
    ops.field_counts_add(ids, torch.tensor([10 ** 6], dtype=torch.int32, device=DEV), ti[:8], 8)      # count clamped to the rows
    want[[5, 0, 7]] += 1
    assert torch.equal(ti.cpu(), want)


# ------------------------------------------------------------------------------------------------ 5. guard bands
def test_guard_bands():
    from test_gpu_safety import guard_bands
    with guard_bands() as bands:
        # observed fields: every case, caller-owned outputs included
        for name in S.OBSERVE_CASES:
            c = S.observe_case(name)
            r = renderer(c["positions"])
            ids_buf = torch.zeros(S.NUM_FIELDS, dtype=torch.int64, device=DEV)
            cnt_buf = torch.zeros(1, dtype=torch.int32, device=DEV)
            rgbd = torch.zeros(c["H"], c["W"], 4, device=DEV)
            rgbd.copy_(dev(c["rgbd"]))
            pose = torch.zeros(4, 4, device=DEV)
            pose.copy_(dev(c["c2w"]))
            r.observed_fields_device(rgbd, pose, num_points=c["num_points"], seed=S.SEED, frame=S.FRAME, out=(ids_buf, cnt_buf),
                                     camera=camera(c["H"], c["W"]))
            sub = torch.zeros(c["num_points"], dtype=torch.int64, device=DEV)
            sub.copy_(r.last_observed["pixels"])
            r.observed_fields_device(rgbd, pose, num_points=c["num_points"], frame=0, out=(ids_buf, cnt_buf), camera=camera(c["H"], c["W"]),
                                     draws=dict(pixels=sub))
        # live sampler over banded fixed-capacity buffers, counts at and inside the maxima, + the counts kernel
        ls = LiveScene(40)
        sc = ls.sc
        r = sc.renderer()
        r.track_training_iterations = True
        for n, m in ((0, 1), (7, 5), (40, 16)):
            cur, c2w, f2s, cnt, nf = ls.buffers(n, m)
            bufs = []
            for t in (cur, c2w, f2s, cnt, nf, sc.rgbd, sc.positions):
                b = torch.zeros(tuple(t.shape), dtype=t.dtype, device=DEV)
                b.copy_(t)
                bufs.append(b)
            cur, c2w, f2s, cnt, nf, rgbd, pos = bufs
            r.set_field_poses(pos, torch.zeros(40, 4, device=DEV))
            for W, rank in ((1, 0), (3, 2)):
                t = r.sample_target_mv_device(cur, c2w, rgbd, f2s, 12, 32, camera=sc.cam, seed=1, iteration=n, world_size=W, rank=rank,
                                              current_count=cnt, num_frames=nf)
                r._count_training_iteration(t.field_ids, t.count)
        n = bands.check()
    assert n > 40


# ------------------------------------------------------------------------------------------------ 6. two ranks
TWO = dict(N=24, T=6, R=16, SEED=11, FRAMES=2, PER_FRAME=3)
ROWS = ("ijs", "c2ws", "near_distances", "far_distances", "gt_distances", "field_ids", "rgbds", "rgb_mask", "depth_mask",
        "term_probs", "term_mask")


def _two_frames():
    return Frames(num_fields=TWO["N"], behind=3, aside=3)


def _two_worker(rank, world, port, out):
    import torch.distributed as dist
    from neural_graph_mapping_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    D.init_from_env(backend="gloo")
    F = _two_frames()
    r = renderer(F.positions, M1, trained=True)
    r.process_group = dist.group.WORLD
    r.peer_exchange = D.PeerExchange(dist.group.WORLD, timeout_s=20.0)
    r.track_training_iterations = True
    st = F.store()
    ids_buf = torch.full((TWO["N"],), -1, dtype=torch.int64, device=DEV)
    cnt_buf = torch.zeros(1, dtype=torch.int32, device=DEV)
    step, rows, graphs = None, [], []
    for f in range(TWO["FRAMES"]):
        F.advance(st, f)
        r.observed_fields_device(st.nc_rgbd[0], dev(F.frames[f]["c2w"]), num_points=S.GRAPH_POINTS, seed=S.SEED, frame=f,
                                 out=(ids_buf, cnt_buf), camera=F.cam)
        if step is None:
            step = r.capture_training(ids_buf, st.c_c2w, st.nc_rgbd, st.frame_cid_to_ncid, TWO["T"], TWO["R"], seed=TWO["SEED"],
                                      camera=F.cam, world_size=world, rank=rank, current_count=cnt_buf, num_frames=st.num_frames)
        for _ in range(TWO["PER_FRAME"]):
            step()
            graphs.append(step.graph)
            k = int(step.target.count)
            rows.append({q: getattr(step.target, q)[:k].cpu().clone() for q in ROWS})
    torch.cuda.synchronize()
    rec = dict(rows=rows, one_graph=isinstance(step.graph, torch.cuda.CUDAGraph) and all(g is step.graph for g in graphs),
               status=r.peer_exchange.status(), it_dev=int(r._target_iter_dev), step_dev=int(r._step_dev),
               training_iterations=r._global_map_dict["training_iterations"].cpu())
    torch.save(rec, os.path.join(out, f"live{rank}.pt"))
    dist.barrier()
    r.peer_exchange.close()
    dist.destroy_process_group()


def test_two_ranks_live_capture(tmp_path):
    """Each rank captures capture_training(world_size=2, rank=r, current_count=, num_frames=) once, with the peer exchange
    inside the graph, and replays it over 2 frames x 3 iterations while the observed set and the store change; each rank's
    rows are bit for bit the single-process sampler's rows of its fields."""
    import torch.multiprocessing as mp
    from test_gpu_device_iteration import _free_port
    world = 2
    ctxm = mp.spawn(_two_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=False)
    deadline = time.monotonic() + 240.0                 # the ranks under a time limit: never wait on a hung exchange
    while not ctxm.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctxm.processes:
                p.kill()
            raise AssertionError("a rank did not finish within its time limit")
    F = _two_frames()
    r = renderer(F.positions, SMALL)
    st = F.store()
    full = []
    for f in range(TWO["FRAMES"]):
        F.advance(st, f)
        ids, cnt = r.observed_fields_device(st.nc_rgbd[0], dev(F.frames[f]["c2w"]), num_points=S.GRAPH_POINTS, seed=S.SEED, frame=f,
                                            camera=F.cam)
        n, m = int(cnt), st.count
        for _ in range(TWO["PER_FRAME"]):
            t = r.sample_target_mv_device(ids[:n].contiguous(), st.c_c2w[:m].contiguous(), st.nc_rgbd, st.frame_cid_to_ncid[:m].contiguous(),
                                          TWO["T"], TWO["R"], camera=F.cam, seed=TWO["SEED"], iteration=len(full)).materialize()
            full.append({q: getattr(t, q).cpu() for q in ROWS})
    total = 0
    for rank in range(world):
        res = torch.load(os.path.join(tmp_path, f"live{rank}.pt"))
        assert res["one_graph"] and res["status"] == 0
        assert res["it_dev"] == res["step_dev"] == TWO["FRAMES"] * TWO["PER_FRAME"] == len(res["rows"])
        tally = torch.zeros(TWO["N"], dtype=torch.int64)
        for i, rows in enumerate(res["rows"]):
            sel = full[i]["field_ids"] % world == rank
            for q in ROWS:
                assert torch.equal(rows[q], full[i][q][sel]), (rank, i, q)
            tally[rows["field_ids"]] += 1
            total += int(sel.sum())
        assert torch.equal(res["training_iterations"], tally)
    assert total == sum(len(x["field_ids"]) for x in full) > 0
